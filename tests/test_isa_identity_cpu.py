"""lab/isa_identity.py on synthetic assembly and remark text: it sees one changed mnemonic and one changed register count as exactly one
differing kernel each, and a shifted per-file function index in the local labels as none."""
import importlib.util
import io
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_identity", os.path.join(REPO, "lab", "isa_identity.py"))
isa_identity = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_identity)

UNIT = "toy"
KERNELS = ("_Z5alphaPf", "_Z4betaPf")


def _kernel(sym, idx, op="v_add_f32"):
    return f"""\t.section\t.text.{sym},"axG",@progbits,{sym},comdat
\t.globl\t{sym}
\t.p2align\t8
\t.type\t{sym},@function
{sym}:                                ; @{sym}
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_cbranch_scc1 .LBB{idx}_2
; %bb.1:                                ; %then
\t{op}_e32 v1, v0, v0
.LBB{idx}_2:                                ; %exit
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {sym}
\t\t.amdhsa_next_free_vgpr 2
\t\t.amdhsa_next_free_sgpr 6
\t.end_amdhsa_kernel
\t.section\t.text.{sym},"axG",@progbits,{sym},comdat
.Lfunc_end{idx}:
\t.size\t{sym}, .Lfunc_end{idx}-{sym}
                                        ; -- End function
"""


def _asm(first_index=0, ops=None):
    ops = ops or {}
    return "\t.text\n" + "".join(_kernel(s, first_index + i, ops.get(s, "v_add_f32")) for i, s in enumerate(KERNELS))


def _remarks(vgprs=None, line=10):
    vgprs = vgprs or {}
    out = []
    for i, s in enumerate(KERNELS):
        loc = f"remark: csrc/toy.hip:{line + i}:0:"
        tail = "[-Rpass-analysis=kernel-resource-usage]"
        out += [f"{loc} Function Name: {s} {tail}", f"{loc}     TotalSGPRs: 6 {tail}", f"{loc}     VGPRs: {vgprs.get(s, 2)} {tail}",
                f"{loc}     ScratchSize [bytes/lane]: 0 {tail}", f"{loc}     LDS Size [bytes/block]: 0 {tail}"]
    return "\n".join(out) + "\n"


def _write(build_dir, asm, remarks):
    tmp = os.path.join(build_dir, UNIT + ".tmp")
    os.makedirs(tmp)
    with open(os.path.join(tmp, f"{UNIT}-hip-amdgcn-amd-amdhsa-gfx950.s"), "w") as f:
        f.write(asm)
    with open(os.path.join(tmp, "resource_usage.txt"), "w") as f:
        f.write(remarks)


CASES = {
    # name: (assembly of the second build, remarks of the second build, differing symbols expected)
    "changed_mnemonic": (_asm(ops={"_Z4betaPf": "v_mul_f32"}), _remarks(), ["_Z4betaPf"]),
    "changed_vgpr_count": (_asm(), _remarks(vgprs={"_Z5alphaPf": 3}), ["_Z5alphaPf"]),
    # two functions in front of these disappeared (labels .LBB2_ -> .LBB0_) and the host code above them moved (remark line numbers)
    "shifted_label_index": (_asm(first_index=2), _remarks(line=40), []),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_isa_identity_reports_exactly_the_changed_kernel(case, tmp_path):
    asm_b, remarks_b, expected = CASES[case]
    r = isa_identity.compare_unit(_asm(), _remarks(), asm_b, remarks_b)
    assert (r["kernels_a"], r["kernels_b"], r["common"]) == (2, 2, 2) and r["added"] == [] and r["removed"] == []
    assert sorted(set(r["res_diff"]) | set(r["isa_diff"])) == expected
    # the same through the directory layout a build leaves, as the command line reads it
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _write(a, _asm(), _remarks())
    _write(b, asm_b, remarks_b)
    table = io.StringIO()
    assert isa_identity.report(a, b, out=table) == len(expected)
    assert f"## Differing symbols ({len(expected)})" in table.getvalue()
    assert f"| {UNIT} | 2 | 2 | 2 | " in table.getvalue()
