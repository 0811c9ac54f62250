"""Are the kernels of two builds the same machine code?

    python lab/isa_identity.py PARENT/climate2weather_amd/build CHANGE/climate2weather_amd/build > table.md

Each directory is what `python -m climate2weather_amd.build --force` leaves: per translation unit `<unit>.tmp/<unit>-hip-amdgcn-amd-amdhsa-gfx950.s`
(the device assembly that was assembled into the object) and `<unit>.tmp/resource_usage.txt` (the compiler's resource-usage remarks of the
same compilation).  For every function symbol the two builds are compared by

* the resource-usage record (SGPRs, VGPRs, AGPRs, scratch, occupancy, spills, LDS);
* the instruction stream from the symbol's `.type` line to its `.Lfunc_end`, comments and section / alignment directives dropped, the
  per-file function index in local labels normalised (`.LBB<n>_<k>` -> `.LBB#_<k>`, likewise `.Lfunc_begin/end<n>`, `.Ltmp<n>`,
  `.LJTI<n>_<k>`): that index shifts when a function in front of the others appears or disappears;
* the `.amdhsa_kernel` descriptor block.

Prints a markdown table per unit and the added / removed / differing symbols; exit status 1 unless all three lists are empty.
Standard library only.
"""
import os
import re
import sys

_FUNC = re.compile(r"^\s*\.type\s+(\S+),@function")
_END = re.compile(r"^\.Lfunc_end\d+:")
_LOCAL = re.compile(r"\.(LBB|Lfunc_begin|Lfunc_end|Ltmp|LJTI)\d+")
_DROP = re.compile(r"^\s*\.(section|p2align|text)\b")
_NAME = re.compile(r"Function Name: (\S+)")
_FIELD = re.compile(r"remark: [^ ]*\s+([A-Za-z][^:\[]*?)(?: \[[^\]]*\])?: (\S+) \[-Rpass")


def parse_asm(asm):
    """{symbol: (instruction lines, descriptor lines)}; the descriptor is empty for a device function that is no kernel."""
    out, name, code, desc, in_desc = {}, None, [], [], False
    for line in asm.splitlines():
        m = _FUNC.match(line)
        if m:
            name, code, desc, in_desc = m.group(1), [], [], False
            continue
        if name is None:
            continue
        if _END.match(line):
            out[name] = (code, desc)
            name = None
            continue
        line = line.split(";", 1)[0].rstrip()  # comments carry source paths and the compiler's own register statistics
        if not line.strip() or _DROP.match(line):
            continue
        line = _LOCAL.sub(lambda m: "." + m.group(1) + "#", line)
        if line.strip().startswith(".amdhsa_kernel"):
            in_desc = True
        (desc if in_desc else code).append(line.strip())
        if line.strip() == ".end_amdhsa_kernel":
            in_desc = False
    return out


def parse_remarks(text):
    """{symbol: {field: value}} from -Rpass-analysis=kernel-resource-usage output."""
    out, cur = {}, None
    for line in text.splitlines():
        m = _NAME.search(line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = _FIELD.match(line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


def compare_unit(asm_a, rem_a, asm_b, rem_b):
    """One translation unit: dict(kernels_a, kernels_b, common, lines, added, removed, res_diff, isa_diff) -- the last four are symbol lists."""
    fa, fb = parse_asm(asm_a), parse_asm(asm_b)
    ra, rb = parse_remarks(rem_a), parse_remarks(rem_b)
    ka, kb = {s for s, (_, d) in fa.items() if d}, {s for s, (_, d) in fb.items() if d}
    common = sorted(set(fa) & set(fb))
    return dict(kernels_a=len(ka), kernels_b=len(kb), common=len(ka & kb), lines=sum(len(fa[s][0]) for s in common),
                added=sorted(set(fb) - set(fa)), removed=sorted(set(fa) - set(fb)),
                res_diff=[s for s in common if ra.get(s) != rb.get(s)],
                isa_diff=[s for s in common if fa[s] != fb[s]])


def read_unit(build_dir, unit):
    tmp = os.path.join(build_dir, unit + ".tmp")
    with open(os.path.join(tmp, unit + "-hip-amdgcn-amd-amdhsa-gfx950.s")) as f:
        asm = f.read()
    with open(os.path.join(tmp, "resource_usage.txt")) as f:
        return asm, f.read()


def units_of(build_dir):
    return {d[:-4] for d in os.listdir(build_dir) if d.endswith(".tmp") and os.path.isdir(os.path.join(build_dir, d))}


def report(dir_a, dir_b, out=sys.stdout):
    """Writes the table; returns the number of added + removed + differing symbols (units present on one side only count as one each)."""
    ua, ub = units_of(dir_a), units_of(dir_b)
    rows, tot_a, tot_b, lines = [], 0, 0, 0
    added, removed, differing = [], [], []
    for unit in sorted(ua & ub):
        r = compare_unit(*read_unit(dir_a, unit), *read_unit(dir_b, unit))
        rows.append(f"| {unit} | {r['kernels_a']} | {r['kernels_b']} | {r['common']} | {len(r['res_diff'])} | {len(r['isa_diff'])} |")
        tot_a, tot_b, lines = tot_a + r["kernels_a"], tot_b + r["kernels_b"], lines + r["lines"]
        added += [(unit, s) for s in r["added"]]
        removed += [(unit, s) for s in r["removed"]]
        differing += [(unit, s) for s in sorted(set(r["res_diff"]) | set(r["isa_diff"]))]
    print("| unit | kernels parent | kernels change | common | resource records differing | instruction streams differing |", file=out)
    print("|---|---|---|---|---|---|", file=out)
    print("\n".join(rows), file=out)
    print(f"| total | {tot_a} | {tot_b} | | | |\n", file=out)
    print(f"translation units compared: {len(ua & ub)}; instruction lines compared over the common symbols: {lines}", file=out)
    only = sorted(ua ^ ub)
    if only:
        print(f"units present in one build only: {', '.join(only)}", file=out)
    for title, items in (("Added symbols", added), ("Removed symbols", removed), ("Differing symbols", differing)):
        print(f"\n## {title} ({len(items)})\n", file=out)
        print("\n".join(f"- {u}: `{s}`" for u, s in items) if items else "none", file=out)
    return len(added) + len(removed) + len(differing) + len(only)


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(1 if report(sys.argv[1], sys.argv[2]) else 0)
