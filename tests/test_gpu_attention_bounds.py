"""Element-wise float64 bounds (tests/fp64_ref.py, attention section) for the attention kernels, on all three routes:

  VALU    attention.hip: fp32 P / dP / dS in LDS, expf; fp32 always, 16-bit where the matrix-core rule does not hold or C2W_ATTN_VALU=1
  T64     attention_mfma.hip:116-232: T = 64, one workgroup per image, P normalised then rounded, delta inside the kernel
  BLOCKS  attention_mfma.hip:238-463: T = 64 n, online softmax over key blocks, two-kernel block backward, delta from rowdot

Every case: forward (o, lse within their bounds), then the backward twice -- on the fp32 emulation's o / lse (what the parity tests
feed it) and on the forward kernel's own outputs (what the engine feeds it) -- dq, dk, dv each against their own bound, the delta
workspace against rowdot's where the route fills it.  Every output buffer is pre-filled with a sentinel and carries a guard row before
and after, checked untouched.  At (3, 64, 512), (2, 256, 512) and (2, 64, 16) the planted defects of attention_cases.attention_defect are put on the
kernel's own output and must be rejected.  The float64 references run on the GPU through torch.

Largest err / bound observed on an MI355X, per route (forward o / lse; backward dq / dk / dv, the larger of the two input kinds;
delta where the route fills it), and the case it came from:
  T64    16-bit  o 0.841 ((128, 64, 512) bf16 randn)   lse 0.030   dq 0.837 ((128, 64, 512) bf16 randn)   dk 0.823   dv 0.903 ((3, 64, 512) bf16 peaked)
  BLOCKS 16-bit  o 0.712   lse 0.036   dq 0.986   dk 0.977   dv 0.858 (all (2, 256, 512) bf16 peaked)   delta 0.060
  VALU   16-bit  o 0.977   lse 0.117   dq 0.997   dk 0.994   dv 0.991 (all (2, 64, 16) bf16, randn / peaked)   delta 0.059
  VALU   fp32    o 0.039   lse 0.104   dq 0.124   dk 0.200 ((2, 256, 512) peaked)   dv 0.113   delta 0.084
The backward on the kernel's own outputs and on the emulated ones differ in the third digit at most.  The 16-bit figures near 1 are
the output's own rounding: u_T |v| is exactly half a spacing at the bottom of a binade, and where few keys carry the row (peaked; C = 16)
little else is in the bound; fp32 shows the slack of the K-sum rule (C_ACC).  The fp16 2^-12 gradient stays below 0.68 on the matrix
cores: their operands keep fp16 subnormals.  fp32 at (1, 1024, 512), the 160 KiB LDS request, launches and is within 0.05.  No kernel
defect was found.  The file runs in 7 s (105 cases); tests/test_gpu_kernels.py takes 23 s without its attention bounds, 26 s with them.
"""
import pytest
import torch

import attention_cases as A
import emu_ops as E
import fp64_ref as R
from climate2weather_amd import ops

pytestmark = pytest.mark.gpu

F32, BF16, F16 = ops.DTYPE_F32, ops.DTYPE_BF16, ops.DTYPE_F16
TD = ops.TORCH_DTYPE
NAME = {F32: "fp32", BF16: "bf16", F16: "fp16"}
SENTINEL = 777.0
SECTION = A.SECTION


def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _knobs_follow_the_environment():
    """monkeypatch restores the environment after a test; the library's knob table (read once) must follow."""
    yield
    ops.knobs_reload()


def guarded(rows, cols, dtype):
    """(buffer with one guard row before and after, the op's view of it), all sentinel"""
    buf = torch.full((rows + 2, cols) if cols else (rows + 2,), SENTINEL, dtype=dtype, device=dev())
    return buf, buf[1:-1]


def guards_untouched(buf, what):
    assert (buf[0] == SENTINEL).all() and (buf[-1] == SENTINEL).all(), f"{what}: a guard row was written"


def check_case(qkv, do, B, T, C, dt, route, tag, defects=False):
    d = dev()
    qkv, do = qkv.to(d), do.to(d)
    parts = R.attention_exact(qkv, B, T, C, do)
    obuf, o = guarded(B * T, C, TD[dt])
    lbuf, lse = guarded(B * T, 0, torch.float32)
    ops.attention_forward(qkv, o, lse, B, T, C, dt)
    guards_untouched(obuf, f"{tag} o")
    guards_untouched(lbuf, f"{tag} lse")
    ro, _ = A.forward_bounds(qkv, o, lse, B, T, C, dt, route, tag, parts)
    o_emu, lse_emu = torch.empty_like(o), torch.empty_like(lse)
    E.attention_forward(qkv, o_emu, lse_emu, B, T, C, dt)
    for kind, oi, li in (("backward on emulated inputs", o_emu, lse_emu), ("backward on own outputs", o, lse)):
        gbuf, dqkv = guarded(B * T, 3 * C, TD[dt])
        dbuf, delta = guarded(B * T, 0, torch.float32)
        ops.attention_backward(qkv, oi, do, li, delta, dqkv, B, T, C, dt)
        guards_untouched(gbuf, f"{tag} dqkv")
        guards_untouched(dbuf, f"{tag} delta")
        rg = A.backward_bounds(qkv, oi, do, li, dqkv, delta, B, T, C, dt, route, f"{tag} {kind}", parts)
    if not defects:
        return
    kinds = ["p_tile", "key", "delta_row", "ds_scale"] + (["dq_block"] if route == R.BLOCKS else [])
    if route == R.BLOCKS and "rising" in tag:
        kinds.append("alpha")  # defined where the maximum grows across the key blocks
    for kind in kinds:
        sec, term, where = A.attention_defect(kind, qkv, do, B, T, C, image=B - 1)
        if sec == "o":
            R.assert_rejects(o.double() + term, ro, what=f"{tag} {kind} ({where})")
        else:
            i = SECTION[sec]
            R.assert_rejects(dqkv[:, i * C:(i + 1) * C].double() + term, A.sect(rg, sec, C), what=f"{tag} {kind} ({where})")
    R.assert_rejects(A.stale_upper_half(dqkv, B, T, C, "v", image=B - 1), rg, what=f"{tag} upper half of dv stale")


SHAPES_T64 = [(3, 64, 32), (3, 64, 96), (3, 64, 160), (3, 64, 352), (3, 64, 480), (3, 64, 512), (128, 64, 512), (1, 64, 512)]
SHAPES_BLOCKS = [(2, 128, 32), (2, 192, 160), (2, 256, 384), (2, 256, 512), (1, 1024, 512), (1, 4096, 64)]
SHAPES_VALU = [(2, 64, 16), (2, 256, 16), (2, 4, 64), (3, 36, 64), (2, 100, 40), (2, 144, 512)]
DEFECT_SHAPES = {(3, 64, 512), (2, 256, 512), (2, 64, 16)}  # where the CPU tier shows every defect above the bound at every regime
REGIME_SHAPES = [(3, 64, 512), (2, 256, 512), (2, 64, 16)]  # T64, BLOCKS, VALU (the tiny test network's attention level)


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("shape", SHAPES_T64 + SHAPES_BLOCKS)
def test_matrix_core_routes(shape, dt):
    B, T, C = shape
    route = A.attn_route(B, T, C, dt)
    assert route == (R.T64 if T == 64 else R.BLOCKS)
    qkv, do = A.attention_inputs("randn", B, T, C, dt)
    check_case(qkv, do, B, T, C, dt, route, f"attention {shape} {NAME[dt]} randn {route}", defects=shape in DEFECT_SHAPES)


@pytest.mark.parametrize("dt", [F32, BF16, F16])
@pytest.mark.parametrize("shape", SHAPES_VALU)
def test_valu_route(shape, dt):
    B, T, C = shape
    assert A.attn_route(B, T, C, dt) == R.VALU
    qkv, do = A.attention_inputs("randn", B, T, C, dt)
    check_case(qkv, do, B, T, C, dt, R.VALU, f"attention {shape} {NAME[dt]} randn valu", defects=shape in DEFECT_SHAPES)


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("shape", [(3, 64, 512), (2, 256, 512)])
def test_valu_fallback_where_the_matrix_cores_would_run(shape, dt, monkeypatch):
    B, T, C = shape
    monkeypatch.setenv("C2W_ATTN_VALU", "1")
    ops.knobs_reload()
    qkv, do = A.attention_inputs("randn", B, T, C, dt)
    check_case(qkv, do, B, T, C, dt, A.attn_route(B, T, C, dt, valu_knob=True), f"attention {shape} {NAME[dt]} randn valu (knob)", defects=True)


def test_valu_fp32_backward_at_the_whole_lds():
    """(1, 1024, 512) in fp32: the backward's LDS request is (16 * 512 + 2 * 16 * 1024) * 4 = 160 KiB exactly (attention.hip:263-264),
    a supported shape by the library's own rule"""
    B, T, C = 1, 1024, 512
    qkv, do = A.attention_inputs("randn", B, T, C, F32)
    check_case(qkv, do, B, T, C, F32, R.VALU, f"attention {(B, T, C)} fp32 randn valu")


# fp32 runs on the VALU route only; the small gradient is the fp16 subnormal case
REGIME_CASES = [(s, r, dt) for s in REGIME_SHAPES for r in A.REGIMES[1:] for dt in (F32, BF16, F16)
                if (dt != F32 or A.attn_route(*s, dt) == R.VALU) and (r != "smallgrad" or dt == F16)]


@pytest.mark.parametrize("shape,regime,dt", REGIME_CASES)
def test_input_regimes(shape, regime, dt):
    B, T, C = shape
    route = A.attn_route(B, T, C, dt)
    qkv, do = A.attention_inputs(regime, B, T, C, dt)
    check_case(qkv, do, B, T, C, dt, route, f"attention {shape} {NAME[dt]} {regime} {route}", defects=True)


@pytest.mark.parametrize("dt", [F32, BF16, F16])  # fp32: the VALU route; 16-bit: T64 at the first shape, BLOCKS at the second
@pytest.mark.parametrize("shape", [(128, 64, 512), (2, 256, 512)])
def test_two_calls_are_bit_identical(shape, dt):
    """no atomics, bit-reproducible (attention.hip:6, attention_mfma.hip:13): two calls, forward and backward"""
    B, T, C = shape
    d = dev()
    qkv, do = (t.to(d) for t in A.attention_inputs("randn", B, T, C, dt))
    outs = []
    for _ in range(2):
        o, lse = torch.full((B * T, C), SENTINEL, dtype=TD[dt], device=d), torch.full((B * T,), SENTINEL, device=d)
        dqkv, delta = torch.full((B * T, 3 * C), SENTINEL, dtype=TD[dt], device=d), torch.full((B * T,), SENTINEL, device=d)
        ops.attention_forward(qkv, o, lse, B, T, C, dt)
        ops.attention_backward(qkv, o, do, lse, delta, dqkv, B, T, C, dt)
        outs.append((o, lse, dqkv, delta))
    for a, b, what in zip(outs[0], outs[1], ("o", "lse", "dqkv", "delta")):
        assert torch.equal(a, b), f"{what} differs between two calls"
