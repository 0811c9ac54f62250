"""The training run's noise stream, defined independently of the kernels and of tests/emu_eval_ops.py: Philox4x32-10 (Salmon, Moraes,
Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 library) in numpy uint64 arithmetic, and the Box-Muller
transform of csrc/philox.h in float64.

The stream (csrc/philox.h):  element e is lane e & 3 of block e >> 2; the block's counter is (blk & 0xffffffff, blk >> 32, 0, 0), the
key (seed & 0xffffffff, seed >> 32); each of the four output words c becomes u = ((float)(c >> 8) + 0.5f) * 2^-24 IN FLOAT32 -- the
sum rounds to even once c >> 8 >= 2^23, and c >> 8 == 2^24 - 1 gives u == 1.0: that rounding is part of the stream's definition, and
numpy float32 reproduces it bit for bit -- and the lanes are (ra cos a, ra sin a, rb cos b, rb sin b) with ra = sqrt(-2 ln u0),
a = 2 pi u1, rb = sqrt(-2 ln u2), b = 2 pi u3.  Here everything after u runs in float64, so what a kernel's float32 __logf / sqrtf /
__sincosf add is its distance from normal_stream: STREAM_ERR below, measured once on an MI355X.

The keyword arguments of normal_stream plant the defects a wrong generator could have (tests/test_gpu_noise_stream.py); the second
half of the module restates, with fp64_ref's V arithmetic, the kernels that consume the stream (csrc/pointwise.hip).
"""
from __future__ import annotations

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)  # the two multipliers of Philox4x32
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85                          # the key schedule (golden ratio, sqrt(3) - 1)

# max |c2w_philox_normal - normal_stream| over the seven seeds of tests/test_gpu_noise_stream.py (n = 1 000 003 each), measured on an
# MI355X: see STREAM_ERR_BY_SEED in that file.  STREAM_TOL = 4 x that is what every comparison with this reference allows the stream.
STREAM_ERR = 1.828193e-06
STREAM_TOL = 4.0 * STREAM_ERR
STREAM_TOL_CAP = 2.0 ** -11  # half a half-precision step for 1 <= |z| < 2: the asserted tolerance may never exceed it


def philox4x32_10(counter4, key2):
    """Ten rounds of Philox4x32: counter4 = four arrays (or ints) of 32-bit words, key2 = two ints.  Returns the four output words
    as uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(w, dtype=np.uint64) & M32 for w in counter4])
    k0, k1 = int(key2[0]) & 0xFFFFFFFF, int(key2[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2  # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & M32, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & 0xFFFFFFFF, (k1 + PHILOX_W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def uniform_f32(c):
    """u of one output word, in float32 exactly as the kernel computes it (0 < u <= 1)"""
    return ((np.asarray(c, dtype=np.uint64) >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def box_muller(words, swap_trig=False):
    """(n, 4) float64 lanes of blocks whose four output words are `words`"""
    u0, u1, u2, u3 = (uniform_f32(c).astype(np.float64) for c in words)
    ra, rb = np.sqrt(-2.0 * np.log(u0)), np.sqrt(-2.0 * np.log(u2))
    a, b = 2.0 * np.pi * u1, 2.0 * np.pi * u3
    first, second = (np.sin, np.cos) if swap_trig else (np.cos, np.sin)
    return np.stack((ra * first(a), ra * second(a), rb * first(b), rb * second(b)), axis=-1)


def _blocks(n, first):
    b0 = first >> 2
    return b0, np.arange(b0, ((first + n + 3) >> 2), dtype=np.uint64)


def normal_stream(n, seed, first=0, *, swap_key=False, block_shift=0, lanes=(0, 1, 2, 3), swap_trig=False):
    """Elements first .. first + n - 1 of the stream of `seed`, float64.
    The keywords plant defects: key words swapped, the counter `block_shift` blocks ahead, the lanes of every block permuted, cos and
    sin exchanged."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (seed & 0xFFFFFFFF, seed >> 32)
    b0, blk = _blocks(n, first)
    blk = blk + np.uint64(block_shift)
    words = philox4x32_10((blk & M32, blk >> S32, 0, 0), key[::-1] if swap_key else key)
    z = box_muller(words, swap_trig)[:, list(lanes)].reshape(-1)
    return z[first - 4 * b0: first - 4 * b0 + n]


def unit_u0_mask(n, seed, first=0):
    """True where the element's radius comes from a u that rounded to exactly 1.0 (lanes 0, 1: u0; lanes 2, 3: u2)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    b0, blk = _blocks(n, first)
    c0, _, c2, _ = philox4x32_10((blk & M32, blk >> S32, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
    ua, ub = uniform_f32(c0) == np.float32(1.0), uniform_f32(c2) == np.float32(1.0)
    m = np.stack((ua, ua, ub, ub), axis=-1).reshape(-1)
    return m[first - 4 * b0: first - 4 * b0 + n]


# ------------------------------------------------------------------------------------------- the kernels that consume the stream

def eps_nchw(B, C, HW, seed, device, **defect):
    """(B, C, HW) float64 torch tensor: the dense stream the consumers address with ((b * C + c) * HW + pixel)"""
    import torch
    return torch.from_numpy(normal_stream(B * C * HW, seed, **defect)).view(B, C, HW).to(device)


def _to_rows(t):
    """(B, C, HW) -> NHWC rows (B * HW, C)"""
    B, C, HW = t.shape
    return t.permute(0, 2, 1).reshape(B * HW, C)


def xt_rows(x, eps, musig, dtype, eps_tol=0.0):
    """The live channels of c2w_nchw_to_nhwc(eps) / c2w_nchw_to_nhwc_noise / c2w_windows_to_nhwc_noise as V rows (B * HW, C).

    x (B, C, HW) fp32; eps (B, C, HW): the fp32 tensor the kernel read (eps_tol = 0) or the float64 stream (eps_tol = STREAM_TOL: the
    kernel's own eps is that far from it at most, which moves the result by |sigma| eps_tol); musig (B, 2) fp32.
    Every route (pointwise.hip: Ld::mix of the tiled kernels, nchw_to_nhwc_kernel, nchw_to_nhwc_eps_kernel) computes
    fma(sigma, eps, mul_rn(mu, x)): the product mu x rounds, the fma rounds -- two fp32 roundings.  Then the storage rounding."""
    import fp64_ref as R
    B, C, HW = x.shape
    mu = musig[:, 0].to(R.D).view(B, 1, 1)
    sg = musig[:, 1].to(R.D).view(B, 1, 1)
    p, q = mu * x.to(R.D), sg * eps.to(R.D)
    v = p + q
    e = sg.abs() * eps_tol + R.U32 * p.abs()
    e = e + R.U32 * (v.abs() + e)
    return R._rnd(R.V(_to_rows(v), _to_rows(e.expand_as(v))), dtype)


def mse_dy_rows(y, eps, B, C, HW, ldc, gscale, dtype, eps_tol):
    """fp64_ref.mse_dy with eps the float64 stream and the kernel's own eps within eps_tol of it: live channels only, V rows (B * HW, C)"""
    import fp64_ref as R
    e = _to_rows(eps.to(R.D))
    d = R._sub(R.exact(R._rows(y, B * HW, ldc)[:, :C]), R.V(e, e.new_full(e.shape, eps_tol)))
    return R._rnd(R._scale(d, gscale), dtype)


def sq_err_planes(y, eps, B, C, HW, ldc, eps_tol):
    """sq_err_tiled_kernel against the float64 stream: out = (y - eps)^2 as V (B, C, HW): a subtraction and a product, both rounded,
    of a y that is exact and an eps within eps_tol"""
    import fp64_ref as R
    yv = R._rows(y, B * HW, ldc)[:, :C].to(R.D).view(B, HW, C).permute(0, 2, 1)
    e = eps.to(R.D)
    d = R._sub(R.V(yv), R.V(e, e.new_full(e.shape, eps_tol)))
    return R._mul(d, d)
