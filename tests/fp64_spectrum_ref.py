"""The radial spectrum restated cell by cell in float64, the yardstick it is judged by, and the test fields (shared by
tests/test_spectra_cpu.py and tests/test_gpu_spectra.py).

``rapsd64`` is the definition with nothing clever in it: the full transform in float64, one boolean mask per r, no half-spectrum
shortcut, no mean removal.  ``rapsd_yardstick`` is the same thing with the transform alone done by torch.fft in float32 on the CPU --
what a careful user of the vendor route gets.  A spectrum S passes against the float64 S64 if its error is at most
``4 * max(error of the yardstick, 16 * 2^-24)`` in the field's measure:

* ``e_log = max_r |log(S_r / S64_r)|`` where every kept bin has power,
* ``e_abs = max_r |S_r - S64_r| / max_r S64_r`` for the sparse fields (an impulse's bins are all equal; a wave's are empty but one;
  ``abs_scale``: what stands in for the denominator when a wave lies in no bin at all).

The factor: a plain radix-2 fp32 transform with mean removal, modelled in NumPy, landed between 0.12 x and 1.8 x the yardstick over white
and power-law fields at the five kernel sizes; another radix and summation order can cost a further factor of two.  The floor: the
yardstick can be lucky (the smallest e_log seen was 4.7e-8), and 16 ulp of fp32 is what ~log2(N^2) butterfly levels may cost anyone.
"""
import math

import numpy as np
import torch

FLOOR = 16.0 * 2.0 ** -24
FACTOR = 4.0


def centred(n):
    """the integer wavenumbers in the transform's own (unshifted) order: 0, 1, ..., then the negative ones"""
    k = np.arange(n)
    return np.where(k < (n + 1) // 2, k, k - n) if n % 2 else np.where(k < n // 2, k, k - n)


def radius(m, n):
    ku, kv = centred(m), centred(n)
    return np.rint(np.sqrt((ku[:, None] ** 2 + kv[None, :] ** 2).astype(np.float64))).astype(np.int64)


def n_bins(m, n):
    l = max(m, n)
    return l // 2 if l % 2 == 0 else l // 2 + 1


def bin_counts(m, n):
    r = radius(m, n)
    return np.array([(r == k).sum() for k in range(n_bins(m, n))])


def _bin_means(P):
    m, n = P.shape[-2:]
    r = radius(m, n)
    return np.stack([P[..., r == k].mean(axis=-1) for k in range(n_bins(m, n))], axis=-1)


def rapsd64(x, normalize=False):
    """x (..., m, n) array-like -> (..., R) float64"""
    x = np.asarray(x, dtype=np.float64)
    m, n = x.shape[-2:]
    S = _bin_means(np.abs(np.fft.fft2(x)) ** 2 / (m * n))
    return S / S.sum(axis=-1, keepdims=True) if normalize else S


def rapsd_yardstick(x, demean=False):
    """the transform in float32 (torch.fft, CPU), power and bin means in float64.  ``demean``: the careful user's variant -- the float64
    mean taken off before the transform and bin 0, the cell P[0][0] alone, formed from the float64 sum."""
    x64 = np.asarray(x, dtype=np.float64)
    m, n = x64.shape[-2:]
    total = x64.sum(axis=(-2, -1))
    if demean:
        x64 = x64 - total[..., None, None] / (m * n)
    z = torch.fft.fft2(torch.as_tensor(x64.astype(np.float32))).numpy()
    S = _bin_means((z.real.astype(np.float64) ** 2 + z.imag.astype(np.float64) ** 2) / (m * n))
    if demean:
        S[..., 0] = total * total / (m * n)
    return S


def e_log(S, S64):
    return np.abs(np.log(np.asarray(S, dtype=np.float64) / S64)).max(axis=-1)


def abs_scale(x, S64):
    """max_r S64_r -- except for a field whose power lies in no bin (a wave on the Nyquist row), where that is rounding noise and no
    scale at all.  There the scale is the largest cell power over the largest bin's cell count: what the most diluted misplaced cell would
    add to a bin.  For every field with its power inside a bin this is below max_r S64_r, and the measure is the plain one."""
    x = np.asarray(x, dtype=np.float64)
    m, n = x.shape[-2:]
    cell = (np.abs(np.fft.fft2(x)) ** 2 / (m * n)).max(axis=(-2, -1))
    return np.maximum(S64.max(axis=-1), cell / bin_counts(m, n).max())


def e_abs(S, S64, x):
    return np.abs(np.asarray(S, dtype=np.float64) - S64).max(axis=-1) / abs_scale(x, S64)


def bound_log(x, S64):
    """per field: FACTOR * max(the yardstick's error on this very field, FLOOR).  The yardstick's error is the smaller of its two variants'
    (never a wider bound than the plain one gives): on a field like 1e-2 of noise on a mean of 1e3 the plain transform is off by percents,
    and a bound from it would let a kernel without mean removal through."""
    y = np.minimum(e_log(rapsd_yardstick(x), S64), e_log(rapsd_yardstick(x, demean=True), S64))
    return FACTOR * np.maximum(y, FLOOR)


def bound_abs(x, S64):
    y = np.minimum(e_abs(rapsd_yardstick(x), S64, x), e_abs(rapsd_yardstick(x, demean=True), S64, x))
    return FACTOR * np.maximum(y, FLOOR)


def rapsd_half64(x):
    """float64 through the half spectrum kv = 0 .. N/2 - 1 of a square even field, kv = 0 once and kv >= 1 twice, the Nyquist row and
    column left out -- the shortcut the kernel takes, for the test that it equals the cell-by-cell definition"""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[-1]
    assert x.shape[-2] == N and N % 2 == 0
    P = np.abs(np.fft.fft2(x)) ** 2 / (N * N)
    r = radius(N, N)
    out = np.zeros(x.shape[:-2] + (N // 2,))
    for k in range(N // 2):
        num, den = 0.0, 0
        for u in range(N):
            if u == N // 2:
                continue
            for v in range(N // 2):
                if r[u, v] == k:
                    w = 1 if v == 0 else 2
                    num, den = num + w * P[..., u, v], den + w
        out[..., k] = num / den
    return out


# ------------------------------------------------------------------------------------------------------------------ melr, line by line

def melr_reference(sample_rapsd_over_time, gt_rapsd_over_time, do_weighted=False, do_max=False):
    """exp/metrics.py:157-181 restated: loops over time and member, NumPy float64"""
    s, g = np.asarray(sample_rapsd_over_time, dtype=np.float64), np.asarray(gt_rapsd_over_time, dtype=np.float64)
    n_members, T, num_wave = s.shape
    over_time = []
    for t in range(T):
        if do_max:
            idx = np.argmax(g[t])
        elif do_weighted:
            weights = g[t] / np.sum(g[t])
        else:
            weights = np.full_like(g[t], 1 / num_wave)
        per_member = []
        for i in range(n_members):
            ratio = np.abs(np.log(s[i, t] / g[t]))
            per_member.append(ratio[idx] if do_max else np.sum(ratio * weights))
        over_time.append(np.array(per_member))
    return np.stack(over_time, axis=1).mean(axis=1)


# ------------------------------------------------------------------------------------------------------------------ fields

def white(N, seed, mean=0.5, amp=1.0):
    return (mean + amp * np.random.default_rng(seed).standard_normal((N, N))).astype(np.float32)


def power_law(N, seed, slope=-2.5):
    """amplitude |k|^slope with random phases: the dynamic range of the power is near 1e10 at N = 128"""
    rng = np.random.default_rng(seed)
    ku = centred(N)
    k = np.sqrt((ku[:, None] ** 2 + ku[None, :] ** 2).astype(np.float64))
    k[0, 0] = 1.0
    z = (rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))) * k ** slope
    return np.real(np.fft.ifft2(z) * N * N).astype(np.float32)


def impulse(N, i=3, j=5):
    x = np.zeros((N, N), dtype=np.float32)
    x[i % N, j % N] = 1.0
    return x


def plane_wave(N, a, b):
    i = np.arange(N)
    return np.cos(2.0 * math.pi * (a * i[:, None] + b * i[None, :]) / N).astype(np.float32)


def dense_fields(N, seed=0):
    """name -> field with power in every bin (measure e_log)"""
    return {"white_mean_half": white(N, seed + 1), "power_law": power_law(N, seed + 2), "small_on_1e3": white(N, seed + 3, mean=1e3, amp=1e-2)}


def sparse_fields(N):
    """name -> field with empty or equal bins (measure e_abs)"""
    return {"impulse": impulse(N), "constant": np.full((N, N), 0.75, dtype=np.float32), "wave_1_2": plane_wave(N, 1, 2),
            "wave_nyquist_row": plane_wave(N, N // 2, 0), "wave_hi_row": plane_wave(N, N // 2 - 1, 0),
            "wave_hi_col": plane_wave(N, 0, N // 2 - 1), "wave_nyq_3": plane_wave(N, -N // 2, 3)}
