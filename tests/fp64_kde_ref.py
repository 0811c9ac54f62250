"""The Gaussian kernel density estimate and the rank histogram restated in float64, the rule a density entry is judged by, and the test
fields (shared by tests/test_kde_cpu.py and tests/test_gpu_kde.py).

The definitions (include/c2w_hip.h: c2w_kde_eval, c2w_pit_counts), line by line:

    h = factor * std(x, ddof=1), factor = n^(-1/5) | (3 n / 4)^(-1/5) | the number given                  ``factor``, ``bandwidths``
    f(g) = (1 / (n h sqrt(2 pi))) * sum_i exp(-(g - x_i)^2 / (2 h^2))                                      ``kde64``
    grid = linspace(min(truth.min, samples.min), max(truth.max, samples.max), N) per variable             ``grid64``
    r = #{m : sample_m <= truth} per (time, variable, cell); counts[f][r]                                ``pit64``

The rule is the project's (tests/fp64_swd_ref.py: FACTOR = 4, 16 ulp, U = 2^-24) with a density's scale.  An entry passes if

    |got - f64| <= FACTOR * max(yardstick error, floor)                                                   ``bound``

* ``f64``: the formula in float64 on the same fp32 values, with the float64 grid and the float64 h;
* the yardstick: the pivoted fp32 torch route -- torch.exp of the same x - c and grid offsets, summed in fp32 per 256 values, the block
  sums folded in float64                                                                                  ``yardstick32``
* floor_j = 16 U * (1 / (n h sqrt(2 pi))) * sum_i (1 + u_ij^2) exp(-u_ij^2 / 2) + 2^-126 / (h sqrt(2 pi)): the first term is what a
  relative U in u does to a term ((d/du) exp(-u^2 / 2) = -u exp, times U u, plus the term's own rounding), the second covers terms
  below the smallest normal fp32, which the exponential instruction flushes to zero.

``naive32`` is the port that is NOT careful -- the float64 grid rounded to fp32 and g - x formed on the raw values, no pivot -- the
negative control, which the rule must refuse on the pressure kind once h is small enough (h shrinks as n^(-1/5)).
"""
import math

import numpy as np
import torch

from fp64_swd_ref import FACTOR, FLOOR, U  # noqa: F401  (4, 16 * 2^-24, 2^-24)

SQRT_2PI = math.sqrt(2.0 * math.pi)
KINDS = ("pressure", "temperature", "wind", "white")
VALUE_BLOCK = 2048  # values per block of the float64 passes


# ------------------------------------------------------------------------------------------------------------------ the definition

def factor(n, bw_method="scott"):
    if bw_method in (None, "scott"):
        return n ** -0.2
    if bw_method == "silverman":
        return (0.75 * n) ** -0.2
    return float(bw_method)


def data_sets(samples, truth=None):
    """samples (n_rep, T, F, hw) and truth (T, F, hw) -> [(variable, values (n,) fp32)] in the launch's order: member-major, then truth"""
    n_rep, T, F, hw = samples.shape
    out = [(f, np.ascontiguousarray(samples[r, :, f]).reshape(-1)) for r in range(n_rep) for f in range(F)]
    if truth is not None:
        out += [(f, np.ascontiguousarray(truth[:, f]).reshape(-1)) for f in range(F)]
    return out


def bandwidths(samples, truth=None, bw_method="scott"):
    """(D,) float64"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.array([factor(v.size, bw_method) * np.std(v.astype(np.float64), ddof=1) for _, v in data_sets(samples, truth)])


def grid64(samples, truth, N):
    """(F, N) float64: exp/figures.py:52-60"""
    F = truth.shape[1]
    return np.stack([np.linspace(min(truth[:, f].min().item(), samples[:, :, f].min().item()),
                                 max(truth[:, f].max().item(), samples[:, :, f].max().item()), N) for f in range(F)])


def kde64(v, g, h):
    """values v (n,) fp32, grid g (N,) float64, bandwidth h -> (density (N,), floor (N,)) in float64"""
    v, g = np.asarray(v, dtype=np.float64), np.asarray(g, dtype=np.float64)
    n = v.size
    s, w = np.zeros(g.size), np.zeros(g.size)
    for i in range(0, n, VALUE_BLOCK):
        u2 = ((g[None, :] - v[i:i + VALUE_BLOCK, None]) / h) ** 2
        e = np.exp(-0.5 * u2)
        s += e.sum(axis=0)
        w += ((1.0 + u2) * e).sum(axis=0)
    norm = 1.0 / (n * h * SQRT_2PI)
    return s * norm, FLOOR * norm * w + 2.0 ** -126 / (h * SQRT_2PI)


def pivot_and_offsets(g):
    """the fp32 pivot near the middle of the grid and the grid as fp32 offsets from it, computed in float64 and rounded once"""
    c = np.float32(0.5 * (g[0] + g[-1]))
    return c, (np.asarray(g, dtype=np.float64) - np.float64(c)).astype(np.float32)


def _sum_per_256(e):
    """e (n, N) fp32 torch -> (N,) float64: fp32 sums of 256 values each, folded in float64"""
    n = e.shape[0]
    full = n // 256 * 256
    s = e[:full].view(-1, 256, e.shape[1]).sum(dim=1).double().sum(dim=0) if full else torch.zeros(e.shape[1], dtype=torch.float64)
    if full < n:
        s = s + e[full:].sum(dim=0).double()
    return s.numpy()


def yardstick32(v, g, h):
    """the pivoted fp32 torch route: x - c and the offsets in fp32, u = (o - (x - c)) / h and torch.exp(-u^2 / 2) in fp32"""
    c, off = pivot_and_offsets(g)
    xo = torch.from_numpy(np.asarray(v, dtype=np.float32) - c)
    u = (torch.from_numpy(off)[None, :] - xo[:, None]) / torch.tensor(np.float32(h))
    e = torch.exp(-0.5 * u * u)
    assert e.dtype == torch.float32
    return _sum_per_256(e) / (v.size * h * SQRT_2PI)


def naive32(v, g, h):
    """the straight fp32 port: the grid rounded to fp32, g - x on the raw values, no pivot; summed as the yardstick is"""
    u = (torch.from_numpy(np.asarray(g).astype(np.float32))[None, :] - torch.from_numpy(np.asarray(v, dtype=np.float32))[:, None]) / torch.tensor(np.float32(h))
    e = torch.exp(-0.5 * u * u)
    assert e.dtype == torch.float32
    return _sum_per_256(e) / (v.size * h * SQRT_2PI)


def bound(v, g, h, f64=None, floor=None):
    """FACTOR * max(the yardstick's error on the entry, the floor), per entry; -> (f64, bound)"""
    if f64 is None:
        f64, floor = kde64(v, g, h)
    return f64, FACTOR * np.maximum(np.abs(yardstick32(v, g, h) - f64), floor)


_REF = {}


def reference(kind, n_rep, T, F, hw, N, seed=0):
    """(samples, truth, grid (F, N), h (D,), f64 (D, N), bound (D, N)) of the fields of `kind`, computed once per key, shared by the
    tests that need it and left unchanged"""
    key = (kind, n_rep, T, F, hw, N, seed)
    if key not in _REF:
        s, t = fields(kind, n_rep, T, F, hw, seed)
        g, h = grid64(s, t, N), bandwidths(s, t)
        rows = [bound(v, g[f], h[i]) for i, (f, v) in enumerate(data_sets(s, t))]
        out = (s, t, g, h, np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]))
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def worst(got, f64, b):
    """the largest error over max(yardstick error, floor) (the limit is FACTOR) and whether every entry passes"""
    e = np.abs(np.asarray(got) - f64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = float(np.nanmax(np.where(b > 0, e / (b / FACTOR), 0.0)))
    return ratio, bool(np.all(e <= b))


# ------------------------------------------------------------------------------------------------------------------ the rank histogram

def pit64(samples, truth):
    """samples (M, T, F, ...), truth (T, F, ...) -> counts (F, M + 1) int64: exp/figures.py:86 and a count of each value of the sum"""
    M, F = samples.shape[0], truth.shape[1]
    with np.errstate(invalid="ignore"):
        r = ((samples - truth[None]) <= 0).sum(axis=0)
    return np.stack([np.bincount(r[:, f].reshape(-1), minlength=M + 1) for f in range(F)]).astype(np.int64)


def pit_histogram_reference(samples, truth):
    """exp/figures.py:86 and :179-190 line by line, per variable: the density=True histogram of the PIT values over the reference's bins"""
    num_samples, F = samples.shape[0], truth.shape[1]
    with np.errstate(invalid="ignore"):
        pmf = ((samples.astype(np.float64) - truth.astype(np.float64)[None]) <= 0).sum(axis=0) / num_samples
    bins = np.linspace(-1 / (2 * num_samples), (1 / (2 * num_samples)) + 1, num_samples + 2, endpoint=True)
    per = [np.histogram(pmf[:, f].flatten(), bins=bins, density=True)[0] for f in range(F)]
    allvars_values = np.concatenate([pmf[:, f].flatten() for f in range(F)])
    return np.stack(per), np.histogram(allvars_values, bins=bins, density=True)[0]


# ------------------------------------------------------------------------------------------------------------------ fields

def fields(kind, n_rep, T, F, hw, seed=0):
    """(samples (n_rep, T, F, hw) fp32, truth (T, F, hw) fp32), de-normalised; variable f differs from its neighbours in offset and
    spread, so a wrong i % F shows; the members are a little wider than the truth and shifted, as an ensemble is"""
    rng = np.random.default_rng(seed + 7919 * KINDS.index(kind) + hw + 31 * T + 977 * n_rep)
    f = np.arange(F, dtype=np.float64)[:, None]
    off, sd = {"pressure": (101325.0 - 300.0 * f, 1200.0 * (1.0 + 0.2 * f)), "temperature": (280.0 + 5.0 * f, 10.0 + 2.0 * f),
               "wind": (2.0 - f, 4.0 * (1.0 + 0.5 * f)), "white": (f, 1.0 + f)}[kind]
    truth = off + sd * rng.standard_normal((T, F, hw))
    samples = off + 0.1 * sd + 1.15 * sd * rng.standard_normal((n_rep, T, F, hw))
    return samples.astype(np.float32), truth.astype(np.float32)
