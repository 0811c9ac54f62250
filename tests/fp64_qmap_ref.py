"""float64 references of the quantile mapping (climate2weather_amd.biascorrect), from numpy alone.

Nodes: ``numpy.nanquantile`` / ``numpy.quantile`` of the float64 series.  They are compared AS NUMBERS: NaN for NaN, a zero of either
sign.

Mapping: ``numpy.interp(x64, xq, yq)`` inside the range of strictly increasing nodes, and the stated tails outside.  The bound of the
kernel's arithmetic against it, derived: with ``d = x - xq_j``, ``s = (yq_{j+1} - yq_j) / (xq_{j+1} - xq_j)``, the kernel rounds four
times in float64 before the product (the two differences, the quotient, ``d``) and twice after (the product, the sum), numpy.interp as
often in its own order: each rounding moves the result by at most ``2^-53`` of ``|d s|`` or, the last one, of ``|yq_j| + |d s|``, so
the two differ by at most ``4 * 2^-53 (|yq_j| + |d s|)`` with room to spare; the clamp at ``yq_{j+1}`` only moves the kernel's value
towards the exact one.  Rounding to fp32 adds half an ulp, at most ``2^-24 |y|``, and ``2^-149`` where the result is denormal:

    |got - interp| <= 2^-24 |y| + 4 * 2^-53 (|yq_j| + |(x - xq_j) slope|) + 2^-149
"""
import warnings

import numpy as np

KINDS = ("pressure", "temperature", "wind", "ties", "zeros", "denormals", "inf", "nans")
EXACT_KINDS = ("pressure", "temperature", "wind")  # the kinds the exact answers of the mapping are stated for
F32 = np.float32


def fields(kind, n_rep, T, F, hw, seed=0):
    """(n_rep, T, F, hw) fp32.  Variable f differs from its neighbours in offset and scale, so a wrong index map fails."""
    rng = np.random.default_rng([seed, KINDS.index(kind), n_rep, T, F, hw])
    z = rng.standard_normal((n_rep, T, F, hw))
    f = np.arange(F).reshape(1, 1, F, 1)
    if kind == "pressure":
        x = 1.0e5 + 50.0 * f + (800.0 + 100.0 * f) * z
    elif kind == "temperature":
        x = 285.0 - 3.0 * f + (8.0 + f) * z
    elif kind == "wind":
        x = np.abs((4.0 + f) * z) + 0.01 * f
    elif kind == "ties":
        x = np.round(3.0 * z) + f  # a handful of distinct values: every node repeats
    elif kind == "zeros":
        x = np.where(rng.random(z.shape) < 0.5, np.where(z < 0, -0.0, 0.0), np.round(z) * (1.0 + f))  # both zeros among small integers
    elif kind == "denormals":
        x = z * 1.0e-41 * (1.0 + f)
    elif kind == "inf":
        x = 10.0 * z + f
        x = np.where(rng.random(z.shape) < 0.02, np.where(z < 0, -np.inf, np.inf), x)
    elif kind == "nans":
        x = 10.0 * z + 100.0 * f
    else:
        raise ValueError(kind)
    x = x.astype(F32)
    if kind == "nans":  # NaNs of both signs, a payload among them; series 0 of every variable keeps them all out of one corner
        bits = x.view(np.uint32).copy()
        hit = rng.random(z.shape) < 0.15
        bits[hit] = np.where(rng.random(int(hit.sum())) < 0.5, np.uint32(0x7FC00000), np.uint32(0xFFC00123))
        x = bits.view(F32)
    return np.ascontiguousarray(x)


def levels_of(K):
    """the K levels k / (K - 1), as biascorrect spells them"""
    return np.array([k / (K - 1) for k in range(K - 1)] + [1.0])


def index_lists(ids, G):
    return [[t for t, v in enumerate(ids) if v == g] for g in range(G)]


def nodes64(x, ids, G, levels, skipna=True):
    """x (n_rep, T, F, hw) fp32 -> (q (n_rep, G, F, hw, K) float64, n_valid (n_rep, G, F, hw) int64) by numpy"""
    n_rep, T, F, hw = x.shape
    levels = np.asarray(levels, np.float64)
    q = np.full((n_rep, G, F, hw, len(levels)), np.nan)
    nv = np.zeros((n_rep, G, F, hw), np.int64)
    fn = np.nanquantile if skipna else np.quantile
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for g, idx in enumerate(index_lists(ids, G)):
            if not idx:
                continue
            s = x[:, idx].astype(np.float64)  # (n_rep, n, F, hw)
            nan = np.isnan(s)
            q[:, g] = np.moveaxis((fn if nan.any() else np.quantile)(s, levels, axis=1), 0, -1)  # without a NaN the two are one function
            nv[:, g] = (~nan).sum(axis=1)
    return q, nv


def same_numbers(a, b):
    """equal as numbers: NaN for NaN, a zero of either sign"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def interp64(x, xq, yq, ids):
    """x (n_rep, T, F, hw) fp32, xq / yq (G, F, hw, K) float64 -> (y, allow) float64 of x's shape: numpy.interp per cell and group and
    the bound above; both NaN where x lies outside [xq_0, xq_{K-1}) or is NaN (the caller checks the tails by their own formula)"""
    n_rep, T, F, hw = x.shape
    G, K = xq.shape[0], xq.shape[-1]
    y, allow = np.full(x.shape, np.nan), np.full(x.shape, np.nan)
    for g, idx in enumerate(index_lists(ids, G)):
        if not idx:
            continue
        for f in range(F):
            for c in range(hw):
                a, b = xq[g, f, c], yq[g, f, c]
                v = x[:, idx, f, c].astype(np.float64)
                inside = (v >= a[0]) & (v < a[-1])
                j = np.clip(np.searchsorted(a, v, side="right") - 1, 0, K - 2)
                with np.errstate(all="ignore"):
                    yy = np.interp(v, a, b)
                    slope = (b[j + 1] - b[j]) / (a[j + 1] - a[j])
                    al = 2.0 ** -24 * np.abs(yy) + 4 * 2.0 ** -53 * (np.abs(b[j]) + np.abs((v - a[j]) * slope)) + 2.0 ** -149
                y[:, idx, f, c] = np.where(inside, yy, np.nan)
                allow[:, idx, f, c] = np.where(inside, al, np.nan)
    return y, allow


def tails64(x, xq, yq, ids):
    """(below, above, y) : where x < xq_0 / x >= xq_{K-1}, and the stated additive tail there (float64, then rounded once to fp32)"""
    gid = np.asarray(ids)
    lo, hi = xq[gid][..., 0], xq[gid][..., -1]                                   # (T, F, hw)
    dlo, dhi = yq[gid][..., 0] - lo, yq[gid][..., -1] - hi
    v = x.astype(np.float64)
    below, above = v < lo[None], v >= hi[None]
    with np.errstate(all="ignore"):
        y = np.where(below, v + dlo[None], v + dhi[None]).astype(F32)
    return below, above, y
