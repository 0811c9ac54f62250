"""The reference of the event tables (climate2weather_amd.events) in NumPy, and the fields the tests run on.

The event is an IEEE comparison of exact fp32 values, and both tables are integers: ``counts_ref`` and ``fss_ref`` are the definition
written out -- the joint histogram of truth indicator and member count, and window sums from an int64 cumulative table padded with a
zero row and column -- and every route must EQUAL them; there is no tolerance anywhere.

The kinds: pressure-like, temperature, wind, constant, a field with ties exactly at the threshold, both zeros at a threshold of 0,
infinities, and NaNs.  Variable ``f`` differs from its neighbours in offset and scale, so a wrong index map fails.
"""
import numpy as np

KINDS = ("pressure", "temperature", "wind", "constant", "ties", "zeros", "infinities", "nans")


def fields(kind, M, T, F, hw, seed=0):
    """x (M, T, F, hw), y (T, F, hw) fp32"""
    rng = np.random.default_rng([seed, KINDS.index(kind), M, T, F, hw])
    z = rng.standard_normal((M + 1, T, F, hw))
    z[1:] = 0.6 * z[:1] + 0.8 * z[1:]  # the members follow the truth, so that every bin of the joint table fills
    f = np.arange(F).reshape(1, 1, F, 1)
    if kind == "pressure":
        v = 1000.0 + 3.0 * f + 12.0 * z
    elif kind == "temperature":
        v = 280.0 - 5.0 * f + (6.0 + f) * z
    elif kind == "wind":
        v = np.abs(z) * (5.0 + f)
    elif kind == "constant":
        v = np.full_like(z, 3.0) + f
    elif kind == "ties":
        v = np.round(z * 2.0) / 2.0 + f  # multiples of 0.5: many values lie exactly on a threshold
    elif kind == "zeros":
        u = rng.random(z.shape)
        v = np.where(u < 0.35, 0.0, np.where(u < 0.7, -0.0, z * 1e-3))  # +0.0, -0.0 and small numbers of both signs
    elif kind == "infinities":
        v = 2.0 * z + f
        u = rng.random(z.shape)
        v = np.where(u < 0.05, np.inf, np.where(u > 0.95, -np.inf, v))
    elif kind == "nans":
        v = 2.0 * z - f
        v = np.where(rng.random(z.shape) < 0.03, np.nan, v)
    else:
        raise KeyError(kind)
    v = v.astype(np.float32)
    return np.ascontiguousarray(v[1:]), np.ascontiguousarray(v[0])


def thresholds(kind, y, K):
    """(F, K) fp32 for the truth y (T, F, hw) of that kind: quantiles of the finite values, moved onto the special values of the kind"""
    F = y.shape[1]
    levels = np.linspace(0.35, 0.97, K)
    thr = np.zeros((F, K), np.float32)
    for f in range(F):
        v = y[:, f][np.isfinite(y[:, f])]
        thr[f] = np.quantile(v.astype(np.float64), levels).astype(np.float32) if v.size else 0.0
    if kind == "constant":
        thr[:, 0] = y[0, :, 0]                      # every value ties with the threshold
    elif kind == "ties":
        thr = (np.round(thr * 2.0) / 2.0).astype(np.float32)
    elif kind == "zeros":
        thr[:, 0::2], thr[:, 1::2] = 0.0, -0.0      # both zeros as the threshold: they compare equal to both zeros
    elif kind == "infinities":
        thr[:, 0] = np.inf
        if K > 1:
            thr[:, -1] = -np.inf
    return thr


def directions(F, K, direction):
    """(F, K) bool, True above: 'above', 'below' or 'mixed' (alternating over the entries)"""
    if direction == "mixed":
        return (np.arange(F * K).reshape(F, K) % 2) == 0
    return np.full((F, K), direction == "above")


def direction_names(above):
    return [["above" if a else "below" for a in row] for row in above]


def indicator(v, thr, above):
    """v (..., F, hw) fp32 -> bool (..., F, K, hw): v >= thr above, v <= thr below, in fp32"""
    assert v.dtype == np.float32 and thr.dtype == np.float32
    v, t, a = v[..., :, None, :], thr[:, :, None], above[:, :, None]
    with np.errstate(invalid="ignore"):
        return np.where(a, v >= t, v <= t)


def counts_ref(x, y, thr, above):
    """counts (T, F, K, 2, M + 1) and invalid (T, F), int64"""
    M, T, F, hw = x.shape
    K = thr.shape[1]
    j = indicator(x, thr, above).sum(axis=0)             # (T, F, K, hw)
    o = indicator(y, thr, above).astype(np.int64)
    nan = np.isnan(y) | np.isnan(x).any(axis=0)          # (T, F, hw)
    counts = np.zeros((T, F, K, 2, M + 1), np.int64)
    for t in range(T):
        for f in range(F):
            ok = ~nan[t, f]
            for k in range(K):
                np.add.at(counts[t, f, k], (o[t, f, k][ok], j[t, f, k][ok]), 1)
    return counts, nan.sum(axis=-1).astype(np.int64)


def padded_table(rows):
    """rows (..., H, W) int64 -> (..., H + 1, W + 1): P[a][b] = the sum of the rows < a and the columns < b"""
    P = np.zeros(rows.shape[:-2] + (rows.shape[-2] + 1, rows.shape[-1] + 1), np.int64)
    P[..., 1:, 1:] = rows.cumsum(axis=-1).cumsum(axis=-2)
    return P


def window_sums(rows, r):
    """n (..., H, W) int64: the sum over the (2r + 1)^2 window centred on every cell, cells outside the domain 0"""
    H, W = rows.shape[-2:]
    P = padded_table(rows.astype(np.int64))
    a0, a1 = np.clip(np.arange(H) - r, 0, H)[:, None], np.clip(np.arange(H) + r + 1, 0, H)[:, None]
    b0, b1 = np.clip(np.arange(W) - r, 0, W)[None, :], np.clip(np.arange(W) + r + 1, 0, W)[None, :]
    return P[..., a1, b1] - P[..., a0, b1] - P[..., a1, b0] + P[..., a0, b0]


def event_rows(x, y, thr, above, H, W):
    """(M + 2, T, F, K, H, W) int64: the truth, the members, the member count"""
    e = indicator(x, thr, above).astype(np.int64)
    rows = np.concatenate([indicator(y, thr, above).astype(np.int64)[None], e, e.sum(axis=0, keepdims=True)])
    return rows.reshape(rows.shape[:-1] + (H, W))


def fss_ref(x, y, thr, above, radii, H, W):
    """sums (T, F, K, S, M + 2, 2) int64"""
    M, T, F, hw = x.shape
    rows = event_rows(x, y, thr, above, H, W)
    out = np.zeros((T, F, thr.shape[1], len(radii), M + 2, 2), np.int64)
    for s, r in enumerate(radii):
        n = window_sums(rows, r)
        out[:, :, :, s, :, 0] = np.moveaxis((n * n).sum(axis=(-1, -2)), 0, -1)
        out[:, :, :, s, :, 1] = np.moveaxis((n * n[:1]).sum(axis=(-1, -2)), 0, -1)
    return out
