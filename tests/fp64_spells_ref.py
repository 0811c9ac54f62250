"""The reference of the spell tables (climate2weather_amd.spells) in NumPy, and the fields the tests run on.

Everything is integers, so every route must EQUAL ``spells_ref``; there is no tolerance anywhere.  It is written independently of the
torch route: per series the indicator is padded with a zero at both ends, ``np.diff`` along time gives the starts (+1) and the ends
(-1), a spell's length is ``end - start``, and the tables are ``bincount``s.  A run that touches the first or the last time is a spell
of its observed length (censored spells are counted) -- the padding does exactly that.

The kinds are made so that spells are not all short (a field random in time alone gives geometric lengths near 1): a smooth AR(1)-like
series, a periodic one, all-event, no-event, alternating, ties exactly at the threshold with both zeros, infinities, NaNs placed inside
spells, and pressure-like magnitudes.  Variable ``f`` differs from its neighbours in offset and scale, so a wrong index map fails.
"""
import numpy as np

KINDS = ("smooth", "periodic", "all", "none", "alternating", "ties", "infinities", "nans", "pressure")


def _ar1(rng, shape, rho=0.9):
    """(M + 1, T, F, hw): unit-variance AR(1) along time"""
    z = rng.standard_normal(shape)
    for t in range(1, shape[1]):
        z[:, t] = rho * z[:, t - 1] + np.sqrt(1.0 - rho * rho) * z[:, t]
    return z


def fields(kind, M, T, F, hw, seed=0):
    """x (M, T, F, hw), y (T, F, hw) fp32"""
    rng = np.random.default_rng([seed, KINDS.index(kind), M, T, F, hw])
    shape = (M + 1, T, F, hw)
    f = np.arange(F).reshape(1, 1, F, 1)
    t = np.arange(T).reshape(1, T, 1, 1)
    z = _ar1(rng, shape)
    if kind == "smooth":
        v = 280.0 - 5.0 * f + (6.0 + f) * z
    elif kind == "periodic":
        v = np.sin(2.0 * np.pi * (t + rng.integers(0, 6, (M + 1, 1, F, hw))) / 6.0) * (2.0 + f) + 0.3 * z + f
    elif kind == "all":
        v = 50.0 + f + np.abs(z)
    elif kind == "none":
        v = -50.0 - f - np.abs(z)
    elif kind == "alternating":
        v = np.where((t + rng.integers(0, 2, (M + 1, 1, F, hw))) % 2 == 0, 3.0 + f, -3.0 - f) + 0.0 * z
    elif kind == "ties":
        u = rng.random(shape)
        v = np.where(u < 0.3, 0.0, np.where(u < 0.6, -0.0, np.round(z * 2.0) / 2.0))  # both zeros and multiples of 0.5
    elif kind == "infinities":
        v = 2.0 * z + f
        u = rng.random(shape)
        v = np.where(u < 0.08, np.inf, np.where(u > 0.92, -np.inf, v))
    elif kind == "nans":
        v = np.where(z > -0.5, 4.0 + f + z, -4.0 - f + z)          # long spells above 0 ...
        v = np.where(rng.random(shape) < 0.06, np.nan, v)          # ... with NaNs inside them
    elif kind == "pressure":
        v = 100000.0 + 300.0 * f + 1200.0 * z
    else:
        raise KeyError(kind)
    v = v.astype(np.float32)
    return np.ascontiguousarray(v[1:]), np.ascontiguousarray(v[0])


def thresholds(kind, y, K):
    """(F, K) fp32 for the truth y (T, F, hw) of that kind: quantiles of the finite values, moved onto the special values of the kind"""
    F = y.shape[1]
    levels = np.linspace(0.3, 0.9, K)
    thr = np.zeros((F, K), np.float32)
    for f in range(F):
        v = y[:, f][np.isfinite(y[:, f])]
        thr[f] = np.quantile(v.astype(np.float64), levels).astype(np.float32) if v.size else 0.0
    if kind in ("all", "none", "alternating", "nans"):
        thr[:] = np.linspace(-1.0, 1.0, K, dtype=np.float32) if K > 1 else 0.0
    elif kind == "ties":
        thr = (np.round(thr * 2.0) / 2.0).astype(np.float32)
        thr[:, 0::2], thr[:, 1::3] = 0.0, -0.0      # both zeros as the threshold: they compare equal to both zeros
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


def indicator(rows, thr, above):
    """rows (D, T, F, hw) fp32 -> bool (D, F, K, hw, T): v >= thr above, v <= thr below, in fp32; time last"""
    assert rows.dtype == np.float32 and thr.dtype == np.float32
    v = np.moveaxis(rows, 1, -1)[:, :, None]                      # (D, F, 1, hw, T)
    t, a = thr[None, :, :, None, None], above[None, :, :, None, None]
    with np.errstate(invalid="ignore"):
        return np.where(a, v >= t, v <= t)


def spells_ref(x, y, thr, above, max_duration, period=0, t0=0):
    """dict of hist (D, F, K, Lmax) int64, hours / count / longest (D, F, K, hw) int32, onsets (D, F, K, period) int64, invalid (D, F)
    int64, censored (D, F, K) int64 for the rows y (or none), x over ALL their times"""
    rows = x if y is None else np.concatenate([y[None], x])
    D, T, F, hw = rows.shape
    K = thr.shape[1]
    e = indicator(rows, thr, above).astype(np.int8)                # (D, F, K, hw, T)
    n_series = D * F * K * hw
    padded = np.zeros((n_series, T + 2), np.int8)
    padded[:, 1:-1] = e.reshape(n_series, T)
    step = np.diff(padded, axis=1)                                 # (series, T + 1): +1 where a spell starts at t, -1 where one ended before t
    s_series, start = np.nonzero(step == 1)                        # row-major: the starts and the ends of a series pair up in order
    e_series, end = np.nonzero(step == -1)
    assert np.array_equal(s_series, e_series)
    length = end - start
    group = s_series // hw                                         # (d, f, k)
    hist = np.bincount(group * max_duration + np.minimum(length, max_duration) - 1, minlength=D * F * K * max_duration)
    count = np.bincount(s_series, minlength=n_series)
    longest = np.zeros(n_series, np.int64)
    np.maximum.at(longest, s_series, length)
    onsets = np.zeros((D, F, K, period), np.int64)
    if period:
        onsets = np.bincount(group * period + (t0 + start) % period, minlength=D * F * K * period).reshape(D, F, K, period)
    censored = np.bincount(group[(start == 0) | (end == T)], minlength=D * F * K) if T else np.zeros(D * F * K, np.int64)
    return dict(hist=hist.reshape(D, F, K, max_duration).astype(np.int64), hours=e.sum(axis=-1).astype(np.int32),
                count=count.reshape(D, F, K, hw).astype(np.int32), longest=longest.reshape(D, F, K, hw).astype(np.int32),
                onsets=onsets.astype(np.int64), invalid=np.isnan(rows).sum(axis=(1, 3)).astype(np.int64),
                censored=censored.reshape(D, F, K).astype(np.int64))
