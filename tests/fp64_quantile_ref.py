"""The quantile definition restated with a numpy sort, the key map, the test fields and the level sets (shared by
tests/test_quantiles_cpu.py and tests/test_gpu_quantiles.py).

The definition (include/c2w_hip.h: c2w_quantiles), line by line, for the values x of one data set and a level q:

    nv = #non-NaN; v = (nv - 1) q in float64; lo = floor(v); hi = min(lo + 1, nv - 1); t = v - lo                      ``ranks``
    a, b = the lo-th and hi-th smallest non-NaN value (fp32, exact)                                                      ``order_stats``
    a + (b - a) t where t < 0.5, b - (b - a)(1 - t) where t >= 0.5, in float64, every operation rounded on its own       ``lerp``

which is ``numpy.quantile(x.astype(float64), q)`` (tests/test_quantiles_cpu.py checks that on every kind), except that a zero may
carry either sign.  Everything is exact, so nothing here is a tolerance: order statistics compare bit for bit with -0.0 == +0.0
allowed (``same_stats``), results as numbers with NaN equal to NaN (``same_numbers``), counts exactly.
"""
import functools

import numpy as np

NINE = (0.0, 0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 1.0)  # data/xarray_preproc.py::compute_quantiles
KINDS = ("pressure", "normal", "ties", "constant", "denormal", "lowbits", "twovalued", "ascending", "descending", "inf", "nan", "allnan")
LEVEL_SETS = ("median", "ends", "nine", "sixteen")


# ------------------------------------------------------------------------------------------------------------------ the definition

def key_of(bits):
    """the monotone key of fp32 bit patterns (uint32 array): unsigned order of the keys is the order of the values"""
    bits = np.asarray(bits, dtype=np.uint32)
    return bits ^ np.where(bits >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def bits_of(key):
    key = np.asarray(key, dtype=np.uint32)
    return key ^ np.where(key >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))


def ranks(nv, q):
    """(lo, hi, t) for nv valid values and the levels q"""
    v = np.float64(nv - 1) * np.asarray(q, dtype=np.float64)
    lo = np.floor(v)
    hi = np.minimum(lo + 1, nv - 1)
    return lo.astype(np.int64), hi.astype(np.int64), v - lo


def lerp(a, b, t):
    a, b, t = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(t, np.float64)
    with np.errstate(invalid="ignore"):
        diff = b - a
        return np.where(t >= 0.5, b - diff * (1.0 - t), a + diff * t)


def quantiles_of(values, q, skipna=True):
    """one data set (fp32, any shape) -> (out (Q,) float64, stats (Q, 2) fp32, nv)"""
    v = np.asarray(values, dtype=np.float32).reshape(-1)
    q = np.asarray(q, dtype=np.float64)
    good = v[~np.isnan(v)]
    nv = int(good.size)
    if nv == 0 or (not skipna and nv < v.size):
        return np.full(q.size, np.nan), np.full((q.size, 2), np.nan, np.float32), nv
    keys = np.sort(key_of(good.view(np.uint32)))  # the order of the keys: -0.0 below +0.0, as the kernel has it
    s = bits_of(keys).view(np.float32)
    lo, hi, t = ranks(nv, q)
    return lerp(s[lo], s[hi], t), np.stack([s[lo], s[hi]], axis=-1), nv


def data_sets(samples, truth=None):
    """samples (n_rep, T, F, hw) and truth (T, F, hw) -> [values (n,) fp32] in the launch's order: member-major, then truth"""
    n_rep, T, F, hw = samples.shape
    out = [np.ascontiguousarray(samples[r, :, f]).reshape(-1) for r in range(n_rep) for f in range(F)]
    if truth is not None:
        out += [np.ascontiguousarray(truth[:, f]).reshape(-1) for f in range(F)]
    return out


def expected(samples, truth, q, skipna=True):
    """(out (D, Q) float64, stats (D, Q, 2) fp32, nv (D,) int64) for every data set of a launch"""
    rows = [quantiles_of(v, q, skipna) for v in data_sets(samples, truth)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.array([r[2] for r in rows], np.int64)


def same_numbers(got, want):
    return np.array_equal(np.asarray(got, np.float64), np.asarray(want, np.float64), equal_nan=True)


def same_stats(got, want):
    """bit for bit, except that the two zeros are one number and every NaN is a NaN"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return False
    bits = got.view(np.uint32) == want.view(np.uint32)
    zeros = (got == 0) & (want == 0)
    nans = np.isnan(got) & np.isnan(want)
    return bool(np.all(bits | zeros | nans))


# ------------------------------------------------------------------------------------------------------------------ fields

def _spread(F):
    """variable f differs from its neighbours in offset and scale, so a wrong i % F shows"""
    f = np.arange(F, dtype=np.float64)
    return (1.0 + 0.37 * f)[None, None, :, None], (3.0 * f)[None, None, :, None]


def fields(kind, n_rep, T, F, hw, seed=0):
    """(samples (n_rep, T, F, hw), truth (T, F, hw)) fp32 of one kind"""
    rng = np.random.default_rng([seed, n_rep, T, F, hw, KINDS.index(kind)])
    z = rng.standard_normal((n_rep + 1, T, F, hw))
    scale, offset = _spread(F)
    if kind == "pressure":
        a = 101325.0 + 900.0 * z * scale + 40.0 * offset
    elif kind in ("normal", "ascending", "descending", "inf", "nan", "allnan"):
        a = z * scale + offset
    elif kind == "ties":
        a = np.round(2.0 * z) * scale
    elif kind == "constant":
        a = np.zeros_like(z) + 3.5 + offset
    elif kind == "denormal":
        a = 1e-41 * z * scale
    elif kind == "lowbits":  # decided only by the last ten key bits, whatever the split
        a = 280.0 + offset + rng.integers(0, 1024, z.shape) * 2.0 ** -15
    elif kind == "twovalued":
        a = np.where(rng.permutation(z.size).reshape(z.shape) % 2 == 0, -1.0 - offset, 2.0 + offset)
    a = a.astype(np.float32)
    if kind == "ties":  # both zeros
        at = np.flatnonzero(a == 0)
        a.reshape(-1)[at[::2]] = -0.0  # every other zero is the negative one
    if kind in ("ascending", "descending"):
        for r in range(n_rep + 1):
            for f in range(F):
                v = np.sort(a[r, :, f].reshape(-1))
                a[r, :, f] = (v if kind == "ascending" else v[::-1]).reshape(T, hw)
    if kind == "inf":
        a[:, 0, :, 0] = np.inf
        a[:, T - 1, :, hw - 1] = -np.inf
    if kind == "nan":
        bits = a.view(np.uint32)
        hit = rng.random(a.shape) < 0.2
        hit[:, 0, :, :2] = True
        neg = rng.random(a.shape) < 0.5
        neg[:, 0, :, 0], neg[:, 0, :, 1] = True, False
        bits[hit & neg] = 0xFFC00001
        bits[hit & ~neg] = 0x7FC00000
        if hw * T > 2:
            a[:, T - 1, :, hw - 1] = np.float32(offset[0, 0, :, 0] - 9.0)  # at least one value survives
    if kind == "allnan":
        a[0, :, 0] = np.nan
    return np.ascontiguousarray(a[:n_rep]), np.ascontiguousarray(a[n_rep])


def levels(name, n, seed=0):
    """a level set for data sets of n values"""
    if name == "median":
        return np.array([0.5])
    if name == "ends":
        return np.array([0.0, 1.0])
    if name == "nine":
        return np.array(NINE)
    assert name == "sixteen"
    rng = np.random.default_rng([seed, n])
    exact = rng.integers(0, n, 4) / max(1, n - 1)  # (n - 1) q is an integer up to rounding
    rand = rng.random(9)
    q = np.concatenate([[0.0, 1.0], np.minimum(exact, 1.0), rand, rand[:1]])  # a repeated level, unsorted
    assert q.size == 16
    return q


@functools.lru_cache(maxsize=None)
def case(kind, n_rep, T, F, hw, level_set, with_truth=True, skipna=True):
    """(samples, truth or None, q, out, stats, nv), computed once and shared: treat the arrays as read-only"""
    s, t = fields(kind, n_rep, T, F, hw)
    t = t if with_truth else None
    q = levels(level_set, T * hw)
    out, stats, nv = expected(s, t, q, skipna)
    for a in (s, t, q, out, stats, nv):
        if a is not None:
            a.setflags(write=False)
    return s, t, q, out, stats, nv
