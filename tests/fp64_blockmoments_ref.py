"""References for the block moments (climate2weather_amd.scalesplit): the NumPy definition, one add after the other -- the same bits as
every route of the module, which is what the tests assert --, rational arithmetic on the exact fp32 values for the bound of
csrc/blockmoments_maps.h (exact, so the error of the code under test is the only error) and for the identity of the split, and the
fields every test of the metric draws from."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

KINDS = ("pressure", "pressure_tight", "smooth", "denormal", "huge", "constant", "neg_zero", "nan_cells", "inf", "truth_nan")
U = Fraction(1, 2 ** 53)
NAN_BITS = np.uint64(0x7FF8000000000000)


# ---------------------------------------------------------------------------------------------------------------------- fields

def field(kind: str, shape, seed: int) -> np.ndarray:
    """fp32 ``shape = (M, T, F, H, W)`` for the members or ``(T, F, H, W)`` for the truth: one of ``KINDS``"""
    rng = np.random.default_rng(seed)
    truth = len(shape) == 4
    a = rng.standard_normal(shape).astype(np.float32)
    smooth = (np.cumsum(np.cumsum(a, axis=-1, dtype=np.float32), axis=-2, dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    if kind == "smooth":
        a = smooth
    elif kind == "pressure":
        a = (np.float32(101325.0) + np.float32(0.5) * a).astype(np.float32)
    elif kind == "pressure_tight":
        a = (np.float32(101325.0) + rng.uniform(-0.5, 0.5, shape).astype(np.float32)).astype(np.float32)
    elif kind == "denormal":
        a = (a * np.float32(1e-41)).astype(np.float32)
    elif kind == "huge":
        a = (np.sign(a) * np.float32(3e38) * rng.uniform(0.5, 1.0, shape).astype(np.float32)).astype(np.float32)
    elif kind == "constant":
        a = np.full(shape, 2.5, np.float32)
    elif kind == "neg_zero":
        r = rng.random(shape)   # zeros of both signs among small numbers: a term e = (-0.0) - (+0.0) is -0.0
        a = np.where(r < 0.4, np.float32(-0.0), np.where(r < 0.8, np.float32(0.0), a)).astype(np.float32)
    elif kind == "nan_cells":
        a = np.where(rng.random(shape) < 0.02, np.float32(np.nan), smooth).astype(np.float32)
        a[..., 0, 0] = -np.float32(np.nan)    # a NaN with the sign bit as the first block's pivot
    elif kind == "inf":
        r = rng.random(shape)
        a = np.where(r < 0.01, np.float32(np.inf), np.where(r < 0.02, np.float32(-np.inf), smooth)).astype(np.float32)
    elif kind == "truth_nan":
        a = smooth.copy()
        if truth:
            a = np.where(rng.random(shape) < 0.02, np.float32(np.nan), a).astype(np.float32)   # the truth alone
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(a, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------- the definition

def finite(a: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(a).view(np.uint32) & np.uint32(0x7F800000)) != np.uint32(0x7F800000)


def blocks(a: np.ndarray, s: int) -> np.ndarray:
    """``(..., H, W) -> (..., h, w, s, s)``, the block's rows then its columns last"""
    H, W = a.shape[-2:]
    return np.swapaxes(a.reshape(a.shape[:-2] + (H // s, s, W // s, s)), -3, -2)


def block_moments(x: np.ndarray, y, s: int) -> dict:
    """x (M, T, F, H, W), y (T, F, H, W) or None -> n int32 and pivot fp32 (D, T, F, h, w), sums float64 (D, T, F, NS, h, w)"""
    rows = x if y is None else np.concatenate([y[None], x])
    D, T, F, H, W = rows.shape
    h, w, NS = H // s, W // s, 2 if y is None else 3
    n, pivot = np.zeros((D, T, F, h, w), np.int32), np.zeros((D, T, F, h, w), np.float32)
    sums = np.zeros((D, T, F, NS, h, w), np.float64)
    nan = NAN_BITS.view(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        yb = None if y is None else blocks(y, s)
        okT = None if y is None else finite(yb).sum(axis=(-1, -2)) == s * s
        eT = None if y is None else yb.astype(np.float64) - yb[..., 0, 0].astype(np.float64)[..., None, None]
        for d in range(D):
            xb = blocks(rows[d], s)                                           # (T, F, h, w, s, s)
            pivot[d] = xb[..., 0, 0]
            n[d] = finite(xb).sum(axis=(-1, -2))
            e = xb.astype(np.float64) - pivot[d].astype(np.float64)[..., None, None]
            terms = [e, e * e] + ([] if y is None else [e * eT])
            for k, term in enumerate(terms):
                total = np.zeros((T, F, h, w), np.float64)
                for c in range(s):
                    col = np.zeros((T, F, h, w), np.float64)
                    for r in range(s):
                        col = col + term[..., r, c]
                    total = total + col
                ok = (n[d] == s * s) & (okT if k == 2 else True)
                sums[d, :, :, k] = np.where(ok, total, nan)
    return dict(n=n, pivot=pivot, sums=sums, s=s, with_truth=y is not None)


def same_bits(st: dict, n, pivot, sums) -> bool:
    """the tables of a route (NumPy arrays) against the reference's ``st``, as bits"""
    ok = st["n"].shape == tuple(n.shape) and np.array_equal(st["n"], n)
    ok = ok and np.array_equal(st["pivot"].view(np.uint32), np.ascontiguousarray(pivot).view(np.uint32))
    return bool(ok and st["sums"].shape == tuple(sums.shape) and np.array_equal(st["sums"].view(np.uint64), np.ascontiguousarray(sums).view(np.uint64)))


# ---------------------------------------------------------------------------------------------------------------------- rational arithmetic

def bound_rounds(s: int, product: bool) -> int:
    """csrc/blockmoments_maps.h, THE BOUND (bound_rounds)"""
    return 2 * s + (2 if product else 0)


def exact_block(xb: np.ndarray, yb):
    """the exact sums (S1, S2[, X]) of one finite block ``xb (s, s)`` about its pivot, and the sums of the absolute terms"""
    P = Fraction(float(xb[0, 0]))
    e = [Fraction(float(v)) - P for v in xb.ravel()]
    terms = [e, [v * v for v in e]]
    if yb is not None:
        PT = Fraction(float(yb[0, 0]))
        terms.append([a * (Fraction(float(v)) - PT) for a, v in zip(e, yb.ravel())])
    return [sum(t) for t in terms], [sum(abs(v) for v in t) for t in terms]


def chosen_blocks(shape, count: int, seed: int = 0):
    """``count`` block indices ``(d, t, f, i, j)`` of tables of ``shape = (D, T, F, h, w)``: the corners and a random draw"""
    D, T, F, h, w = shape
    rng = np.random.default_rng(seed)
    out = {(0, 0, 0, 0, 0), (D - 1, T - 1, F - 1, h - 1, w - 1)}
    while len(out) < min(count, D * T * F * h * w):
        out.add(tuple(int(rng.integers(0, m)) for m in shape))
    return sorted(out)


def check_bound(x, y, st, chosen, sums=None):
    """the sums of ``st`` (or ``sums`` in its place) against exact arithmetic at the ``chosen`` blocks: asserts the bound where the
    block is valid; returns the worst observed fraction of it (an exact sum of zero terms has the bound 0: the fraction is 0 / 0 = 0)"""
    s = st["s"]
    rows = x if y is None else np.concatenate([y[None], x])
    table = st["sums"] if sums is None else sums
    worst = 0.0
    for d, t, f, i, j in chosen:
        xb = rows[d, t, f, i * s:(i + 1) * s, j * s:(j + 1) * s]
        yb = None if y is None else y[t, f, i * s:(i + 1) * s, j * s:(j + 1) * s]
        if not finite(xb).all():
            continue
        tru = yb is not None and finite(yb).all()
        exact, absolute = exact_block(xb, yb if tru else None)
        for k in range(len(exact)):
            err, b = abs(Fraction(float(table[d, t, f, k, i, j])) - exact[k]), bound_rounds(s, k > 0) * U * absolute[k]
            assert err <= b, (d, t, f, i, j, k, float(err), float(b))
            if b:
                worst = max(worst, float(err / b))
    return worst


def exact_mse(x: np.ndarray, y: np.ndarray) -> Fraction:
    """mean (x - y)^2 of two finite fp32 arrays of one shape, in rational arithmetic"""
    return sum((Fraction(float(a)) - Fraction(float(b))) ** 2 for a, b in zip(x.ravel(), y.ravel())) / x.size
