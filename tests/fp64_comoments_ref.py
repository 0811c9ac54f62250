"""References for the co-moments (climate2weather_amd.dependence): the NumPy definition hour by hour -- the same bits as every route
of the module, which is what the tests assert --, rational arithmetic on the exact fp32 values for the bounds of
csrc/comoments_maps.h (exact, so the error of the code under test is the only error), the same for ``merge``, and the fields every
test of the metric draws from."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

KINDS = ("smooth", "pressure", "pressure_tight", "constant", "inf", "nan_hours", "late_start", "nan_series", "truth_nan", "denormal", "huge")
U = Fraction(1, 2 ** 53)
TINY = Fraction(1, 2 ** 1074)


# ---------------------------------------------------------------------------------------------------------------------- fields

def field(kind: str, shape, seed: int) -> np.ndarray:
    """fp32 ``shape = (M, T, F, hw)`` for the members or ``(T, F, hw)`` for the truth: one of ``KINDS``"""
    rng = np.random.default_rng(seed)
    T, truth = shape[-3], len(shape) == 3
    a = rng.standard_normal(shape).astype(np.float32)
    smooth = np.cumsum(a, axis=-3, dtype=np.float32) * np.float32(0.3)
    if kind == "smooth":
        a = smooth
    elif kind == "pressure":
        a = (np.float32(1e5) + np.float32(1e3) * a).astype(np.float32)
    elif kind == "pressure_tight":
        a = (np.float32(101325.0) + rng.uniform(-0.5, 0.5, shape).astype(np.float32)).astype(np.float32)
    elif kind == "constant":
        a = np.full(shape, 2.5, np.float32)
    elif kind == "inf":
        r = rng.random(shape)
        a = np.where(r < 0.15, np.float32(np.inf), np.where(r < 0.3, np.float32(-np.inf), smooth)).astype(np.float32)
    elif kind == "nan_hours":
        a = np.where(rng.random(shape) < 0.2, np.float32(np.nan), smooth).astype(np.float32)   # each variable at hours of its own
        a[..., T - 1, 0, 0] = np.float32(-np.nan)                                              # a NaN with the sign bit
    elif kind == "late_start":
        a = smooth.copy()
        a[..., :min(2, T - 1), :, :] = np.nan    # the first hours of every series: the pivot arrives late
    elif kind == "nan_series":
        a = smooth.copy()
        a[..., :, :, 1] = np.nan                 # cell 1 of every row and variable is never valid
    elif kind == "truth_nan":
        a = smooth.copy()
        if truth:
            a[..., 0, :] = np.where(rng.random(a[..., 0, :].shape) < 0.3, np.float32(np.nan), a[..., 0, :])  # the truth alone, in variable 0
    elif kind == "denormal":
        a = (a * np.float32(1e-41)).astype(np.float32)
    elif kind == "huge":
        a = (np.sign(a) * np.float32(3e38) * rng.uniform(0.5, 1.0, shape).astype(np.float32)).astype(np.float32)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(a, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------- the definition

def pair_list(F):
    return [(f, g) for f in range(F) for g in range(f, F)]


def entries(F, with_truth):
    return F + F * (F + 1) // 2 + (3 * F if with_truth else 0)


def finite(a: np.ndarray) -> np.ndarray:
    return (a.view(np.uint32) & np.uint32(0x7F800000)) != np.uint32(0x7F800000)


def new_state(D, F, hw, with_truth):
    return dict(n=np.zeros((D, hw), np.int32), pivot=np.zeros((D, F, hw), np.float32),
                truth_pivot=np.zeros((D, F, hw), np.float32) if with_truth else None,
                sums=np.zeros((D, entries(F, with_truth), hw), np.float64), invalid=np.zeros((D,), np.int64))


def update(st, x: np.ndarray, y) -> dict:
    """``T`` more hours onto the state ``st``, one hour and one entry after the other: x (M, T, F, hw), y (T, F, hw) or None"""
    M, T, F, hw = x.shape
    rows = x if y is None else np.concatenate([y[None], x])
    D, NP = rows.shape[0], F * (F + 1) // 2
    n, P, PT, s = st["n"], st["pivot"], st["truth_pivot"], st["sums"]
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(D):
            for t in range(T):
                r = rows[d, t]                                                     # (F, hw)
                valid = finite(r).all(axis=0)
                if y is not None:
                    valid &= finite(y[t]).all(axis=0)
                first = valid & (n[d] == 0)
                P[d][:, first] = r[:, first]
                n[d] += valid
                st["invalid"][d] += int((~valid).sum())
                e = r.astype(np.float64) - P[d].astype(np.float64)
                for f in range(F):
                    s[d, f, valid] = s[d, f, valid] + e[f, valid]
                for k, (f, g) in enumerate(pair_list(F)):
                    term = e[f] * e[g]
                    s[d, F + k, valid] = s[d, F + k, valid] + term[valid]
                if y is not None:
                    PT[d][:, first] = y[t][:, first]
                    eT = y[t].astype(np.float64) - PT[d].astype(np.float64)
                    for f in range(F):
                        q, c = eT[f] * eT[f], e[f] * eT[f]
                        s[d, F + NP + f, valid] = s[d, F + NP + f, valid] + eT[f, valid]
                        s[d, 2 * F + NP + f, valid] = s[d, 2 * F + NP + f, valid] + q[valid]
                        s[d, 3 * F + NP + f, valid] = s[d, 3 * F + NP + f, valid] + c[valid]
    return st


def comoments(x: np.ndarray, y) -> dict:
    M, T, F, hw = x.shape
    return update(new_state(M + (y is not None), F, hw, y is not None), x, y)


def same_bits(st: dict, n, pivot, truth_pivot, sums, invalid) -> bool:
    """the tables of a route (NumPy arrays of any shape with the same elements) against the state ``st``, as bits"""
    ok = np.array_equal(st["n"].ravel(), n.ravel()) and np.array_equal(st["invalid"].ravel(), invalid.ravel())
    ok = ok and np.array_equal(st["pivot"].view(np.uint32).ravel(), np.ascontiguousarray(pivot).view(np.uint32).ravel())
    ok = ok and np.array_equal(st["sums"].view(np.uint64).ravel(), np.ascontiguousarray(sums).view(np.uint64).ravel())
    if st["truth_pivot"] is not None:
        ok = ok and np.array_equal(st["truth_pivot"].view(np.uint32).ravel(), np.ascontiguousarray(truth_pivot).view(np.uint32).ravel())
    return bool(ok)


# ---------------------------------------------------------------------------------------------------------------------- rational arithmetic

def _series(x, y, d, cell):
    """the valid hours of (d, cell) as exact values: ([row's F Fractions], [truth's F Fractions] or None) per hour"""
    row = (x[d] if y is None else (y if d == 0 else x[d - 1]))[:, :, cell]        # (T, F)
    tru = None if y is None else y[:, :, cell]
    out = []
    for t in range(row.shape[0]):
        if not finite(np.ascontiguousarray(row[t])).all() or (tru is not None and not finite(np.ascontiguousarray(tru[t])).all()):
            continue
        out.append(([Fraction(float(v)) for v in row[t]], None if tru is None else [Fraction(float(v)) for v in tru[t]]))
    return out


def exact_sums(hours, P, PT):
    """the NS exact sums of the valid ``hours`` about the pivots ``P`` / ``PT`` (Fractions), and the sums of the absolute terms"""
    F = len(P)
    NS = entries(F, PT is not None)
    s, a = [Fraction(0)] * NS, [Fraction(0)] * NS
    NP = F * (F + 1) // 2
    for xs, ys in hours:
        e = [xs[f] - P[f] for f in range(F)]
        terms = e + [e[f] * e[g] for f, g in pair_list(F)]
        if PT is not None:
            eT = [ys[f] - PT[f] for f in range(F)]
            terms += eT + [v * v for v in eT] + [e[f] * eT[f] for f in range(F)]
        s = [p + q for p, q in zip(s, terms)]
        a = [p + abs(q) for p, q in zip(a, terms)]
    return s, a, NP


def is_product(k, F):
    """whether entry ``k`` is a sum of products (C, QT, X) and not of differences (S, ST)"""
    NP = F * (F + 1) // 2
    return F <= k < F + NP or k >= 2 * F + NP


def bound(n, product, A):
    """csrc/comoments_maps.h, THE BOUND (bound_rounds)"""
    return (n + (2 if product else 1)) * U * A + TINY


def check_bound(x, y, st, cells, rows=None):
    """the sums of ``st`` against exact arithmetic at ``cells`` (of every row, or of ``rows``): asserts n, the pivots and the bound;
    returns the worst observed fraction of the bound"""
    M, T, F, hw = x.shape
    D = M + (y is not None)
    worst = 0.0
    for d in (range(D) if rows is None else rows):
        for c in cells:
            hours = _series(x, y, d, c)
            n = len(hours)
            assert int(st["n"][d, c]) == n, (d, c, int(st["n"][d, c]), n)
            P = hours[0][0] if n else [Fraction(0)] * F
            PT = None if y is None else (hours[0][1] if n else [Fraction(0)] * F)
            assert [Fraction(float(v)) for v in st["pivot"][d, :, c]] == P, (d, c)
            if y is not None:
                assert [Fraction(float(v)) for v in st["truth_pivot"][d, :, c]] == PT, (d, c)
            s, a, _ = exact_sums(hours, P, PT)
            for k in range(len(s)):
                err, b = abs(Fraction(float(st["sums"][d, k, c])) - s[k]), bound(n, is_product(k, F), a[k])
                assert err <= b, (d, c, k, float(err), float(b))
                worst = max(worst, float(err / b))
    return worst


def check_merge(xs, ys, xo, yo, st, cells):
    """``st``: the state of an accumulator over the hours ``(xs, ys)`` after ``merge`` of one over the hours ``(xo, yo)``, against
    exact arithmetic about the first one's pivots, within the merge bound of csrc/comoments_maps.h; returns the worst fraction"""
    M, _, F, hw = xs.shape
    D = M + (ys is not None)
    worst = 0.0
    for d in range(D):
        for c in cells:
            hs, ho = _series(xs, ys, d, c), _series(xo, yo, d, c)
            ns, no = len(hs), len(ho)
            assert int(st["n"][d, c]) == ns + no, (d, c)
            zero = [Fraction(0)] * F
            Po, PTo = (ho[0][0] if no else zero), (None if ys is None else (ho[0][1] if no else zero))
            P, PT = (hs[0][0], None if ys is None else hs[0][1]) if ns else (Po, PTo)
            assert [Fraction(float(v)) for v in st["pivot"][d, :, c]] == P, (d, c)
            s, _, NP = exact_sums(hs + ho, P, PT)
            _, a_s, _ = exact_sums(hs, P, PT)
            _, a_o, _ = exact_sums(ho, Po, PTo)
            if ns == 0:
                bounds = [bound(no, is_product(k, F), a_o[k]) for k in range(len(s))]      # the other's state as it is
            else:
                dl = [abs(Po[f] - P[f]) for f in range(F)]
                dT = None if ys is None else [abs(PTo[f] - PT[f]) for f in range(F)]
                # the majorants A' = sum_o (|e| + |d|) [(|e'| + |d'|)], expanded: sum |e e'| + |d| sum |e'| + |d'| sum |e| + n |d d'|
                maj = [a_o[f] + no * dl[f] for f in range(F)]
                maj += [a_o[F + k] + dl[f] * a_o[g] + dl[g] * a_o[f] + no * dl[f] * dl[g] for k, (f, g) in enumerate(pair_list(F))]
                if ys is not None:
                    aT = a_o[F + NP:2 * F + NP]
                    maj += [aT[f] + no * dT[f] for f in range(F)]
                    maj += [a_o[2 * F + NP + f] + 2 * dT[f] * aT[f] + no * dT[f] * dT[f] for f in range(F)]
                    maj += [a_o[3 * F + NP + f] + dl[f] * aT[f] + dT[f] * a_o[f] + no * dl[f] * dT[f] for f in range(F)]
                bounds = []
                for k in range(len(s)):
                    prod = is_product(k, F)
                    bounds.append((ns + (4 if prod else 3)) * U * a_s[k] + (no + (11 if prod else 6)) * U * maj[k] + 2 * TINY)
            for k in range(len(s)):
                err = abs(Fraction(float(st["sums"][d, k, c])) - s[k])
                assert err <= bounds[k], (d, c, k, float(err), float(bounds[k]))
                worst = max(worst, float(err / bounds[k]))
    return worst


def central_bound(n, S_f, S_g, C, a_f, a_g, a_fg):
    """the error of ``C - S_f S_g / n`` formed in float64 from sums within THE BOUND: their own errors, and the roundings of the
    product, the quotient and the difference (4 u by the convention) on the two parts"""
    Ef, Eg, Ec = bound(n, False, a_f), bound(n, False, a_g), bound(n, True, a_fg)
    return Ec + (abs(S_f) * Eg + abs(S_g) * Ef + Ef * Eg) / n + 4 * U * (abs(C) + abs(S_f * S_g) / n)
