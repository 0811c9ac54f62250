"""The float64 side of the temporal-increment tests (climate2weather_amd.temporal, csrc/temporal.hip): the table by brute force, the
field kinds -- series in time, which the kinds of fp64_crps_ref are not -- and the rules an fp32 result is held to.

The definition (include/c2w_hip.h: c2w_tincr_terms), with the fp32 inputs read as doubles.  Rows r_0 = y when a truth is given, then
r_1 .. r_n = x; for lag tau = 1 .. L and anchor t with t + tau < T
    dx_c = r_d[t + tau][f][c] - r_d[t][f][c],  dy_c the truth's
    S[d][t][f][tau - 1] = (A1, A2, E2) = (sum_c |dx_c|, sum_c dx_c^2, sum_c (dx_c - dy_c)^2)
+0 where t + tau >= T and, without a truth, in E2.  A plane with a NaN or an infinity makes the entries it is an end of NaN, a truth
plane also the E2 of the same entries of every row -- applied explicitly here.

The rules are derived from the count of fp32 roundings, not tuned (eps = 2^-24).  The kernel adds every fp32 term straight into a
double: it keeps no fp32 chain (a chain of n terms would add n eps to each constant below; n = 0 here).  A double sum of hw <= 2^20
non-negative terms adds hw 2^-53 < 2^-33 relative; each constant is rounded up by 1 for that and for the second-order terms.
  A1.  A term is |fl(b - a)|: one rounding, the absolute value is exact: |error| <= eps term.  Non-negative terms: A1 within
       (1 + 1) eps A1.  A1_C = 2.
  A2.  A term is fl(fl(b - a)^2): the rounding of the difference, doubled by the square, and the product's: 3 eps term to first order.
       The round-up is inside the 3, as for the D2 of fp64_escore_ref (2 eps + eps^2 from the square, eps from the product, and
       2^-33): A2 within 3 eps A2.  A2_C = 3.
  E2.  e^ = fl(dx^ - dy^) with dx^ = dx (1 + d1), dy^ = dy (1 + d2): |e^ - e| <= eps (|dx| + |dy|) + eps |e|, and |e| <= |dx| + |dy|.
       The term fl(e^ e^) is off by at most 2 |e| |e^ - e| + eps e^2 <= (2 + 2 + 1) eps (|dx| + |dy|)^2 to first order; rounded up:
       E2 within 6 eps sum_c (|dx_c| + |dy_c|)^2.  E2_C = 6.  The yardstick is the increments, not their difference: a member equal
       to the truth to six digits still rounds its two increments separately.
  Floor.  A product that underflows is off by up to one fp32 denormal, 2^-149, whatever its size: a field of magnitude 1e-30 has
       squares of 1e-60, seven orders of magnitude below, and the relative form alone would ask for the impossible.  Each limit gets
       hw 2^-149 added -- one denormal per term.
"""
import numpy as np

from fp64_escore_ref import worst

KINDS = ("pressure", "temperature", "wind", "ties", "constant", "tiny", "nonfinite")
EPS = 2.0 ** -24
DENORMAL = 2.0 ** -149
A1_C, A2_C, E2_C = 2.0, 3.0, 6.0
CHAIN = 0  # fp32 terms a thread adds up before the double: the kernel keeps no chain


def fields(kind, M, T, F, hw, seed=0):
    """x (M, T, F, hw), y (T, F, hw) fp32, series in time.  Variable f differs from its neighbours in offset and scale, so a wrong index
    map fails.  pressure: 101325 +- 1200 per cell, every row a random walk of its own with hourly steps of 0.05; temperature: 280 +- 10,
    a shared daily wave of amplitude 3 and steps of 0.3; wind: 0 +- 5, new every hour (jittery); ties: wind on a grid of 1 / 2 with
    every third hour repeated (increments of exactly 0); constant: one value per variable for all rows, hours and cells; tiny:
    magnitude 1e-30, whose squares underflow; nonfinite: temperature with a NaN in a member plane, an infinity in another and one in a
    truth plane."""
    rng = np.random.default_rng([seed, M, T, F, hw, KINDS.index(kind)])
    scale = (1.0 + 0.5 * np.arange(F))[None, None, :, None]
    noise = rng.standard_normal((M + 1, T, F, hw))
    if kind == "pressure":
        rows = 101325.0 + 1200.0 * rng.standard_normal((1, 1, F, hw)) + 0.05 * np.cumsum(noise, axis=1)
    elif kind in ("temperature", "nonfinite"):
        wave = 3.0 * np.sin(2.0 * np.pi * np.arange(T) / 24.0)[None, :, None, None]
        rows = 280.0 + 10.0 * rng.standard_normal((1, 1, F, hw)) + wave + 0.3 * np.cumsum(noise, axis=1)
    elif kind in ("wind", "ties", "tiny"):
        rows = 5.0 * noise
    elif kind == "constant":
        rows = np.full((M + 1, T, F, hw), 7.25)
    else:
        raise ValueError(kind)
    rows = rows * scale
    if kind == "ties":
        rows = np.round(2.0 * rows) / 2.0
        for t in range(2, T, 3):
            rows[:, t] = rows[:, t - 1]
    if kind == "tiny":
        rows = rows * 1e-30
    rows = rows.astype(np.float32)
    if kind == "nonfinite":
        rows[1 + M // 2, T // 2, 0, hw // 2] = np.nan
        rows[1, T - 1, F - 1, hw - 1] = np.inf
        rows[0, 0, F // 2, 0] = -np.inf
    return rows[1:].copy(), rows[0].copy()


def table64(x, y, L):
    """x (n_rep, T, F, hw), y (T, F, hw) or None, fp32 -> (S (D, T, F, L, 3), Y (D, T, F, L)) float64: the table by a loop over the lags
    and the yardstick sum_c (|dx_c| + |dy_c|)^2 of its third column"""
    rows = (x if y is None else np.concatenate([y[None], x])).astype(np.float64)
    D, T, F, hw = rows.shape
    bad = ~np.isfinite(rows).all(axis=-1)
    rows = np.where(bad[..., None], 0.0, rows)
    S, Y = np.zeros((D, T, F, L, 3)), np.zeros((D, T, F, L))
    for tau in range(1, L + 1):
        if tau >= T:
            break
        dx = rows[:, tau:] - rows[:, :-tau]
        touched = bad[:, tau:] | bad[:, :-tau]
        S[:, :T - tau, :, tau - 1, 0] = np.where(touched, np.nan, np.abs(dx).sum(axis=-1))
        S[:, :T - tau, :, tau - 1, 1] = np.where(touched, np.nan, (dx * dx).sum(axis=-1))
        if y is not None:
            dy = dx[:1]
            S[:, :T - tau, :, tau - 1, 2] = np.where(touched | touched[:1], np.nan, ((dx - dy) ** 2).sum(axis=-1))
            Y[:, :T - tau, :, tau - 1] = ((np.abs(dx) + np.abs(dy)) ** 2).sum(axis=-1)
    return S, Y


_REF = {}


def reference(kind, M, T, F, hw, L, with_truth=True, seed=0):
    """(x (M, T, F, hw), y (T, F, hw) or None, S, Y) computed once per key, shared and left unchanged"""
    key = (kind, M, T, F, hw, L, with_truth, seed)
    if key not in _REF:
        x, y = fields(kind, M, T, F, hw, seed)
        y = y if with_truth else None
        S, Y = table64(x, y, L)
        for a in (x, y, S, Y):
            if a is not None:
                a.setflags(write=False)
        _REF[key] = (x, y, S, Y)
    return _REF[key]


def limits(S, Y, hw):
    """the three rules as one array of the table's shape"""
    floor = hw * DENORMAL
    lim = np.empty_like(S)
    lim[..., 0] = (A1_C + CHAIN) * EPS * np.nan_to_num(S[..., 0]) + floor
    lim[..., 1] = (A2_C + CHAIN) * EPS * np.nan_to_num(S[..., 1]) + floor
    lim[..., 2] = (E2_C + CHAIN) * EPS * Y + floor
    return lim


def worst_table(got, S, Y, hw):
    """(the largest error over its limit per column -- the limit is 1 --, whether every entry passes).  An entry without a pair must be
    +0.0 to the bit."""
    got = np.asarray(got, dtype=np.float64)
    if got.shape != S.shape:
        return (np.inf,) * 3, False
    lim = limits(S, Y, hw)
    out = [worst(got[..., c], S[..., c], lim[..., c]) for c in range(3)]
    T, L = S.shape[1], S.shape[3]
    no_pair = np.arange(T)[:, None] + np.arange(1, L + 1)[None, :] >= T
    zeros = np.moveaxis(got, 3, 2)[:, no_pair]  # (D, T, L, F, 3) under the (T, L) mask
    exact = bool(np.all(zeros == 0.0) and not np.signbit(zeros).any())
    return tuple(r for r, _ in out), all(ok for _, ok in out) and exact
