"""The float64 side of the energy-score and variogram-score tests (climate2weather_amd.multivariate, csrc/escore.hip): the definitions
by brute force -- pairs by double loop, offsets by slicing --, the field kinds (those of fp64_crps_ref, imported) and the rules an fp32
result is held to.

The definitions (include/c2w_hip.h: c2w_escore_pairs, c2w_vario_terms), with the fp32 inputs read as doubles.  Rows r_0 = y, r_m = x_m.
    D2[p] = sum_c (r_i[c] - r_j[c])^2, i < j, p row-major
    V[o][0..2] = sum over the pairs (c, c + o) inside the field of ((g_y - g_x)^2, g_y, g_x),
                 g_y = |y_c - y_{c+o}|^p, g_x = (1 / M) sum_m |x_{m,c} - x_{m,c+o}|^p
A row with a NaN or an infinity makes its D2 entries NaN; a cell with one (in any row) makes the three sums of every offset one of
whose pairs touches it NaN -- applied explicitly here.

The rules are derived from the count of fp32 roundings, not tuned (eps = 2^-24; a double sum of n <= 2^20 non-negative terms adds
n 2^-53 < 2^-33 relative, which the first-order constants below absorb because no term ever meets all its worst roundings at once --
and which the round-up of each constant by 1 where noted covers anyway).
  D2.  A term is fl(fl(a - b)^2): one rounding in the difference, which the square doubles, one in the product: 3 roundings,
       |error| <= 3 eps term.  The terms are non-negative and are summed in double, no fp32 chain is kept: D2 within 3 eps D2.
       D2_C = 3.
  V.   A single term t = fl(pow(fl(a - b))) carries at most 2 roundings at every order (p = 1: the difference only; p = 0.5: the
       difference, halved by the root, and the correctly rounded root; p = 2: the difference twice and the product -- 3, so the count
       below takes 3 for a term).  g_y is one term: <= 3 eps g_y.  g_x is a chain of M such terms (M - 1 additions), times fl(1 / M)
       (one rounding in the constant, one in the product): <= (3 + M - 1 + 2) eps g_x = (M + 4) eps g_x.
       V[1] = sum g_y within V1_C eps of itself, V1_C = 3;  V[2] = sum g_x within (M + 4) eps of itself.
       (g_y - g_x)^2 is formed in double from the two fp32 values: its error is |2 (g_y - g_x) (dy - dx)| + (dy - dx)^2 with
       |dy - dx| <= (M + 4) eps (g_y + g_x), so at most 2 (M + 4) eps (g_y + g_x)^2 to first order: V[0] within
       (2 M + 8) eps sum (g_y + g_x)^2 over its pairs.  c(M) = 2 M + 8.
"""
import numpy as np

import fp64_crps_ref as C

KINDS = C.KINDS
EPS = 2.0 ** -24
D2_C = 3.0
V1_C = 3.0


def v0_factor(M):
    return (2 * M + 8) * EPS


def v2_factor(M):
    return (M + 4) * EPS


def offsets(R):
    """written out again, not imported: (0, 1) .. (0, R), then di = 1 .. R each with dj = -R .. R"""
    out = []
    for di in range(0, R + 1):
        for dj in range(-R, R + 1):
            if di > 0 or dj > 0:
                out.append((di, dj))
    return out


def fields(kind, M, T, F, H, W, seed=0):
    """fp64_crps_ref.fields as (M, T, F, H, W), (T, F, H, W)"""
    x, y = C.fields(kind, M, T, F, H * W, seed)
    return x.reshape(M, T, F, H, W), y.reshape(T, F, H, W)


def d2_64(x, y):
    """x (M, planes.., n), y (planes.., n) fp32 -> D2 (planes.., P) float64 by a double loop over the rows"""
    rows = np.concatenate([y[None], x]).astype(np.float64)
    bad = ~np.isfinite(rows).all(axis=-1)
    rows = np.where(bad[..., None], 0.0, rows)
    out = []
    for i in range(rows.shape[0]):
        for j in range(i + 1, rows.shape[0]):
            d = rows[i] - rows[j]
            out.append(np.where(bad[i] | bad[j], np.nan, (d * d).sum(axis=-1)))
    return np.stack(out, axis=-1) if out else np.zeros(y.shape[:-1] + (0,))


def _pw(d, p):
    a = np.abs(d)
    return np.sqrt(a) if p == 0.5 else a if p == 1 else a * a if p == 2 else a ** p


def vario64(x, y, R, p):
    """x (M, planes.., H, W), y (planes.., H, W) fp32 -> (V (planes.., O, 3), S (planes.., O)) float64: the three sums per offset and
    the yardstick sum (g_y + g_x)^2 of the first"""
    M, H, W = x.shape[0], y.shape[-2], y.shape[-1]
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    bad = ~(np.isfinite(xd).all(axis=0) & np.isfinite(yd))
    xd, yd = np.where(bad[None], 0.0, xd), np.where(bad, 0.0, yd)
    offs = offsets(R)
    V, S = np.zeros(y.shape[:-2] + (len(offs), 3)), np.zeros(y.shape[:-2] + (len(offs),))
    for o, (di, dj) in enumerate(offs):
        if di >= H or abs(dj) >= W:
            continue
        ci, cj = slice(0, H - di), slice(max(0, -dj), W - max(0, dj))
        ni, nj = slice(di, H), slice(max(0, dj), W + min(0, dj))
        gy = _pw(yd[..., ci, cj] - yd[..., ni, nj], p)
        gx = _pw(xd[..., ci, cj] - xd[..., ni, nj], p).sum(axis=0) / M
        touched = (bad[..., ci, cj] | bad[..., ni, nj]).any(axis=(-2, -1))
        V[..., o, 0], V[..., o, 1], V[..., o, 2] = ((gy - gx) ** 2).sum(axis=(-2, -1)), gy.sum(axis=(-2, -1)), gx.sum(axis=(-2, -1))
        S[..., o] = ((gy + gx) ** 2).sum(axis=(-2, -1))
        V[..., o, :][touched] = np.nan
    return V, S


_REF = {}


def pairs_reference(kind, M, T, F, hw, seed=0):
    """(x (M, T, F, hw), y (T, F, hw), D2 (T, F, P)) computed once per key, shared and left unchanged"""
    key = ("pairs", kind, M, T, F, hw, seed)
    if key not in _REF:
        x, y = C.fields(kind, M, T, F, hw, seed)
        d2 = d2_64(x, y)
        for a in (x, y, d2):
            a.setflags(write=False)
        _REF[key] = (x, y, d2)
    return _REF[key]


def vario_reference(kind, M, T, F, H, W, R, p, seed=0):
    """(x (M, T, F, H, W), y (T, F, H, W), V (T, F, O, 3), S (T, F, O)) computed once per key, shared and left unchanged"""
    key = ("vario", kind, M, T, F, H, W, R, p, seed)
    if key not in _REF:
        x, y = fields(kind, M, T, F, H, W, seed)
        V, S = vario64(x, y, R, p)
        for a in (x, y, V, S):
            a.setflags(write=False)
        _REF[key] = (x, y, V, S)
    return _REF[key]


def worst(got, f64, limit):
    """(the largest error over its limit -- the limit is 1 -- and whether every entry passes): a NaN must meet a NaN, an entry whose
    limit is 0 must be exact"""
    got, f64, limit = np.asarray(got, dtype=np.float64), np.asarray(f64), np.asarray(limit)
    nan = np.isnan(f64)
    if got.shape != f64.shape or not np.array_equal(np.isnan(got), nan):
        return np.inf, False
    e, lim = np.abs(got - f64)[~nan], limit[~nan]
    ok = bool(np.all(e <= lim))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(e == 0, 0.0, e / lim)
    return (float(r.max()) if r.size else 0.0), ok


def worst_d2(got, d2):
    return worst(got, d2, D2_C * EPS * np.nan_to_num(d2))


def worst_vario(got, V, S, M):
    """the three rules at once: (ratio, ok) over V[..0], V[..1], V[..2]"""
    got = np.asarray(got, dtype=np.float64)
    if got.shape != V.shape:
        return np.inf, False
    r0, ok0 = worst(got[..., 0], V[..., 0], v0_factor(M) * S)
    r1, ok1 = worst(got[..., 1], V[..., 1], V1_C * EPS * np.nan_to_num(V[..., 1]))
    r2, ok2 = worst(got[..., 2], V[..., 2], v2_factor(M) * np.nan_to_num(V[..., 2]))
    return max(r0, r1, r2), ok0 and ok1 and ok2


def energy64(d2, M, beta=1.0, fair=False):
    """(..., P) float64 -> (...): A - B / M^2 or the fair form, by the same algebra"""
    with np.errstate(invalid="ignore", divide="ignore"):
        dist = np.sqrt(d2) ** beta
        a, b = dist[..., :M].sum(axis=-1) / M, dist[..., M:].sum(axis=-1)
        if fair:
            return a - b / (M * (M - 1)) if M > 1 else np.full(a.shape, np.nan)
        return a - b / (M * M)
