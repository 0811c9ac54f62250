"""The float64 side of the wind-power tests (climate2weather_amd.windpower, csrc/wind.hip): the definition, the curves, the field kinds,
and the rule an fp32 result is held to.

The definition (include/c2w_hip.h: c2w_wind_power), with the fp32 inputs read as doubles: per cell
    speed = numpy.sqrt(u * u + v * v) * c,  c = (hub_height / reference_height) ** alpha in float64
    power = numpy.interp(speed, xs, ps, left=0, right=0)
and per (d, t) plane numpy.sum of each over its cells.  Where u * u + v * v lies beyond the fp32 range the fp32 definition gives speed
+inf (power 0): the reference says inf there too (the generator keeps such sums away from the boundary by a factor 2^-20 and asserts it).

The rule is derived from the arithmetic of csrc/wind_core.h, not fitted.  eps = 2^-24, the unit roundoff of fp32.

Speed.  fl(u u), fl(v v), their sum, the square root, the factor rounded to fp32, the product: six roundings.  The two squares are not
negative, so the sum carries at most two of the three (1 + eps) factors relative to itself and the square root halves them -- the count
of six is already generous, and (1 + eps)^6 - 1 <= 6 eps (1 + 2^-20).  Where a square or the sum falls below the normal range it is
off by at most 2^-126 absolutely (flushed to zero, or rounded to a subnormal) instead: together less than 2^-124 on the sum, and
|sqrt(q + e) - sqrt(q)| <= sqrt(|e|) = 2^-62 on the root.  Hence
    |speed32 - speed64| <= delta_s = 6 eps (1 + 2^-20) speed64 + 2^-62 c.

Power.  The table holds the knots rounded to fp32, x^_j, the powers rounded to fp32, and slope_j = (p_{j+1} - p_j) / (x^_{j+1} - x^_j)
formed in float64 from the ROUNDED knots: exactly evaluated it is the piecewise-linear curve through (x^_j, p_j), whose value at s is the
float64 curve's value at t = x_j + (s - x^_j) (x_{j+1} - x_j) / (x^_{j+1} - x^_j), and t - s is a convex combination of the two knots'
roundings: |t - s| <= delta_k = eps max|xs|.  So the exact table value at speed32 is a value of the float64 curve on
[speed64 - delta, speed64 + delta], delta = delta_s + delta_k, hence between the least and the largest value of the curve there (taken
at the ends of the window and at every knot inside it).  At or beyond the ends of the curve the kernel says p_{K-1} or 0; the window
then reaches xs[0] or xs[-1], and the set includes 0.  On top come the roundings of the interpolation itself, each relative to
pm = the largest |p| among the knots of the intervals the window touches: p_j rounded (eps |p_j|), the slope rounded, the subtraction
and the multiplication (eps |p_{j+1} - p_j| <= 2 eps pm each), the addition (eps |result| <= eps pm): 8 eps pm to first order, 9 eps pm
with every second-order term.  A window that lies outside the curve altogether allows nothing but 0.

Sums.  A sum is within the sum of its cells' bounds (the double accumulation adds 2^-53 per term, which does not show).

The condition on the inputs: the either-branch allowance at xs[0] and xs[-1] must stay rare, or it would hide a wrong sum.  In every
kind but "on_knots" -- which targets the knots and the cut-out, and is checked for equality -- at most 1 % of the cells may have xs[0]
or xs[-1] inside their window; ``reference`` asserts it.
"""
import numpy as np

KINDS = ("calm", "typical", "storm", "on_knots", "tiny", "huge", "nonfinite")
CURVES = ("k2", "k3", "k61", "crowded", "tenths")
EPS = 2.0 ** -24
SPEED_ROUNDINGS = 6 * EPS * (1 + 2.0 ** -20)
SPEED_FLOOR = 2.0 ** -62
POWER_ROUNDINGS = 9 * EPS
F32_MAX = float(np.finfo(np.float32).max)
RATED = 2.0e6  # W; no turbine's numbers: a cubic ramp to a round rated power


def hub_factor(hub_height=100.0, reference_height=10.0, alpha=1.0 / 7.0):
    return (hub_height / reference_height) ** alpha


# ------------------------------------------------------------------------------------------------------------------ the curves

def _ramp(xs, cut_in, rated_at):
    return RATED * np.clip((xs - cut_in) / (rated_at - cut_in), 0.0, 1.0) ** 3


def curve(name):
    """(xs, ps) float64.  k2: two knots; k3: three, not uniform; k61: 0.5 m/s steps from the cut-in at 2 m/s, a ramp to 12 m/s, the
    rated plateau, the last knot at rated power; crowded: 256 knots, 120 of them within 0.5 m/s and 120 within 0.3 m/s, so that a
    bucket of the kernel's index holds about twenty (the lookup's fallback); tenths: 251 knots in steps of 0.1, none of them an fp32."""
    if name == "k2":
        xs, ps = np.array([3.0, 25.0]), np.array([0.0, RATED])
    elif name == "k3":
        xs, ps = np.array([2.5, 11.0, 25.0]), np.array([0.0, RATED, 0.9 * RATED])
    elif name == "k61":
        xs = 2.0 + 0.5 * np.arange(61)
        ps = _ramp(xs, 2.0, 12.0)
    elif name == "crowded":
        xs = np.concatenate([np.linspace(3.0, 3.5, 120), np.linspace(12.0, 12.3, 120), np.linspace(13.0, 25.0, 16)])
        ps = _ramp(xs, 3.0, 12.3)
    elif name == "tenths":
        xs = np.arange(1, 252) / 10.0
        ps = _ramp(xs, 3.0, 11.0)
    else:
        raise KeyError(name)
    assert np.all(np.diff(xs) > 0) and xs[0] > 0 and xs.shape == ps.shape
    return xs.astype(np.float64), ps.astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------ the fields

def fields(kind, curve_name, D, T, F, hw, u, v, seed=0):
    """(x (D, T, F, hw) fp32, c): the wind components in variables u and v, every other variable filled with values far from any
    wind (a wrong plane index fails); neighbouring (d, t) planes differ in offset and scale.  The speeds below are at hub height.
    calm: below 0.9 xs[0]; typical: Weibull-like (shape 2, scale 8), 0 - 25 m/s (capped at 24.9); storm: 15 - 40 m/s, a sizeable share above the
    cut-out; on_knots: hub factor 1, v = 0, u a knot rounded to fp32 or one of its fp32 neighbours, both signs; tiny: magnitudes
    1e-30 - 1e-20 (the squares underflow); huge: 1e20 - 1e30 (the squares overflow); nonfinite: typical with a NaN u, a NaN v, an
    infinite u and an infinite v planted in four cells (of four different planes where there are as many)."""
    xs, ps = curve(curve_name)
    rng = np.random.default_rng([seed, KINDS.index(kind), CURVES.index(curve_name), D, T, F, hw, u, v])
    c = 1.0 if kind == "on_knots" else hub_factor()
    shape = (D, T, hw)
    plane_scale = (1.0 - 0.05 * np.arange(D * T).reshape(D, T, 1) / max(1, D * T))  # every plane a little different, all <= 1
    if kind == "calm":
        hub = 0.9 * xs[0] * rng.uniform(0.0, 1.0, shape)
    elif kind in ("typical", "nonfinite"):
        hub = np.minimum(8.0 * rng.weibull(2.0, shape), 24.9)  # the cap stays clear of a cut-out at 25
    elif kind == "storm":
        hub = rng.uniform(15.0, 40.0, shape)
    elif kind == "tiny":
        hub = 10.0 ** rng.uniform(-30.0, -20.0, shape)
    elif kind == "huge":
        hub = 10.0 ** rng.uniform(20.0, 30.0, shape)
    else:
        hub = np.zeros(shape)
    theta = rng.uniform(0.0, 2.0 * np.pi, shape)
    r = hub * plane_scale / c
    x = (1000.0 + 50.0 * np.arange(F)[None, None, :, None] + 7.0 * rng.standard_normal((D, T, F, hw))).astype(np.float32)
    x[:, :, u], x[:, :, v] = (r * np.cos(theta)).astype(np.float32), (r * np.sin(theta)).astype(np.float32)
    if kind == "on_knots":
        x32 = xs.astype(np.float32)
        k = np.arange(D * T * hw).reshape(shape)
        knot = x32[(k // 3) % xs.shape[0]]
        side = k % 3  # the knot, the fp32 below it, the fp32 above it
        val = np.where(side == 0, knot, np.where(side == 1, np.nextafter(knot, np.float32(-np.inf)), np.nextafter(knot, np.float32(np.inf))))
        val[..., -1] = x32[-1]                                           # the cut-out itself: ps[-1]
        if hw >= 4:
            val[..., -2] = np.nextafter(x32[-1], np.float32(np.inf))     # one ulp above it: 0
            val[..., -3] = np.nextafter(x32[0], np.float32(-np.inf))     # one ulp below the first knot: 0
            val[..., -4] = x32[0]
        x[:, :, u], x[:, :, v] = np.where(k % 2 == 0, val, -val).astype(np.float32), np.float32(0.0)
    if kind == "nonfinite":
        x[0, 0, u, hw // 2] = np.nan
        x[D - 1, T - 1, v, hw - 1] = np.nan
        x[D // 2, 0, u, 0] = np.inf
        x[0, T // 2, v, 1] = -np.inf
    return x, c


# ------------------------------------------------------------------------------------------------------------------ the definition

def speed64(u, v, c):
    """fp32 components -> the float64 speed; +inf where u u + v v is beyond the fp32 range (module docstring)"""
    ud, vd = u.astype(np.float64), v.astype(np.float64)
    with np.errstate(all="ignore"):
        q = ud * ud + vd * vd
        s = np.sqrt(q) * c
    over = q >= 2.0 ** 128
    edge = (q > F32_MAX * (1 - 2.0 ** -20)) & (q < 2.0 ** 128 * (1 + 2.0 ** -20))
    assert not edge.any(), "a sum of squares at the edge of the fp32 range: neither answer is wrong there"
    return np.where(over, np.inf, s)


def power64(s, xs, ps):
    return np.interp(s, xs, ps, left=0.0, right=0.0)


def bounds(s, c, xs, ps):
    """per cell: delta_s, the least and the largest power the rule allows, and whether xs[0] or xs[-1] lies inside the window"""
    fin = np.isfinite(s)
    sf = np.where(fin, s, 0.0)
    ds = np.where(fin, SPEED_ROUNDINGS * sf + SPEED_FLOOR * c, 0.0)
    delta = ds + EPS * np.abs(xs).max()
    lo, hi = sf - delta, sf + delta
    inside = (hi >= xs[0]) & (lo <= xs[-1])                     # the window touches the curve
    a, b = np.clip(lo, xs[0], xs[-1]), np.clip(hi, xs[0], xs[-1])
    pa, pb = power64(a, xs, ps), power64(b, xs, ps)
    p_lo, p_hi = np.minimum(pa, pb), np.maximum(pa, pb)
    ja = np.clip(np.searchsorted(xs, a, side="right") - 1, 0, xs.shape[0] - 2)
    jb = np.clip(np.searchsorted(xs, b, side="right") - 1, 0, xs.shape[0] - 2)
    pm = np.maximum(np.abs(ps[ja]), np.abs(ps[jb + 1]))
    some = np.flatnonzero((jb > ja).reshape(-1))               # windows with a knot inside: rare but for on_knots
    if some.size:
        fl_lo, fl_hi, fl_pm = p_lo.reshape(-1), p_hi.reshape(-1), pm.reshape(-1)
        for j in range(xs.shape[0]):
            m = some[(ja.reshape(-1)[some] <= j) & (j <= jb.reshape(-1)[some] + 1)]
            fl_pm[m] = np.maximum(fl_pm[m], abs(ps[j]))
            m = m[(xs[j] >= a.reshape(-1)[m]) & (xs[j] <= b.reshape(-1)[m])]
            fl_lo[m], fl_hi[m] = np.minimum(fl_lo[m], ps[j]), np.maximum(fl_hi[m], ps[j])
    edge = inside & ((lo <= xs[0]) | (hi >= xs[-1]))            # the kernel may be on the other side of an end: 0 is allowed
    p_lo, p_hi = np.where(edge, np.minimum(p_lo, 0.0), p_lo), np.where(edge, np.maximum(p_hi, 0.0), p_hi)
    w = POWER_ROUNDINGS * pm
    p_lo, p_hi = np.where(inside, p_lo - w, 0.0), np.where(inside, p_hi + w, 0.0)
    p_lo, p_hi = np.where(fin, p_lo, 0.0), np.where(fin, p_hi, 0.0)  # +inf: 0 exactly
    near = fin & (((lo <= xs[0]) & (xs[0] <= hi)) | ((lo <= xs[-1]) & (xs[-1] <= hi)))
    return ds, p_lo, p_hi, near


class Ref:
    """x (D, T, F, hw) fp32, c; speed, power (D, T, hw) float64 and their sums (D, T, 2); d_speed, p_lo, p_hi per cell and summed"""


_REF = {}


def reference_of(x, c, xs, ps, u, v, targets_the_ends=False):
    """the float64 side of fields x (..., F, hw) fp32 with the hub factor c; asserts the condition on the inputs"""
    r = Ref()
    r.x, r.c, r.xs, r.ps = x, c, xs, ps
    r.speed = speed64(x[..., u, :], x[..., v, :], c)
    with np.errstate(invalid="ignore"):
        r.power = power64(r.speed, xs, ps)
        r.d_speed, r.p_lo, r.p_hi, near = bounds(r.speed, c, xs, ps)
        nan = np.isnan(r.speed)
        r.p_lo, r.p_hi = np.where(nan, np.nan, r.p_lo), np.where(nan, np.nan, r.p_hi)
        assert np.all((r.p_lo <= r.power) & (r.power <= r.p_hi) | nan)
        if not targets_the_ends:
            assert near.mean() <= 0.01, float(near.mean())
        r.sums = np.stack([r.speed.sum(axis=-1), r.power.sum(axis=-1)], axis=-1)
        r.d_sums = r.d_speed.sum(axis=-1)
        r.s_lo, r.s_hi = r.p_lo.sum(axis=-1), r.p_hi.sum(axis=-1)
    for a in (r.x, r.speed, r.power, r.d_speed, r.p_lo, r.p_hi, r.sums, r.d_sums, r.s_lo, r.s_hi):
        a.setflags(write=False)
    return r


def reference(kind, curve_name, D, T, F, hw, u, v, seed=0):
    """computed once per key, shared by the tests that need it and left unchanged"""
    key = (kind, curve_name, D, T, F, hw, u, v, seed)
    if key not in _REF:
        x, c = fields(kind, curve_name, D, T, F, hw, u, v, seed)
        _REF[key] = reference_of(x, c, *curve(curve_name), u, v, targets_the_ends=kind == "on_knots")
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------------ the rule

def _ratio(got, f64, below, above):
    """the largest error over its bound (the limit is 1) and whether every entry passes: an error downwards is held to `below`,
    upwards to `above`; a NaN must meet a NaN, an infinity itself, an entry whose bound is 0 must be exact"""
    got, f64 = np.asarray(got, dtype=np.float64), np.asarray(f64, dtype=np.float64)
    below, above = np.broadcast_to(below, f64.shape), np.broadcast_to(above, f64.shape)
    if got.shape != f64.shape or not np.array_equal(np.isnan(got), np.isnan(f64)):
        return np.inf, False
    fin = np.isfinite(f64)
    if not np.array_equal(got[~fin & ~np.isnan(f64)], f64[~fin & ~np.isnan(f64)]):
        return np.inf, False
    if not np.isfinite(got[fin]).all():
        return np.inf, False
    e = got[fin] - f64[fin]
    lim = np.where(e >= 0, above[fin], below[fin])
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(e == 0, 0.0, np.abs(e) / lim)
    worst = float(r.max()) if r.size else 0.0
    return worst, bool(worst <= 1.0)


def worst_speed(got, ref):
    return _ratio(got, ref.speed, ref.d_speed, ref.d_speed)


def worst_power(got, ref):
    with np.errstate(invalid="ignore"):
        return _ratio(got, ref.power, ref.power - ref.p_lo, ref.p_hi - ref.power)


def worst_sums(got, ref):
    """(speed sums, power sums): each (ratio, ok)"""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (_ratio(got[..., 0], ref.sums[..., 0], ref.d_sums, ref.d_sums),
                _ratio(got[..., 1], ref.sums[..., 1], ref.sums[..., 1] - ref.s_lo, ref.s_hi - ref.sums[..., 1]))


# ------------------------------------------------------------------------------------------------------------------ derived series

def series64(sums, hw):
    """sums (..., T, 2) -> (mean power (..., T), cumulative energy (..., T)) by the reference's numpy lines: ``np.cumsum(power.mean((-2,
    -1)) / 1e3)``"""
    mean = sums[..., 1] / hw
    return mean, np.cumsum(mean / 1e3, axis=-1)
