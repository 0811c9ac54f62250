"""The reference of the object tables (climate2weather_amd.objects) in NumPy and plain Python, and the fields the tests run on.

Everything is integers, so every route must EQUAL ``objects_ref``; there is no tolerance anywhere.  It is written as a plain FLOOD FILL,
deliberately not the kernel's algorithm (runs and a union-find) nor the torch route's (iterated neighbour minimum): the plane is
scanned in row-major order, and an event cell nobody has reached yet starts a fill over its 4 or 8 neighbours.  The first cell of a
fill is the smallest index of its object -- the label -- and the fills come in label order, which is the order of the list.

The kinds are the adversarial planes of a labeller: ``empty`` and ``full``; ``checker`` (``H W / 2`` one-cell objects at connectivity
4, one object at 8); ``diagonal``, two blocks that touch at a corner only; ``comb``, teeth that join on the last row, so labels merge
late; ``U`` and nested ``rings``; ``spiral`` and ``serpentine``, one object whose label must travel the whole plane; ``random`` at
event densities 0.3, 0.59 (the site-percolation threshold at connectivity 4) and 0.8; ``smooth``; ``nans``; ``infs``; ``ties`` at the
threshold with both zeros.  Variable ``f`` differs from its neighbours in offset and scale, so a wrong index map fails; the rows and
times differ by a mirror image or by their random draws.
"""
import numpy as np

KINDS = ("empty", "full", "checker", "diagonal", "comb", "U", "rings", "spiral", "serpentine", "random30", "random59", "random80", "smooth",
         "nans", "infs", "ties")
LARGE_KINDS = ("spiral", "serpentine", "checker", "full", "random59")  # what the 128 x 128 plane is asked


def _spiral(H, W):
    g = np.zeros((H, W), bool)
    i = j = 0
    di, dj = 0, 1
    g[0, 0] = True
    inside = lambda a, b: 0 <= a < H and 0 <= b < W
    while True:
        for _ in range(2):
            ni, nj, mi, mj = i + di, j + dj, i + 2 * di, j + 2 * dj
            if inside(ni, nj) and not g[ni, nj] and not (inside(mi, mj) and g[mi, mj]):
                i, j = ni, nj
                g[i, j] = True
                break
            di, dj = dj, -di
        else:
            return g


def _smooth(rng, H, W):
    z = rng.standard_normal((H + 8, W + 8))
    for _ in range(3):
        z = (z + np.roll(z, 1, 0) + np.roll(z, -1, 0) + np.roll(z, 1, 1) + np.roll(z, -1, 1)) / 5.0
    z = z[4:-4, 4:-4]
    return z / max(float(z.std()), 1e-6)


def pattern(kind, H, W, rng, flip=False):
    """u (H, W) float64: the event of the kinds made of two values is u = +1 against -1"""
    i, j = np.indices((H, W))
    if kind == "empty":
        g = np.zeros((H, W), bool)
    elif kind == "full":
        g = np.ones((H, W), bool)
    elif kind == "checker":
        g = (i + j) % 2 == 0
    elif kind == "diagonal":
        g = ((i < H // 2) & (j < W // 2)) | ((i >= H // 2) & (j >= W // 2))
    elif kind == "comb":
        g = (j % 2 == 0) | (i == H - 1)
    elif kind == "U":
        g = (j == 0) | (j == W - 1) | (i == H - 1)
    elif kind == "rings":
        g = np.minimum(np.minimum(i, H - 1 - i), np.minimum(j, W - 1 - j)) % 2 == 0
    elif kind == "spiral":
        g = _spiral(H, W)
    elif kind == "serpentine":
        g = (i % 2 == 0) | ((i % 4 == 1) & (j == W - 1)) | ((i % 4 == 3) & (j == 0))
    elif kind.startswith("random"):
        g = rng.random((H, W)) < int(kind[6:]) / 100.0
    elif kind in ("smooth", "nans", "infs"):
        u = _smooth(rng, H, W)
        if kind == "nans":
            u = np.where(rng.random((H, W)) < 0.06, np.nan, u)
        if kind == "infs":
            r = rng.random((H, W))
            u = np.where(r < 0.05, np.inf, np.where(r > 0.95, -np.inf, u))
        return u[:, ::-1] if flip else u
    elif kind == "ties":
        r = rng.random((H, W))
        return np.where(r < 0.3, 0.0, np.where(r < 0.6, -0.0, np.round(rng.standard_normal((H, W)) * 2.0) / 2.0))
    else:
        raise KeyError(kind)
    g = g[:, ::-1] if flip else g
    return np.where(g, 1.0, -1.0)


def _affine(kind, F):
    f = np.arange(F, dtype=np.float64)
    return (0.0 * f, 1.0 + 0.0 * f) if kind == "ties" else (10.0 * f, 1.0 + f)


def fields(kind, M, T, F, H, W, seed=0):
    """x (M, T, F, H W), y (T, F, H W) fp32; row d at time t is mirrored where d + t is odd"""
    rng = np.random.default_rng([seed, KINDS.index(kind), M, T, F, H, W])
    off, scl = _affine(kind, F)
    v = np.zeros((M + 1, T, F, H, W), np.float64)
    for d in range(M + 1):
        for t in range(T):
            for f in range(F):
                v[d, t, f] = off[f] + scl[f] * pattern(kind, H, W, rng, flip=(d + t) % 2 == 1)
    v = v.astype(np.float32).reshape(M + 1, T, F, H * W)
    return np.ascontiguousarray(v[1:]), np.ascontiguousarray(v[0])


def thresholds(kind, F, K):
    """(F, K) fp32: levels inside the gap of the two-valued kinds, spread over the continuous ones, the special values of the rest"""
    off, scl = _affine(kind, F)
    wide = 0.8 if kind in ("smooth", "nans", "infs") else 0.5
    levels = np.linspace(-wide, wide, K) if K > 1 else np.zeros(1)
    thr = (off[:, None] + scl[:, None] * levels[None]).astype(np.float32)
    if kind == "ties":
        thr[:] = np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 0.0, -0.0], np.float32)[:K]
    if kind == "infs":
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


def n_bins(hw):
    return int(hw).bit_length()  # floor(log2(hw)) + 1


def fill(e, connectivity):
    """e (H, W) bool -> the objects in label order, each the list of its cells (i, j), the first of them the label's cell"""
    H, W = e.shape
    P = W + 2
    todo = np.zeros((H + 2, P), bool)
    todo[1:-1, 1:-1] = e
    todo = todo.ravel().tolist()
    steps = (-P, -1, 1, P) if connectivity == 4 else (-P - 1, -P, -P + 1, -1, 1, P - 1, P, P + 1)
    out = []
    for at in range(P + 1, (H + 1) * P):
        if not todo[at]:
            continue
        todo[at] = False
        stack, cells = [at], []
        while stack:
            c = stack.pop()
            cells.append((c // P - 1, c % P - 1))
            for s in steps:
                if todo[c + s]:
                    todo[c + s] = False
                    stack.append(c + s)
        out.append(cells)
    return out


def indicator(rows, thr, above):
    """rows (D, T, F, hw) fp32 -> bool (D, T, F, K, hw)"""
    assert rows.dtype == np.float32 and thr.dtype == np.float32
    v, t, a = rows[:, :, :, None, :], thr[None, None, :, :, None], above[None, None, :, :, None]
    with np.errstate(invalid="ignore"):
        return np.where(a, v >= t, v <= t)


def objects_ref(x, y, thr, above, H, W, connectivity=8, max_objects=64):
    """dict of plane (D, T, F, K, 6) int64, area_hist (D, F, K, B) int64, objects (D, T, F, K, max_objects, 8) int32, invalid (D, T, F)
    int64 for the rows y (or none), x"""
    rows = x if y is None else np.concatenate([y[None], x])
    D, T, F, hw = rows.shape
    assert hw == H * W
    K, B = thr.shape[1], n_bins(hw)
    e = indicator(rows, thr, above).reshape(D, T, F, K, H, W)
    plane = np.zeros((D, T, F, K, 6), np.int64)
    hist = np.zeros((D, F, K, B), np.int64)
    objs = np.zeros((D, T, F, K, max_objects, 8), np.int32)
    objs[..., 0] = -1
    for d, t, f, k in np.ndindex(D, T, F, K):
        found = fill(e[d, t, f, k], connectivity)
        row = plane[d, t, f, k]
        row[0] = len(found)
        for n, cells in enumerate(found):
            ii, jj = np.array(cells).T
            area = len(cells)
            row[1] += area
            row[2] = max(row[2], area)
            row[3] += int(ii.min() == 0 or jj.min() == 0 or ii.max() == H - 1 or jj.max() == W - 1)
            row[4] += ii.sum()
            row[5] += jj.sum()
            hist[d, f, k, area.bit_length() - 1] += 1
            if n < max_objects:
                objs[d, t, f, k, n] = (cells[0][0] * W + cells[0][1], area, ii.sum(), jj.sum(), ii.min(), ii.max(), jj.min(), jj.max())
    return dict(plane=plane, area_hist=hist, objects=objs, invalid=np.isnan(rows).sum(axis=3).astype(np.int64))
