"""Event objects of an ensemble on the device: *how many events are there, how big are they, and where?*  ``events.py`` asks per cell
or per box whether a value beyond a threshold was forecast, ``spells.py`` how long it lasts in a cell; neither knows which event cells
belong together.  A member that draws one 900-cell wind storm and one that scatters thirty 30-cell patches over the same region can
share their joint counts and nearly their FSS; their objects tell them apart.

**The event** is that of ``events.py`` (its ``_event_spec`` and ``_indicator`` are used here): ``thresholds (F, K)`` fp32 -- a float64
threshold is rounded once -- with a direction per entry, ``"above"`` (``x >= thr``) or ``"below"`` (``x <= thr``); IEEE comparisons on
exact fp32 values, infinities compare as numbers, a NaN is no event and is counted in ``invalid``.

**Rows.**  ``d = 0`` is the truth if one is given, then the ``M`` members: ``D = M + 1``, or ``M`` without a truth.

**Object.**  A maximal connected set of event cells of one ``(d, t, f, k)`` plane of ``H x W``; ``connectivity`` 4 joins edge
neighbours, 8 (the default) edge and corner neighbours; nothing wraps around.  Its **label** is the smallest linear index ``i W + j``
of its cells: it depends on nothing but the plane.

**The tables** (include/c2w_hip.h: c2w_object_tables), every integer exact:

* ``plane[d, t, f, k, 0..5]``, int64: the number of objects, the event cells, the largest area, the objects that touch the domain's
  border (they are cut by it, so they are censored, as open spells are), ``sum i`` and ``sum j`` over the event cells.
* ``area_hist[d, f, k, b]``, int64 ``(D, F, K, B)``, ``B = floor(log2(H W)) + 1``: the objects of all times with area in
  ``[2^b, 2^(b + 1))``.  An accumulator: ``object_tables(..., area_hist=h)`` adds to ``h``, and planes are independent in time, so a
  year that arrives in blocks needs nothing else (``ObjectTables.merge`` appends the rest).
* ``objects[d, t, f, k, n, 0..7]``, int32: the first ``max_objects`` objects of the plane in label order, each ``(label, area, sum_i,
  sum_j, i_min, i_max, j_min, j_max)``; unused slots are ``label = -1`` and the rest 0.  Objects past the cap are not listed but every
  other table counts them: ``plane[..., 0] - max_objects`` says how many are missing.
* ``invalid[d, t, f]``, int64: the NaN cells.

**The scores** are float64 algebra on the tables: ``object_count_ratio``, ``area_pmf``, ``mean_area``, ``area_distance`` (the
1-Wasserstein distance between the area PMFs of a member and of the truth in bin index), ``largest_object_error``,
``censored_share``, ``centroid_displacement`` (``|c_member - c_truth| / diag`` with ``c = (sum_i, sum_j) / cells`` and ``diag =
hypot(H - 1, W - 1)``: the binary-mass form of the ``L1`` of Wernli's SAL, recalled), ``object_scatter`` and ``location_error`` (its
``L2``, from the lists), ``object_matches`` and ``object_csi`` (centroids within ``max_distance``), and ``objects_report``.

On the GPU ``W`` a multiple of 4, ``H W <= 16384``, ``K <= 8`` and ``max_objects <= 256`` take the kernel (csrc/objects.hip), a
workgroup per plane, labelled in LDS.  Everything else and CPU tensors take the same integers from torch: labels by iterated
neighbour minimum with pointer jumping, which reads ONE FLAG back per round (has anything changed?) -- the only synchronisation of
this module, and only on that route.

Out of scope: intensity-weighted SAL (``S``, ``A``), one-to-one matching, tracking objects through time, objects joint over
variables, periodic domains, plotting.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import object_ops
from .ensemble_host import VariableReport, check_ensemble, chunk_step, datasets, member_mean_std, variable_names
from .ensemble_host import on_device as _on_device
from .events import _event_spec, _indicator

N_OBJECTS, CELLS, LARGEST, CENSORED, SUM_I, SUM_J = range(6)                      # the slots of ``plane``
LABEL, AREA, OBJ_SUM_I, OBJ_SUM_J, I_MIN, I_MAX, J_MIN, J_MAX = range(8)          # the fields of a listed object


def n_bins(H: int, W: int) -> int:
    """``B = floor(log2(H W)) + 1``: the bins of ``area_hist``"""
    return int(H * W).bit_length()


class ObjectTables(NamedTuple):
    """What ``object_tables`` returns (module docstring)"""
    plane: torch.Tensor      # (D, T, F, K, 6) int64
    area_hist: torch.Tensor  # (D, F, K, B) int64
    objects: torch.Tensor    # (D, T, F, K, max_objects, 8) int32
    invalid: torch.Tensor    # (D, T, F) int64
    n_times: int
    shape: Tuple[int, int]   # (H, W)

    def merge(self, other: "ObjectTables") -> "ObjectTables":
        """``other``'s times appended behind these, the histograms added"""
        same = (self.shape == other.shape and tuple(self.area_hist.shape) == tuple(other.area_hist.shape)
                and tuple(self.objects.shape[-2:]) == tuple(other.objects.shape[-2:]) and self.plane.shape[0] == other.plane.shape[0])
        if not same:
            raise ValueError(f"tables of {self.shape}, {tuple(self.area_hist.shape)} bins and lists of {tuple(self.objects.shape[-2:])} "
                             f"cannot take those of {other.shape}, {tuple(other.area_hist.shape)} and {tuple(other.objects.shape[-2:])}")
        return ObjectTables(torch.cat([self.plane, other.plane], dim=1), self.area_hist + other.area_hist,
                            torch.cat([self.objects, other.objects], dim=1), torch.cat([self.invalid, other.invalid], dim=1),
                            self.n_times + other.n_times, self.shape)


# ---------------------------------------------------------------------------------------------------------------------- the tables

def _labels(e: torch.Tensor, connectivity: int) -> torch.Tensor:
    """``e (P, H, W)`` bool -> ``(P, H W)`` int64: the label of every event cell, ``H W`` where there is no event.  Every cell starts as
    its own index; a round takes the minimum over the cell and its neighbours and then, twice, the label of the cell its label names
    (pointer jumping: a label is always a cell of the same object).  Labels only decrease, so the rounds end; ONE FLAG is read back per
    round to see that they have."""
    P, H, W = (int(s) for s in e.shape)
    N = H * W
    flat = e.view(P, N)
    lab = torch.where(e, torch.arange(N, device=e.device).view(1, H, W), N)
    shifts = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    for _ in range(N + 1):
        p = torch.nn.functional.pad(lab, (1, 1, 1, 1), value=N)
        m = lab
        for di, dj in shifts:
            m = torch.minimum(m, p[:, 1 + di:1 + di + H, 1 + dj:1 + dj + W])
        m = torch.where(e, m, N).view(P, N)
        for _ in range(2):
            m = torch.where(flat, torch.gather(m, 1, m.clamp(max=N - 1)), N)
        m = m.view(P, H, W)
        if torch.equal(m, lab):
            break
        lab = m
    return lab.view(P, N)


def _general(x, y, thr, dirn, plane, area_hist, objects, invalid, H: int, W: int, connectivity: int, max_objects: int) -> None:
    """The definition for any shape and any device, chunked over time: x (M, T, F, hw), y (T, F, hw) or None; the tables as
    ``object_ops.object_tables`` takes them.  Areas and sums by ``scatter_add``, the list by the rank of the roots in index order."""
    M, T, F, N = (int(s) for s in x.shape)
    D, K, B = int(plane.shape[0]), int(thr.shape[1]), int(area_hist.shape[-1])
    dev = x.device
    th, dr = thr[:, :, None], dirn[:, :, None]
    cell = torch.arange(N, device=dev)
    ii, jj = (cell // W).view(1, N), (cell % W).view(1, N)
    border = (ii == 0) | (ii == H - 1) | (jj == 0) | (jj == W - 1)
    pow2 = 2 ** torch.arange(1, B, device=dev).view(1, B - 1)
    step = chunk_step(D * F * K * N * 8)
    for s0 in range(0, T, step):
        rows = x[:, s0:s0 + step] if y is None else torch.cat([y[None, s0:s0 + step], x[:, s0:s0 + step]])   # (D, n, F, hw)
        n = int(rows.shape[1])
        P = D * n * F * K
        invalid[:, s0:s0 + n] = torch.isnan(rows).sum(dim=3)
        ev = _indicator(rows[:, :, :, None, :], th, dr).reshape(P, N)                                        # planes in (d, t, f, k) order
        lab = _labels(ev.view(P, H, W), connectivity)
        to = lab.clamp(max=N - 1)                       # a cell without the event adds 0 to entry N - 1
        one = ev.to(torch.int64)
        root = ev & (lab == cell)
        area = torch.zeros((P, N), dtype=torch.int64, device=dev).scatter_add_(1, to, one)
        touch = torch.zeros((P, N), dtype=torch.int64, device=dev).scatter_add_(1, to, one * border)
        out = torch.stack([root.sum(dim=1), one.sum(dim=1), area.amax(dim=1), (root & (touch > 0)).sum(dim=1), (one * ii).sum(dim=1),
                           (one * jj).sum(dim=1)], dim=1)
        plane[:, s0:s0 + n] = out.view(D, n, F, K, 6)
        at = root.nonzero()                                                                                    # (objects, 2): plane, label
        a = area[at[:, 0], at[:, 1]]
        p = at[:, 0]
        group = ((p // (n * F * K)) * F + p // K % F) * K + p % K
        area_hist.view(-1).scatter_add_(0, group * B + (a[:, None] >= pow2).sum(dim=1), torch.ones_like(a))
        if max_objects == 0:
            continue
        rank = torch.gather(root.cumsum(dim=1) - 1, 1, to)                                                    # of the cell's root
        listed = ev & (rank < max_objects)
        slot = torch.where(listed, rank, max_objects)                                                         # the rest to a slot behind the list
        lst = listed.to(torch.int64)
        table = lambda fill: torch.full((P, max_objects + 1), fill, dtype=torch.int64, device=dev)
        fields = [table(-1).scatter_reduce_(1, slot, torch.where(listed & root, cell, -1), "amax"),
                  table(0).scatter_add_(1, slot, lst), table(0).scatter_add_(1, slot, lst * ii), table(0).scatter_add_(1, slot, lst * jj),
                  table(N).scatter_reduce_(1, slot, torch.where(listed, ii, N), "amin"), table(-1).scatter_reduce_(1, slot, torch.where(listed, ii, -1), "amax"),
                  table(N).scatter_reduce_(1, slot, torch.where(listed, jj, N), "amin"), table(-1).scatter_reduce_(1, slot, torch.where(listed, jj, -1), "amax")]
        lists = torch.stack(fields, dim=2)[:, :max_objects]
        used = lists[:, :, LABEL:LABEL + 1] >= 0
        blank = torch.tensor([-1, 0, 0, 0, 0, 0, 0, 0], device=dev)
        objects[:, s0:s0 + n] = torch.where(used, lists, blank).to(torch.int32).view(D, n, F, K, max_objects, 8)


def _launch(x, y, thr, dirn, plane, area_hist, objects, invalid, H: int, W: int, connectivity: int, max_objects: int) -> bool:
    M, T, F, _ = (int(s) for s in x.shape)
    K = int(thr.shape[1])
    if not object_ops.supported(H, W, K, connectivity, max_objects):
        return False
    return object_ops.object_tables(x, y, thr, dirn, plane, area_hist, objects if max_objects else None, invalid, M, T, F, H, W, K, connectivity,
                                    max_objects)


def _count(value, name: str, low: int) -> int:
    if isinstance(value, bool) or int(value) != value or int(value) < low:
        raise ValueError(f"{name} {value!r} must be an integer >= {low}")
    return int(value)


def object_tables(samples: torch.Tensor, truth: Optional[torch.Tensor], thresholds, direction="above", connectivity: int = 8,
                  max_objects: int = 64, area_hist: Optional[torch.Tensor] = None) -> ObjectTables:
    """``samples (M, T, F, H, W)``, ``truth (T, F, H, W)`` or None -> the tables of the module docstring.  Any float dtype and any
    strides: a strided or 16-bit input costs one dense fp32 copy.  ``area_hist``: an int64 ``(D, F, K, B)`` accumulator of an earlier
    call, which is ADDED to and returned; default a new one."""
    if truth is not None:
        check_ensemble(samples, truth, members="M >= 1", floating=True)
    elif samples.dim() != 5 or not samples.is_floating_point() or int(samples.shape[0]) < 1:
        raise ValueError(f"samples {tuple(samples.shape)} ({samples.dtype}) must be floating point (M >= 1, T, F, H, W)")
    if connectivity not in (4, 8) or isinstance(connectivity, bool):
        raise ValueError(f"connectivity {connectivity!r} must be 4 or 8")
    max_objects = _count(max_objects, "max_objects", 0)
    M, T, F, H, W = (int(s) for s in samples.shape)
    if H < 1 or W < 1 or F < 1:
        raise ValueError(f"samples {tuple(samples.shape)} must have F, H, W >= 1")
    x, y, _ = datasets(samples, truth)
    thr, dirn = _event_spec(thresholds, direction, F, x.device)
    D, K, B = M + (0 if truth is None else 1), int(thr.shape[1]), n_bins(H, W)
    if area_hist is None:
        area_hist = torch.zeros((D, F, K, B), dtype=torch.int64, device=x.device)
    elif (tuple(area_hist.shape) != (D, F, K, B) or area_hist.dtype != torch.int64 or area_hist.device != x.device
          or not area_hist.is_contiguous()):
        raise ValueError(f"area_hist {tuple(area_hist.shape)} ({area_hist.dtype}, {area_hist.device}) must be contiguous int64 "
                         f"(D, F, K, B) = ({D}, {F}, {K}, {B}) on {x.device}")
    plane = torch.empty((D, T, F, K, 6), dtype=torch.int64, device=x.device)
    objects = torch.empty((D, T, F, K, max_objects, 8), dtype=torch.int32, device=x.device)
    invalid = torch.empty((D, T, F), dtype=torch.int64, device=x.device)
    args = (x, y, thr, dirn, plane, area_hist, objects, invalid, H, W, connectivity, max_objects)
    if T > 0 and not (_on_device(x) and _launch(*args)):
        _general(*args)
    return ObjectTables(plane, area_hist, objects, invalid, T, (H, W))


# ---------------------------------------------------------------------------------------------------------------------- the algebra

def _number(n: float, like: torch.Tensor) -> torch.Tensor:
    """``n`` as a float64 tensor next to ``like``: a quotient of two tensors is a division on every device"""
    return torch.full((), float(n), dtype=torch.float64, device=like.device)


def _ordered_sum(v: torch.Tensor) -> torch.Tensor:
    """the sum over the last axis in ONE order on every device: the axis padded with zeros to a power of two and halved until one entry
    is left, every step an elementwise add"""
    n = int(v.shape[-1])
    size = 1 << max(0, n - 1).bit_length()
    v = torch.nn.functional.pad(v, (0, size - n))
    while size > 1:
        size //= 2
        v = v[..., :size] + v[..., size:]
    return v[..., 0]


def _plane(plane: torch.Tensor, truth_row: bool = False) -> torch.Tensor:
    if plane.dim() < 5 or int(plane.shape[-1]) != 6 or (truth_row and int(plane.shape[-5]) < 2):
        raise ValueError(f"plane {tuple(plane.shape)} must be (..., D{' >= 2' if truth_row else ''}, T, F, K, 6)" + (", row 0 the truth" if truth_row else ""))
    return plane.to(torch.float64)


def _hist(area_hist: torch.Tensor, truth_row: bool = False) -> torch.Tensor:
    if area_hist.dim() < (4 if truth_row else 1) or int(area_hist.shape[-1]) < 1 or (truth_row and int(area_hist.shape[-4]) < 2):
        raise ValueError(f"area_hist {tuple(area_hist.shape)} must be " + ("(..., D >= 2, F, K, B), row 0 the truth" if truth_row else "(..., B)"))
    return area_hist.to(torch.float64)


def _lists(objects: torch.Tensor, plane: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    if objects.dim() < 6 or int(objects.shape[-1]) != 8 or plane.dim() < 5 or tuple(objects.shape[:-2]) != tuple(plane.shape[:-1]) or int(plane.shape[-1]) != 6:
        raise ValueError(f"objects {tuple(objects.shape)} must be (..., D, T, F, K, max_objects, 8) next to plane {tuple(plane.shape)} = (..., D, T, F, K, 6)")
    return objects.to(torch.float64), plane.to(torch.float64)


def _shape(shape) -> Tuple[int, int]:
    if len(shape) != 2 or int(shape[0]) < 1 or int(shape[1]) < 1:
        raise ValueError(f"shape {tuple(shape)} must be (H, W)")
    return int(shape[0]), int(shape[1])


def object_count_ratio(plane: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``plane (..., D, T, F, K, 6)`` with row 0 the truth -> ``(ratio_t (..., M, T, F, K), ratio (..., M, F, K), bias (..., M, F, K))``
    float64: the number of objects of each member over the truth's per time and pooled over time (NaN for 0 / 0, inf for n / 0), and the
    mean difference per time"""
    n = _plane(plane, True)[..., N_OBJECTS]
    member, truth = n[..., 1:, :, :, :], n[..., :1, :, :, :]
    times = _number(int(n.shape[-3]), n)
    return member / truth, member.sum(dim=-3) / truth.sum(dim=-3), (member - truth).sum(dim=-3) / times


def area_pmf(area_hist: torch.Tensor) -> torch.Tensor:
    """``area_hist (..., B)`` -> float64 of the same shape: the share of the objects with area in ``[2^b, 2^(b + 1))``; NaN without one"""
    h = _hist(area_hist)
    return h / h.sum(dim=-1, keepdim=True)


def mean_area(plane: torch.Tensor) -> torch.Tensor:
    """``plane (..., D, T, F, K, 6)`` -> ``(..., D, F, K)`` float64: event cells over objects, pooled over time; NaN without an object"""
    p = _plane(plane)
    return p[..., CELLS].sum(dim=-3) / p[..., N_OBJECTS].sum(dim=-3)


def area_distance(area_hist: torch.Tensor) -> torch.Tensor:
    """``area_hist (..., D, F, K, B)`` with row 0 the truth -> ``(..., D - 1, F, K)`` float64: the 1-Wasserstein distance between the
    area PMFs of each member and of the truth in bin index (one unit is a doubling of the area), ``sum_{b < B - 1} |P(bin <= b) -
    Q(bin <= b)|``.  NaN where either has no object."""
    h = _hist(area_hist, True)
    cdf = h.cumsum(dim=-1)[..., :-1] / h.sum(dim=-1, keepdim=True)  # integers first, one division: the same bits on every device
    return _ordered_sum((cdf[..., 1:, :, :, :] - cdf[..., :1, :, :, :]).abs())  # not integers: one order of the adds on every device


def largest_object_error(plane: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``plane (..., D, T, F, K, 6)`` with row 0 the truth -> ``(bias, rmse)``, each ``(..., D - 1, F, K)`` float64, of each member's
    largest area against the truth's, over time"""
    a = _plane(plane, True)[..., LARGEST]
    diff = a[..., 1:, :, :, :] - a[..., :1, :, :, :]
    times = _number(int(a.shape[-3]), a)
    return diff.sum(dim=-3) / times, ((diff * diff).sum(dim=-3) / times).sqrt()


def censored_share(plane: torch.Tensor) -> torch.Tensor:
    """``plane (..., D, T, F, K, 6)`` -> ``(..., D, F, K)`` float64: the share of the objects that touch the border; NaN without one"""
    p = _plane(plane)
    return p[..., CENSORED].sum(dim=-3) / p[..., N_OBJECTS].sum(dim=-3)


def _centroid(p: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return p[..., SUM_I] / p[..., CELLS], p[..., SUM_J] / p[..., CELLS]


def centroid_displacement(plane: torch.Tensor, shape) -> torch.Tensor:
    """``plane (..., D, T, F, K, 6)`` with row 0 the truth, ``shape = (H, W)`` -> ``(..., D - 1, T, F, K)`` float64: ``|c_member -
    c_truth| / diag`` with ``c = (sum_i, sum_j) / cells`` the centroid of the event cells and ``diag = hypot(H - 1, W - 1)``; NaN where
    either plane has no event cell"""
    H, W = _shape(shape)
    ci, cj = _centroid(_plane(plane, True))
    di, dj = ci[..., 1:, :, :, :] - ci[..., :1, :, :, :], cj[..., 1:, :, :, :] - cj[..., :1, :, :, :]
    return (di * di + dj * dj).sqrt() / _number(math.hypot(H - 1, W - 1), di)


def object_scatter(objects: torch.Tensor, plane: torch.Tensor) -> torch.Tensor:
    """``objects (..., D, T, F, K, max_objects, 8)``, ``plane (..., D, T, F, K, 6)`` -> ``(..., D, T, F, K)`` float64: ``r = sum_n A_n
    |c_n - c| / sum_n A_n``, the area-weighted mean distance of the objects' centroids ``c_n`` from the plane's centroid ``c``.  NaN
    where the plane has no object, and where its list overflowed"""
    o, p = _lists(objects, plane)
    ci, cj = _centroid(p)
    area = o[..., AREA]
    used = o[..., LABEL] >= 0
    safe = torch.where(used, area, torch.ones_like(area))
    di, dj = o[..., OBJ_SUM_I] / safe - ci[..., None], o[..., OBJ_SUM_J] / safe - cj[..., None]
    terms = torch.where(used, area * (di * di + dj * dj).sqrt(), torch.zeros_like(area))
    r = _ordered_sum(terms) / p[..., CELLS]
    whole = (p[..., N_OBJECTS] >= 1) & (p[..., N_OBJECTS] <= int(o.shape[-2]))
    return torch.where(whole, r, torch.full_like(r, float("nan")))


def location_error(objects: torch.Tensor, plane: torch.Tensor, shape) -> torch.Tensor:
    """-> ``(..., D - 1, T, F, K)`` float64: ``L2 = 2 |r_member - r_truth| / diag`` of ``object_scatter``, row 0 the truth; NaN where
    either is"""
    H, W = _shape(shape)
    _plane(plane, True)
    r = object_scatter(objects, plane)
    return 2.0 * (r[..., 1:, :, :, :] - r[..., :1, :, :, :]).abs() / _number(math.hypot(H - 1, W - 1), r)


def object_matches(objects: torch.Tensor, plane: torch.Tensor, max_distance: float, min_area: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> ``(hits, misses, false_alarms)``, each ``(..., D - 1, T, F, K)`` int64, row 0 the truth, over the LISTED objects of area
    ``>= min_area``: a truth object is a hit for a member if a centroid of that member's objects lies within ``max_distance`` cells of
    its own, else a miss; a member object with no truth centroid within ``max_distance`` is a false alarm.  Not one-to-one."""
    if not (float(max_distance) >= 0.0):
        raise ValueError(f"max_distance {max_distance!r} must be >= 0")
    min_area = _count(min_area, "min_area", 0)
    o, p = _lists(objects, plane)
    _plane(plane, True)
    ok = (o[..., LABEL] >= 0) & (o[..., AREA] >= min_area)
    safe = torch.where(ok, o[..., AREA], torch.ones_like(o[..., AREA]))
    ci, cj = o[..., OBJ_SUM_I] / safe, o[..., OBJ_SUM_J] / safe
    t_i, t_j, t_ok = ci[..., :1, :, :, :, :, None], cj[..., :1, :, :, :, :, None], ok[..., :1, :, :, :, :, None]        # the truth's along the axis before last
    m_i, m_j, m_ok = ci[..., 1:, :, :, :, None, :], cj[..., 1:, :, :, :, None, :], ok[..., 1:, :, :, :, None, :]
    di, dj = m_i - t_i, m_j - t_j
    near = (di * di + dj * dj <= _number(float(max_distance) ** 2, di)) & t_ok & m_ok                                   # (..., M, T, F, K, truth n, member n)
    hit = near.any(dim=-1)
    hits = hit.sum(dim=-1)
    misses = t_ok[..., 0].sum(dim=-1) - hits
    false_alarms = (m_ok[..., 0, :] & ~near.any(dim=-2)).sum(dim=-1)
    return hits, misses, false_alarms


def object_csi(hits: torch.Tensor, misses: torch.Tensor, false_alarms: torch.Tensor) -> torch.Tensor:
    """``hits / (hits + misses + false alarms)``, float64; NaN where all three are 0"""
    if not (tuple(hits.shape) == tuple(misses.shape) == tuple(false_alarms.shape)):
        raise ValueError(f"hits {tuple(hits.shape)}, misses {tuple(misses.shape)} and false_alarms {tuple(false_alarms.shape)} must have one shape")
    h = hits.to(torch.float64)
    return h / (h + misses.to(torch.float64) + false_alarms.to(torch.float64))


# ---------------------------------------------------------------------------------------------------------------------- the report

class ObjectsReport(VariableReport):
    """Per variable, as device tensors, ``K`` thresholds, ``D`` rows (0 the truth), ``T`` times: ``thresholds (K,)``, ``objects``,
    ``cells``, ``largest (D, T, K)``, ``mean_area``, ``censored_share (D, K)``, ``area_pmf (D, K, B)``, ``count_ratio``,
    ``count_bias``, ``area_distance``, ``largest_bias``, ``largest_rmse (M, K)``, ``centroid_displacement``, ``location_error``,
    ``hits``, ``misses``, ``false_alarms (M, T, K)``, ``csi (M, K)`` pooled over time, ``overflowed (D, K)``, the planes whose list
    was cut, and ``invalid (D, T)``, the NaN cells."""

    def as_dict(self, prefix: str = "objects") -> dict:
        """flat ``{f"{prefix}/{name}/count_ratio_k{k}": mean over the members, ..."_std": their population std}``, the same for
        ``area_distance``, ``largest_bias`` and ``csi``, for a logger (one device-to-host copy)"""
        if not self.variables:
            return {}
        rows, keys = [], []
        for name, v in self:
            for k in range(int(v["thresholds"].shape[0])):
                for key in ("count_ratio", "area_distance", "largest_bias", "csi"):
                    rows.append(v[key][:, k])
                    keys.append(f"{prefix}/{name}/{key}_k{k}")
        return member_mean_std(rows, keys)


def objects_report(samples: torch.Tensor, truth: torch.Tensor, thresholds, direction="above", connectivity: int = 8, max_objects: int = 64,
                   max_distance: float = 8.0, min_area: int = 0, names: Optional[Sequence[str]] = None) -> ObjectsReport:
    """The object statistics of an ensemble ``samples (M, L, F, H, W)`` against ``truth (L, F, H, W)`` per variable, from one pass over
    the fields.  ``names``: one per variable, default ``var0 ...``."""
    check_ensemble(samples, truth, time="L", members="M >= 1", floating=True)
    F = int(samples.shape[2])
    names = variable_names(names, F)
    thr, _ = _event_spec(thresholds, direction, F, samples.device)
    t = object_tables(samples, truth, thr, direction, connectivity, max_objects)
    _, ratio, bias = object_count_ratio(t.plane)
    big_bias, big_rmse = largest_object_error(t.plane)
    hits, misses, false_alarms = object_matches(t.objects, t.plane, max_distance, min_area)
    csi = object_csi(hits.sum(dim=1), misses.sum(dim=1), false_alarms.sum(dim=1))
    mean, share, pmf, dist = mean_area(t.plane), censored_share(t.plane), area_pmf(t.area_hist), area_distance(t.area_hist)
    move, spread = centroid_displacement(t.plane, t.shape), location_error(t.objects, t.plane, t.shape)
    over = (t.plane[..., N_OBJECTS] > max_objects).sum(dim=1)
    variables = []
    for f in range(F):
        variables.append(dict(thresholds=thr[f], objects=t.plane[:, :, f, :, N_OBJECTS], cells=t.plane[:, :, f, :, CELLS],
                              largest=t.plane[:, :, f, :, LARGEST], mean_area=mean[:, f], censored_share=share[:, f], area_pmf=pmf[:, f],
                              count_ratio=ratio[:, f], count_bias=bias[:, f], area_distance=dist[:, f], largest_bias=big_bias[:, f],
                              largest_rmse=big_rmse[:, f], centroid_displacement=move[:, :, f], location_error=spread[:, :, f],
                              hits=hits[:, :, f], misses=misses[:, :, f], false_alarms=false_alarms[:, :, f], csi=csi[:, f],
                              overflowed=over[:, f], invalid=t.invalid[:, :, f]))
    return ObjectsReport(names, variables)
