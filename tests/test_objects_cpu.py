"""CPU checks of the event objects (climate2weather_amd.objects): both routes of a call -- the general torch one and the launcher's,
with tests/emu_object_ops.py standing in for the HIP kernel -- EQUAL to the flood fill of tests/fp64_objects_ref.py on every kind of
field at both connectivities; the known answers, all exact; the identities between the tables and against events.event_counts; the
list cap; merge and the accumulator; the algebra on hand-made tables, NaN rules included; every ValueError; the launcher declining
what the kernel does not take; what c2w_object_tables refuses and with which code; the kernel's own maps and link / flatten arithmetic
compiled for the host (csrc/objects_maps.h), once plain and once under the address and undefined-behaviour sanitizers; the two
core_side checks on that header; and the C declarations against the ctypes prototypes."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import c_abi
import emu_object_ops
import fp64_objects_ref as R
import host_program
from climate2weather_amd import _lib, build
from climate2weather_amd import events as EV
from climate2weather_amd import object_ops
from climate2weather_amd import objects as OB
from climate2weather_amd.ensemble_host import VariableReport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "climate2weather_amd", "csrc")
NAMES = ("plane", "area_hist", "objects", "invalid")


@pytest.fixture(params=["general", "launcher"])
def route(request, monkeypatch):
    """both branches of objects.object_tables on CPU tensors"""
    if request.param == "launcher":
        emu_object_ops.install(monkeypatch, object_ops, OB)
    return request.param


def _case(kind, M, T, F, H, W, K, direction="mixed", seed=0):
    """the arrays of the reference and the tensors of the public interface"""
    x, y = R.fields(kind, M, T, F, H, W, seed)
    thr, above = R.thresholds(kind, F, K), R.directions(F, K, direction)
    return x, y, thr, above, torch.tensor(x).view(M, T, F, H, W), torch.tensor(y).view(T, F, H, W), torch.tensor(thr), R.direction_names(above)


def _assert_equal_ref(t, want, what=""):
    assert t.plane.dtype == torch.int64 and t.area_hist.dtype == torch.int64 and t.invalid.dtype == torch.int64 and t.objects.dtype == torch.int32
    for name in NAMES:
        got = getattr(t, name).numpy()
        assert got.shape == want[name].shape and np.array_equal(got, want[name]), (name, what)


def _assert_same_tables(a, b, what=""):
    assert a.n_times == b.n_times and a.shape == b.shape, what
    for name in NAMES:
        assert torch.equal(getattr(a, name), getattr(b, name)), (name, what)


def _planes(masks):
    """masks (T, H, W) of 0 / 1 -> samples (1, T, 1, H, W) fp32 with the event at values >= 1"""
    return torch.tensor(np.asarray(masks), dtype=torch.float32)[None, :, None]


ONE = torch.tensor([[1.0]])


# ------------------------------------------------------------------------------------------------------------------ against the reference

@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H,W,M,K,cap", [(1, 4, 1, 1, 1), (5, 12, 3, 2, 64), (16, 20, 2, 3, 4), (9, 8, 1, 8, 0)])
def test_the_tables_equal_the_reference(route, H, W, M, K, cap, connectivity):
    """every kind at every shape and both connectivities; with and without a truth; mixed directions; caps of 0, 1, a few and plenty"""
    for i, kind in enumerate(R.KINDS):
        with_truth = i % 2 == 0
        x, y, thr, above, S, Tr, th, names = _case(kind, M, 2, 2, H, W, K, ("mixed", "above", "below")[i % 3])
        t = OB.object_tables(S, Tr if with_truth else None, th, names, connectivity, cap)
        assert t.n_times == 2 and t.shape == (H, W) and t.area_hist.shape == (M + with_truth, 2, K, R.n_bins(H * W))
        _assert_equal_ref(t, R.objects_ref(x, y if with_truth else None, thr, above, H, W, connectivity, cap), kind)
    if route == "launcher":
        assert len(emu_object_ops.CALLS) == len(R.KINDS) and emu_object_ops.CALLS[0] == (M, 2, 2, H, W, K, connectivity, cap)


def test_the_general_route_serves_what_the_kernel_does_not(route):
    """W no multiple of 4, and a plane over 16384 cells: the launcher is not reached, the integers are the reference's"""
    for kind, H, W in (("random59", 7, 9), ("serpentine", 6, 10), ("rings", 132, 128)):
        x, y, thr, above, S, Tr, th, names = _case(kind, 1, 1, 1, H, W, 1, "above")
        _assert_equal_ref(OB.object_tables(S, Tr, th, names, 4, 8), R.objects_ref(x, y, thr, above, H, W, 4, 8), kind)
    assert not [c for c in emu_object_ops.CALLS if route == "launcher"]


def test_the_general_route_chunked_over_time_gives_the_same_tables(monkeypatch):
    monkeypatch.setattr(OB, "chunk_step", lambda per_item: 2)  # 5 times in chunks of 2: the last chunk is short
    for kind in ("smooth", "nans", "random30"):
        x, y, thr, above, S, Tr, th, names = _case(kind, 2, 5, 2, 6, 8, 3)
        _assert_equal_ref(OB.object_tables(S, Tr, th, names, 8, 5), R.objects_ref(x, y, thr, above, 6, 8, 8, 5), kind)


# ------------------------------------------------------------------------------------------------------------------ known answers

def test_the_known_answers(route):
    H, W = 12, 16
    i, j = np.indices((H, W))
    ring = np.maximum(np.abs(i - 5), np.abs(j - 7)) == 3                                      # a square ring of side 7 around (5, 7)
    blocks = ((i < 6) & (j < 8)) | ((i >= 6) & (j >= 8))
    S = _planes([(i + j) % 2 == 0, np.ones((H, W)), blocks, ring, np.zeros((H, W))])
    for conn, n_checker, n_blocks in ((4, H * W // 2, 2), (8, 1, 1)):
        t = OB.object_tables(S, None, ONE, "above", conn, 4)
        p = t.plane[0, :, 0, 0]
        assert p[:, 0].tolist() == [n_checker, 1, n_blocks, 1, 0] and p[:, 1].tolist() == [H * W // 2, H * W, H * W // 2, 24, 0]
        assert p[:, 2].tolist() == [H * W // 2 if conn == 8 else 1, H * W, H * W // 2 if conn == 8 else H * W // 4, 24, 0]
        assert p[:, 3].tolist() == [H + W - 2 if conn == 4 else 1, 1, n_blocks, 0, 0]
        o = t.objects[0, :, 0, 0]
        assert o[1, 0].tolist() == [0, H * W, W * H * (H - 1) // 2, H * W * (W - 1) // 2, 0, H - 1, 0, W - 1] and o[1, 1].tolist() == [-1] + [0] * 7
        assert o[3, 0].tolist() == [2 * W + 4, 24, 24 * 5, 24 * 7, 2, 8, 4, 10] and o[4, :, 0].tolist() == [-1] * 4     # the ring's box and sums
        ci, cj = OB._centroid(t.plane.double())
        assert ci[0, 3, 0, 0].item() == 5.0 and cj[0, 3, 0, 0].item() == 7.0                                           # and its centroid
        hist = t.area_hist[0, 0, 0].tolist()
        assert hist[R.n_bins(H * W) - 1] == 1 and sum(hist) == int(p[:, 0].sum())                                      # the full plane: the last bin


def test_the_identities_between_the_tables_and_against_event_counts(route):
    M, T, F, H, W, K = 3, 3, 2, 8, 12, 3
    for kind in ("smooth", "random59", "nans"):
        x, y, thr, above, S, Tr, th, names = _case(kind, M, T, F, H, W, K)
        t = OB.object_tables(S, Tr, th, names, 8, 96)                                            # 96 = H W: no list overflows
        assert torch.equal(t.objects[..., 1].sum(dim=-1, dtype=torch.int64), t.plane[..., 1])    # the list's areas are the event cells
        assert torch.equal((t.objects[..., 0] >= 0).sum(dim=-1), t.plane[..., 0])
        assert torch.equal(t.objects[..., 2].sum(dim=-1, dtype=torch.int64), t.plane[..., 4]) and torch.equal(t.objects[..., 3].sum(dim=-1, dtype=torch.int64), t.plane[..., 5])
        assert torch.equal(t.area_hist.sum(dim=-1), t.plane[..., 0].sum(dim=1))                  # every object is in one bin
        assert torch.equal(t.objects[..., 1].amax(dim=-1).to(torch.int64), t.plane[..., 2])
        # the event cells of one member against the truth alone: the joint table of events.event_counts at M = 1
        for m in range(M):
            counts, invalid = EV.event_counts(S[m:m + 1], Tr, th, names)                         # (T, F, K, 2, 2), (T, F)
            if int(invalid.sum()) == 0:
                assert torch.equal(counts[..., 1].sum(dim=-1), t.plane[m + 1, ..., 1]) and torch.equal(counts[..., 1, :].sum(dim=-1), t.plane[0, ..., 1])
        assert torch.equal(t.invalid, torch.isnan(torch.cat([Tr[None], S])).sum(dim=(-1, -2)))


def test_the_list_cap(route):
    """a plane with exactly max_objects, max_objects + 1 and 0 objects: the list holds the first max_objects in label order, the other
    tables count every object, unused slots are -1, 0 ..."""
    H, W, cap = 4, 12, 3
    dots = lambda n: [[1.0 if (i == 1 and j % 2 == 0 and j // 2 < n) else 0.0 for j in range(W)] for i in range(H)]
    t = OB.object_tables(_planes([dots(3), dots(4), dots(0)]), None, ONE, "above", 8, cap)
    assert t.plane[0, :, 0, 0, 0].tolist() == [3, 4, 0] and t.plane[0, :, 0, 0, 1].tolist() == [3, 4, 0]
    labels = t.objects[0, :, 0, 0, :, 0].tolist()
    assert labels == [[W, W + 2, W + 4], [W, W + 2, W + 4], [-1, -1, -1]]
    assert t.objects[0, 2, 0, 0].abs().sum().item() == 3 and t.area_hist[0, 0, 0].tolist() == [7, 0, 0, 0, 0, 0]
    r = OB.object_scatter(t.objects, t.plane)[0, :, 0, 0]
    assert not math.isnan(r[0].item()) and math.isnan(r[1].item()) and math.isnan(r[2].item())   # whole; overflowed; no object
    none = OB.object_tables(_planes([dots(4)]), None, ONE, "above", 8, 0)
    assert none.objects.shape == (1, 1, 1, 1, 0, 8) and none.plane[0, 0, 0, 0, 0].item() == 4


def test_merge_and_the_accumulator_equal_one_call(route):
    x, y, thr, above, S, Tr, th, names = _case("random30", 2, 5, 2, 8, 12, 2)
    whole = OB.object_tables(S, Tr, th, names, 4, 8)
    _assert_equal_ref(whole, R.objects_ref(x, y, thr, above, 8, 12, 4, 8))
    first, rest = OB.object_tables(S[:, :2], Tr[:2], th, names, 4, 8), OB.object_tables(S[:, 2:], Tr[2:], th, names, 4, 8)
    _assert_same_tables(first.merge(rest), whole)
    kept = first.area_hist.clone()
    second = OB.object_tables(S[:, 2:], Tr[2:], th, names, 4, 8, area_hist=kept)
    assert second.area_hist is kept and torch.equal(kept, whole.area_hist)
    empty = OB.object_tables(S[:, :0], Tr[:0], th, names, 4, 8)                                  # no times: empty tables, a zero histogram
    assert empty.n_times == 0 and empty.plane.shape == (3, 0, 2, 2, 6) and int(empty.area_hist.sum()) == 0
    _assert_same_tables(empty.merge(whole), whole)


# ------------------------------------------------------------------------------------------------------------------ the algebra

def test_the_algebra_on_hand_made_tables():
    # D = 3 rows (truth, two members), T = 2, F = K = 1; slots: objects, cells, largest, censored, sum_i, sum_j
    plane = torch.tensor([[[2, 10, 6, 1, 20, 30], [0, 0, 0, 0, 0, 0]],
                          [[4, 12, 8, 2, 36, 36], [1, 4, 4, 0, 8, 12]],
                          [[1, 10, 10, 1, 20, 70], [0, 0, 0, 0, 0, 0]]], dtype=torch.int64).view(3, 2, 1, 1, 6)
    ratio_t, ratio, bias = OB.object_count_ratio(plane)
    assert ratio_t[:, 0, 0, 0].tolist() == [2.0, 0.5] and math.isinf(ratio_t[0, 1, 0, 0].item()) and math.isnan(ratio_t[1, 1, 0, 0].item())
    assert ratio[:, 0, 0].tolist() == [2.5, 0.5] and bias[:, 0, 0].tolist() == [1.5, -0.5]
    assert OB.mean_area(plane)[:, 0, 0].tolist() == [5.0, 3.2, 10.0] and OB.censored_share(plane)[:, 0, 0].tolist() == [0.5, 0.4, 1.0]
    b, r = OB.largest_object_error(plane)
    assert b[:, 0, 0].tolist() == [3.0, 2.0]
    for got, want in zip(r[:, 0, 0].tolist(), (math.sqrt(10.0), math.sqrt(8.0))):   # torch's float64 sqrt on the CPU is within an ulp, not exact
        assert abs(got - want) <= 2.0 ** -51 * want
    move = OB.centroid_displacement(plane, (4, 5))          # diag = hypot(3, 4) = 5; centroids (2, 3), (3, 3), (2, 7)
    assert move[:, 0, 0, 0].tolist() == [0.2, 0.8] and torch.isnan(move[:, 1]).all()
    hist = torch.tensor([[4, 0, 0, 0], [0, 0, 0, 2], [1, 1, 1, 1], [0, 0, 0, 0]], dtype=torch.int64).view(4, 1, 1, 4)
    assert OB.area_pmf(hist)[2, 0, 0].tolist() == [0.25] * 4 and torch.isnan(OB.area_pmf(hist)[3]).all()
    dist = OB.area_distance(hist)[:, 0, 0]
    assert dist[:2].tolist() == [3.0, 1.5] and math.isnan(dist[2].item())
    # lists: the truth has objects at centroids (1, 1) area 4 and (5, 9) area 2; member 1 at (1, 2) area 3; member 2 has none
    obj = torch.tensor([[[0, 4, 4, 4, 0, 2, 0, 2], [50, 2, 10, 18, 5, 5, 8, 10]],
                        [[3, 3, 3, 6, 1, 1, 1, 3], [-1, 0, 0, 0, 0, 0, 0, 0]],
                        [[-1, 0, 0, 0, 0, 0, 0, 0], [-1, 0, 0, 0, 0, 0, 0, 0]]], dtype=torch.int32).view(3, 1, 1, 1, 2, 8)
    pl = torch.tensor([[2, 6, 4, 1, 14, 22], [1, 3, 3, 0, 3, 6], [0, 0, 0, 0, 0, 0]], dtype=torch.int64).view(3, 1, 1, 1, 6)
    hits, misses, fa = OB.object_matches(obj, pl, 1.0)
    assert (hits.flatten().tolist(), misses.flatten().tolist(), fa.flatten().tolist()) == ([1, 0], [1, 2], [0, 0])
    assert OB.object_csi(hits, misses, fa).flatten().tolist() == [0.5, 0.0]
    hits, misses, fa = OB.object_matches(obj, pl, 0.5)
    assert (hits.flatten().tolist(), misses.flatten().tolist(), fa.flatten().tolist()) == ([0, 0], [2, 2], [1, 0])
    hits, misses, fa = OB.object_matches(obj, pl, 1.0, min_area=3)                      # the truth's second object is filtered out
    assert (hits.flatten().tolist(), misses.flatten().tolist(), fa.flatten().tolist()) == ([1, 0], [0, 1], [0, 0])
    assert math.isnan(OB.object_csi(torch.zeros(1), torch.zeros(1), torch.zeros(1)).item())
    scatter = OB.object_scatter(obj, pl)[:, 0, 0, 0]
    c = (14 / 6, 22 / 6)
    want = (4 * math.sqrt((1 - c[0]) ** 2 + (1 - c[1]) ** 2) + 2 * math.sqrt((5 - c[0]) ** 2 + (9 - c[1]) ** 2)) / 6
    assert abs(scatter[0].item() - want) < 1e-14 and scatter[1].item() == 0.0 and math.isnan(scatter[2].item())
    loc = OB.location_error(obj, pl, (4, 5))[:, 0, 0, 0]
    assert abs(loc[0].item() - 2 * want / 5) < 1e-14 and math.isnan(loc[1].item())
    over = pl.clone()
    over[0, ..., 0] = 3                                                                  # three objects, two slots: overflowed
    assert math.isnan(OB.object_scatter(obj, over)[0, 0, 0, 0].item())
    assert OB._ordered_sum(torch.arange(5.0).view(1, 5)).tolist() == [10.0] and OB._ordered_sum(torch.zeros(2, 0)).tolist() == [0.0, 0.0]


def test_the_report(route):
    x, y, thr, above, S, Tr, th, names = _case("smooth", 3, 4, 2, 8, 12, 2)
    rep = OB.objects_report(S, Tr, th, names, 8, 16, 3.0, 2, names=["tas", "psl"])
    assert isinstance(rep, VariableReport) and rep.names == ["tas", "psl"]
    t = OB.object_tables(S, Tr, th, names, 8, 16)
    v = rep["psl"]
    assert torch.equal(v["objects"], t.plane[:, :, 1, :, 0]) and torch.equal(v["invalid"], t.invalid[:, :, 1]) and torch.equal(v["thresholds"], th[1])
    assert torch.equal(v["area_distance"], OB.area_distance(t.area_hist)[:, 1]) and v["csi"].shape == (3, 2) and v["hits"].shape == (3, 4, 2)
    flat = rep.as_dict()
    assert set(flat) == {f"objects/{n}/{k}_k{i}{s}" for n in ("tas", "psl") for k in ("count_ratio", "area_distance", "largest_bias", "csi")
                         for i in range(2) for s in ("", "_std")}


# ------------------------------------------------------------------------------------------------------------------ errors

def test_every_value_error():
    S, Tr, thr = torch.zeros(2, 3, 2, 4, 8), torch.zeros(3, 2, 4, 8), torch.zeros(2, 1)
    with pytest.raises(ValueError, match=r"must be \(M >= 1,\) \+ truth"):
        OB.object_tables(S, Tr[:2], thr)
    with pytest.raises(ValueError, match="must be floating point"):
        OB.object_tables(S.long(), Tr.long(), thr)
    with pytest.raises(ValueError, match=r"must be floating point \(M >= 1, T, F, H, W\)"):
        OB.object_tables(Tr, None, thr)
    with pytest.raises(ValueError, match="connectivity 6 must be 4 or 8"):
        OB.object_tables(S, Tr, thr, connectivity=6)
    with pytest.raises(ValueError, match="max_objects -1 must be an integer >= 0"):
        OB.object_tables(S, Tr, thr, max_objects=-1)
    with pytest.raises(ValueError, match=r"thresholds \(3, 1\) must be \(F, K\) = \(2, K >= 1\)"):
        OB.object_tables(S, Tr, torch.zeros(3, 1))
    with pytest.raises(ValueError, match="must be 'above' or 'below'"):
        OB.object_tables(S, Tr, thr, "over")
    with pytest.raises(ValueError, match=r"area_hist \(3, 2, 1, 5\) .* must be contiguous int64 \(D, F, K, B\) = \(3, 2, 1, 6\)"):
        OB.object_tables(S, Tr, thr, area_hist=torch.zeros(3, 2, 1, 5, dtype=torch.int64))
    with pytest.raises(ValueError, match="must be contiguous int64"):
        OB.object_tables(S, Tr, thr, area_hist=torch.zeros(3, 2, 1, 6, dtype=torch.int32))
    a, b = OB.object_tables(S, Tr, thr), OB.object_tables(S, None, thr)
    with pytest.raises(ValueError, match="cannot take those of"):
        a.merge(b)
    with pytest.raises(ValueError, match="cannot take those of"):
        a.merge(OB.object_tables(S, Tr, thr, max_objects=3))
    for fn in (OB.object_count_ratio, OB.largest_object_error):
        with pytest.raises(ValueError, match=r"must be \(\.\.\., D >= 2, T, F, K, 6\), row 0 the truth"):
            fn(torch.zeros(1, 2, 2, 1, 6))
    for fn in (OB.mean_area, OB.censored_share):
        with pytest.raises(ValueError, match=r"must be \(\.\.\., D, T, F, K, 6\)"):
            fn(torch.zeros(2, 2, 1, 5))
    with pytest.raises(ValueError, match=r"must be \(\.\.\., D >= 2, F, K, B\), row 0 the truth"):
        OB.area_distance(torch.zeros(1, 2, 2, 4))
    with pytest.raises(ValueError, match=r"must be \(\.\.\., B\)"):
        OB.area_pmf(torch.zeros(()))
    with pytest.raises(ValueError, match=r"shape \(4,\) must be \(H, W\)"):
        OB.centroid_displacement(a.plane, (4,))
    with pytest.raises(ValueError, match=r"must be \(\.\.\., D, T, F, K, max_objects, 8\) next to plane"):
        OB.object_scatter(a.objects, a.plane[:, :2])
    with pytest.raises(ValueError, match="row 0 the truth"):
        OB.location_error(a.objects[:1], a.plane[:1], (4, 8))
    with pytest.raises(ValueError, match="max_distance -1.0 must be >= 0"):
        OB.object_matches(a.objects, a.plane, -1.0)
    with pytest.raises(ValueError, match="min_area -2 must be an integer >= 0"):
        OB.object_matches(a.objects, a.plane, 1.0, -2)
    with pytest.raises(ValueError, match="must have one shape"):
        OB.object_csi(torch.zeros(2), torch.zeros(2), torch.zeros(3))
    with pytest.raises(ValueError, match="1 names for 2 variables"):
        OB.objects_report(S, Tr, thr, names=["a"])
    with pytest.raises(ValueError, match=r"\(L, F, H, W\)"):
        OB.objects_report(S, Tr[:2], thr)


def test_the_launcher_declines_what_the_kernel_does_not_take(monkeypatch):
    """W = 6, H W over 16384, K = 9, max_objects = 257: *_supported says no before a launcher is reached, the launcher itself answers
    False and writes nothing, and the general route gives the reference's integers"""
    emu_object_ops.install(monkeypatch, object_ops, OB)
    for H, W, K, cap in ((2, 6, 2, 4), (2, 8, 9, 4), (2, 8, 2, 257)):
        x, y, thr, above, S, Tr, th, names = _case("random59", 2, 2, 1, H, W, K)
        _assert_equal_ref(OB.object_tables(S, Tr, th, names, 8, cap), R.objects_ref(x, y, thr, above, H, W, 8, cap), (H, W, K, cap))
        assert emu_object_ops.CALLS == [] and not emu_object_ops.supported(H, W, K, 8, cap)
        D, B = 3, R.n_bins(H * W)
        plane, hist, invalid = (torch.full(s, -7, dtype=torch.int64) for s in ((D, 2, 1, K, 6), (D, 1, K, B), (D, 2, 1)))
        objs = torch.full((D, 2, 1, K, cap, 8), -7, dtype=torch.int32)
        assert emu_object_ops.object_tables(torch.tensor(x), torch.tensor(y), th, torch.tensor(above.astype(np.int32)), plane, hist, objs, invalid, 2, 2, 1, H, W, K,
                                            8, cap) is False
        assert all(bool((t == -7).all()) for t in (plane, hist, objs, invalid))
        del emu_object_ops.CALLS[:]
    assert emu_object_ops.supported(1, 4, 1, 8, 0) and emu_object_ops.supported(128, 128, 8, 4, 256) and not emu_object_ops.supported(132, 128, 1, 8, 4)
    assert not emu_object_ops.supported(4, 8, 1, 6, 4) and not emu_object_ops.supported(4, 8, 0, 8, 4) and not emu_object_ops.supported(0, 8, 1, 8, 4)
    assert not emu_object_ops.supported(4, 8, 1, 8, -1)


def test_the_emulation_restates_the_constants_of_the_kernel():
    core = open(os.path.join(CSRC, "objects_maps.h")).read()
    for text in ("THREADS = 512", "MAX_CELLS = 16384, MAX_K = 8, MAX_OBJECTS = 256, MAX_BINS = 15", "LDS_BYTES <= 80 * 1024",
                 "H >= 1 && W >= 4 && W % 4 == 0 && (long long)H * W <= MAX_CELLS && K >= 1 && K <= MAX_K && (connectivity == 4 || connectivity == 8) &&"):
        assert text in core, text
    assert (emu_object_ops.MAX_CELLS, emu_object_ops.MAX_K, emu_object_ops.MAX_OBJECTS) == (16384, 8, 256) and R.n_bins(16384) == 15
    assert OB.n_bins(128, 128) == 15 and OB.n_bins(1, 4) == 3 and OB.n_bins(1, 1) == 1


# ------------------------------------------------------------------------------------------------------------------ refusals

BAD_ARG, BAD_SHAPE, UNSUPPORTED = -1, -2, -3
POINTERS = ("x", "y", "thr", "dir", "plane", "area_hist", "objects", "invalid")
BASE = dict(x=1, y=1, thr=1, dir=1, plane=1, area_hist=1, objects=1, invalid=1, M=2, T=2, F=2, H=4, W=8, K=2, connectivity=8, max_objects=4, stream=None)
M20 = 1 << 20


def _refusal_rows():
    """(what is broken, the change, the code the documented order gives it): unsupported, then bad argument, then bad shape
    (include/c2w_hip.h).  A required pointer null or a pointer moved off its alignment class -- 16 bytes for the fields, 8 for the
    int64 tables, 4 for the rest -- is a bad argument; a grid over what a launch takes is a bad shape; an unsupported shape wins over
    both.  Derived from the declaration's comment, not recorded from the launcher."""
    rows = [(f"{n} null", {n: None}, BAD_ARG) for n in POINTERS if n != "y"]                       # y may be null: no truth
    rows += [(f"{n} off by 4", {n: 4}, BAD_ARG) for n in ("x", "y", "plane", "area_hist", "invalid")]
    rows += [(f"{n} off by 2", {n: 2}, BAD_ARG) for n in ("thr", "dir", "objects")]
    rows += [("F = 0", dict(F=0), BAD_ARG), ("T < 0", dict(T=-1), BAD_ARG)]
    rows += [("grid", dict(T=M20, F=M20), BAD_SHAPE)]
    rows += [("W no multiple of 4", dict(W=6), UNSUPPORTED), ("over 16384 cells", dict(H=132, W=128), UNSUPPORTED), ("K = 9", dict(K=9), UNSUPPORTED),
             ("connectivity 6", dict(connectivity=6), UNSUPPORTED), ("max_objects 257", dict(max_objects=257), UNSUPPORTED), ("M = 0", dict(M=0), UNSUPPORTED),
             ("unsupported and a null pointer", dict(W=6, x=None), UNSUPPORTED), ("unsupported and a grid", dict(K=0, T=M20, F=M20), UNSUPPORTED),
             ("a null pointer and a grid", dict(plane=None, T=M20, F=M20), BAD_ARG)]
    return rows


def _arguments(change):
    out = []
    for i, (arg, value) in enumerate(BASE.items()):
        address = 4096 * (16 + i)  # a made-up device address
        if arg in change:
            c = change[arg]
            value = address + c if arg in POINTERS and isinstance(c, int) else c
        elif arg in POINTERS:
            value = address
        out.append(value)
    return out


def test_object_tables_refuses_in_the_documented_order():
    """made-up addresses that nothing dereferences: every row returns before any launch.  Skipped where a GPU is visible: no row may
    ever be in a position to launch."""
    assert len(BASE) == len(_lib._PROTOS["c2w_object_tables"])
    if torch.cuda.is_available():
        pytest.skip("made-up device addresses: only where nothing can launch")
    build.build(verbose=False)
    lib = _lib.load()
    wrong = []
    for what, change, code in _refusal_rows():
        assert change and code < 0
        rc = lib.c2w_object_tables(*_arguments(change))
        if rc != code:
            wrong.append((what, rc, code))
    assert not wrong, wrong
    assert lib.c2w_objects_supported(128, 128, 8, 4, 256) == 1 and lib.c2w_objects_supported(132, 128, 8, 4, 256) == 0
    assert lib.c2w_objects_supported(4, 6, 1, 8, 0) == 0 and lib.c2w_objects_supported(1, 4, 1, 8, 0) == 1


# ------------------------------------------------------------------------------------------------------------------ the host program

@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_objects(request, tmp_path_factory):
    """a stand-alone program, once plain and once under the address and undefined-behaviour sanitizers; it is run directly, never loaded
    into Python"""
    return host_program.build(tmp_path_factory, "objects", sanitize=request.param == "sanitized", timeout=600)


@pytest.mark.parametrize("H,W,connectivity,cap", [(1, 4, 8, 4), (4, 4, 4, 0), (5, 12, 8, 1), (64, 4, 4, 64), (33, 68, 8, 256), (33, 68, 4, 3),
                                                  (128, 128, 8, 64), (128, 128, 4, 256)])
def test_the_host_program_equals_its_flood_fill(host_objects, H, W, connectivity, cap):
    """csrc/objects_maps.h compiled for the host, every adversarial kind: the maps, the runs in the bit mask, the link and flatten
    arithmetic in either thread order, the ranks, the list, the bins; every cell of a plane staged once"""
    rc = subprocess.run([str(host_objects), "check"] + [str(a) for a in (H, W, connectivity, cap)], timeout=600).returncode
    assert rc == 0, f"check {rc} of host_objects_main.cpp failed"


# ------------------------------------------------------------------------------------------------------------------ the header, the C ABI

def test_the_maps_header_compiles_as_the_first_include_on_either_side(tmp_path):
    """what tests/test_core_side_cpu.py asks of every *_core.h, of csrc/objects_maps.h"""
    unit = tmp_path / "unit.cpp"
    unit.write_text('#include "objects_maps.h"\n')
    subprocess.run(host_program.cxx() + ["-std=c++17", "-fsyntax-only", "-I" + CSRC, str(unit)], check=True, timeout=300)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "--cuda-device-only", "-fsyntax-only", "-std=c++17", "-I" + CSRC, str(unit)],
                   check=True, timeout=300)


def test_the_object_files_define_no_side_by_hand():
    private = re.compile(r"\b(OB|OBJ|OBJECTS)_(HD|BOTH|HOST)\b")
    defines = re.compile(r"#define C2W_(HD|BOTH|CORE_HOST)")
    for path in (os.path.join(CSRC, "objects_maps.h"), os.path.join(CSRC, "objects.hip"), os.path.join(ROOT, "tests", "host_objects_main.cpp")):
        text = open(path).read()
        assert not private.search(text) and not defines.search(text), path
    assert '#include "core_side.h"' in open(os.path.join(CSRC, "objects_maps.h")).read()


def test_new_entry_points_have_matching_argument_lists():
    names = {"c2w_objects_supported": "int", "c2w_object_tables": "int"}
    c_abi.assert_declared(names, "objects.hip", object_ops, ("supported", "object_tables"))
