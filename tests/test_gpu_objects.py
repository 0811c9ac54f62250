"""The event-object kernel on the MI355X (csrc/objects.hip through object_ops and climate2weather_amd.objects): all four tables EQUAL
to the flood fill of tests/fp64_objects_ref.py at the smallest shapes that can go wrong -- everything is integers, so no test here
carries a tolerance -- then the properties the interface promises: nothing written past the end, nothing written for unsupported
arguments, the same integers wherever a plane lies in the launch and on a second call, a NaN or an infinity kept to its own plane, the
same tables on another stream, a strided fp16 input equal to the dense route, every public function on the device equal to the
general route on CPU copies, and the known answers."""
import numpy as np
import pytest
import torch

import fp64_objects_ref as R
from climate2weather_amd import object_ops
from climate2weather_amd import objects as OB

pytestmark = pytest.mark.gpu

CANARY = -7
TAIL = 64  # canary values behind each output
NAMES = ("plane", "area_hist", "objects", "invalid")


def dev():
    return torch.device("cuda:0")


def to_dev(*arrays):
    return [torch.tensor(np.asarray(a)).to(dev()) for a in arrays]


def tables(x, y, thr, above, H, W, conn, cap, expect=True):
    """One object_ops.object_tables on x (M, T, F, H W), y (T, F, H W) or None: (plane, area_hist, objects, invalid) as int64 arrays.
    The written tables start as canaries, so an entry the call leaves out shows; the accumulator starts at zero; the TAIL values
    behind all four must keep the canary.  expect False: the call must answer False and leave every value alone."""
    M, T, F, hw = x.shape
    K, D = thr.shape[1], M + (0 if y is None else 1)
    xd, td, dd = to_dev(x, thr, above.astype(np.int32))
    yd = None if y is None else to_dev(y)[0]
    sizes = (D * T * F * K * 6, D * F * K * R.n_bins(hw), D * T * F * K * cap * 8, D * T * F)
    bufs = [torch.full((n + TAIL,), CANARY, dtype=torch.int32 if i == 2 else torch.int64, device=dev()) for i, n in enumerate(sizes)]
    if expect:
        bufs[1][:sizes[1]] = 0
    ok = object_ops.object_tables(xd, yd, td, dd, bufs[0], bufs[1], bufs[2] if cap else None, bufs[3], M, T, F, H, W, K, conn, cap)
    assert ok is expect
    for buf, n in zip(bufs, sizes):
        assert torch.equal(buf[n if expect else 0:], torch.full_like(buf[n if expect else 0:], CANARY))
    shapes = ((D, T, F, K, 6), (D, F, K, R.n_bins(hw)), (D, T, F, K, cap, 8), (D, T, F))
    return [buf[:n].view(s).cpu().numpy().astype(np.int64) for buf, n, s in zip(bufs, sizes, shapes)]


def assert_ref(got, want, what=""):
    for g, name in zip(got, NAMES):
        assert np.array_equal(g, want[name]), (name, what)


def assert_tables(t, want, what=""):
    for name in NAMES:
        assert np.array_equal(getattr(t, name).cpu().numpy(), want[name]), (name, what)


def same_tables(a, b, what=""):
    assert a.n_times == b.n_times and a.shape == b.shape
    for name in NAMES:
        assert torch.equal(getattr(a, name).cpu(), getattr(b, name).cpu()), (name, what)


# ------------------------------------------------------------------------------------------------------------------ against the reference

SHAPES = [(1, 4), (4, 4), (5, 12), (64, 4), (33, 68)]
KS, CAPS = (1, 3, 8), (0, 1, 64, 256)


@pytest.mark.parametrize("H,W", SHAPES)
def test_the_tables_equal_the_reference(H, W):
    """one thread's worth, the smallest square, W no power of two with an odd H, a tall plane of many row links, remainder threads.
    Sixteen deals a shape, one per kind; M in {1, 3} with and without a truth, K in {1, 3, 8}, both connectivities, mixed directions
    and max_objects in {0, 1, 64, 256} take turns, and the pairings shift with the shape.  Variable f differs from its neighbours in
    offset and scale, so a wrong index map fails."""
    s = SHAPES.index((H, W))
    for i, kind in enumerate(R.KINDS):
        M, with_truth, K = (1, 3)[(i + s) % 2], ((i + s) // 2) % 2 == 0, KS[(i + s) % 3]
        conn, cap, T, F = (4, 8)[(i // 2 + s) % 2], CAPS[(i + i // 4 + s) % 4], 1 + i % 2, 2
        x, y = R.fields(kind, M, T, F, H, W)
        thr, above = R.thresholds(kind, F, K), R.directions(F, K, ("mixed", "above", "below")[(i + s) % 3])
        y = y if with_truth else None
        assert_ref(tables(x, y, thr, above, H, W, conn, cap), R.objects_ref(x, y, thr, above, H, W, conn, cap), (kind, M, with_truth, K, conn, cap, T))


@pytest.mark.parametrize("conn", [4, 8])
def test_the_largest_plane_equals_the_reference(conn):
    """128 x 128, the limit: one object whose label travels the whole plane (spiral, serpentine), 8192 objects or one (checker), one
    object of 16384 cells (full: the area that needs 15 bits) and the percolation threshold, where objects of every size merge"""
    for kind in R.LARGE_KINDS:
        x, y = R.fields(kind, 1, 1, 1, 128, 128)
        thr, above = R.thresholds(kind, 1, 1), R.directions(1, 1, "above")
        got = tables(x, None, thr, above, 128, 128, conn, 256)
        assert_ref(got, R.objects_ref(x, None, thr, above, 128, 128, conn, 256), kind)
    # random59 at connectivity 4 is below the threshold: the list overflowed and the plane's row still counts every object; at 8 it
    # is far above it and nearly everything is one object
    assert (got[0][0, 0, 0, 0, 0] > 256) == (conn == 4)


def test_a_plane_over_the_limit_is_refused_and_the_general_route_serves_it():
    H, W = 132, 128
    assert not object_ops.supported(H, W, 1, 8, 64) and object_ops.supported(128, 128, 8, 4, 256) and object_ops.supported(1, 4, 1, 8, 0)
    x, y = R.fields("random59", 1, 1, 1, H, W)
    thr, above = R.thresholds("random59", 1, 1), R.directions(1, 1, "above")
    tables(x, y, thr, above, H, W, 8, 64, expect=False)
    S, Tr, th = to_dev(x.reshape(1, 1, 1, H, W), y.reshape(1, 1, H, W), thr)
    t = OB.object_tables(S, Tr, th, "above", 8, 64)
    assert t.plane.is_cuda
    assert_tables(t, R.objects_ref(x, y, thr, above, H, W, 8, 64))


def test_unsupported_arguments_write_nothing_and_take_the_general_route():
    for H, W, K, conn, cap in ((4, 6, 2, 8, 4), (4, 8, 9, 8, 4), (4, 8, 2, 8, 257)):
        assert not object_ops.supported(H, W, K, conn, cap)
        x, y = R.fields("random59", 2, 2, 1, H, W)
        thr, above = R.thresholds("random59", 1, K), R.directions(1, K, "mixed")
        tables(x, y, thr, above, H, W, conn, cap, expect=False)
        S, Tr, th = to_dev(x.reshape(2, 2, 1, H, W), y.reshape(2, 1, H, W), thr)
        t = OB.object_tables(S, Tr, th, R.direction_names(above), conn, cap)
        assert t.plane.is_cuda
        assert_tables(t, R.objects_ref(x, y, thr, above, H, W, conn, cap), (H, W, K, conn, cap))
    assert not object_ops.supported(4, 8, 2, 6, 4) and not object_ops.supported(4, 8, 0, 8, 4) and not object_ops.supported(4, 8, 2, 8, -1)
    x, y = R.fields("random59", 2, 2, 1, 4, 8)
    tables(x, y, R.thresholds("random59", 1, 2), R.directions(1, 2, "mixed"), 4, 8, 6, 4, expect=False)


# ------------------------------------------------------------------------------------------------------------------ the promises

def test_the_same_plane_gives_the_same_integers_at_every_position_and_on_a_second_call():
    """one plane placed as the truth, as the last member at the last time in the last variable, and alone"""
    M, T, F, H, W, K = 3, 3, 3, 33, 68, 3
    x, y = R.fields("random59", M, T, F, H, W)
    x, y = x.copy(), y.copy()
    p = x[1, 1, 1].copy()
    y[0, 0], x[2, 2, 2] = p, p
    thr = np.repeat(R.thresholds("random59", F, K)[1:2], F, axis=0)          # the same thresholds for every variable
    above = R.directions(F, K, "above")
    a, b = tables(x, y, thr, above, H, W, 8, 64), tables(x, y, thr, above, H, W, 8, 64)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    alone = tables(p[None, None, None], None, thr[:1], above[:1], H, W, 8, 64)
    for d, t, f in ((2, 1, 1), (0, 0, 0), (3, 2, 2)):
        assert np.array_equal(a[0][d, t, f], alone[0][0, 0, 0]) and np.array_equal(a[2][d, t, f], alone[2][0, 0, 0]), (d, t, f)
    assert not np.array_equal(a[0][1, 0, 0], alone[0][0, 0, 0])


def test_a_nan_or_an_infinity_stays_in_its_own_plane():
    M, T, F, H, W, K = 2, 2, 2, 33, 68, 2
    x, y = R.fields("smooth", M, T, F, H, W)
    thr, above = R.thresholds("smooth", F, K), R.directions(F, K, "mixed")
    clean = tables(x, y, thr, above, H, W, 8, 64)
    x, y = x.copy(), y.copy()
    x[1, 1, 0, H * W - 1] = np.nan
    y[0, 1, 0] = np.inf
    x[0, 1, 1, 513] = -np.inf
    got = tables(x, y, thr, above, H, W, 8, 64)
    keep = np.ones((M + 1, T, F), bool)
    keep[2, 1, 0] = keep[0, 0, 1] = keep[1, 1, 1] = False
    assert np.array_equal(got[0][keep], clean[0][keep]) and np.array_equal(got[2][keep], clean[2][keep]) and int(clean[3].sum()) == 0
    assert int(got[3].sum()) == 1 and got[3][2, 1, 0] == 1
    assert_ref(got, R.objects_ref(x, y, thr, above, H, W, 8, 64))


def test_a_call_on_another_stream_gives_the_same_tables():
    x, y = R.fields("smooth", 3, 4, 2, 36, 56)
    thr = R.thresholds("smooth", 2, 3)
    S, Tr, th = to_dev(x.reshape(3, 4, 2, 36, 56), y.reshape(4, 2, 36, 56), thr)
    want = OB.object_tables(S, Tr, th, "below", 4, 16)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = OB.object_tables(S, Tr, th, "below", 4, 16)
    side.synchronize()
    same_tables(got, want)
    assert_tables(want, R.objects_ref(x, y, thr, R.directions(2, 3, "below"), 36, 56, 4, 16))


def test_strided_half_precision_input_agrees_with_the_dense_route():
    base = (torch.randn(3, 5, 2, 16, 64, device=dev()) * 3.0 + 1.0).to(torch.float16)
    view, truth = base[..., ::2], base[0, ..., 1::2]
    dense, dtruth = view.float().contiguous(), truth.float().contiguous()
    thr = torch.tensor([[0.5, 4.0], [1.0, -2.0]], dtype=torch.float64)
    a = OB.object_tables(view, truth, thr, ["above", "below"], 8, 32)
    b = OB.object_tables(dense, dtruth, thr.float().to(dev()), ["above", "below"], 8, 32)
    same_tables(a, b)
    assert int(a.plane[..., 0].sum()) > 0 and a.n_times == 5


def test_the_accumulator_and_merge_on_the_device_equal_one_call():
    x, y = R.fields("random30", 2, 5, 2, 12, 20)
    thr = R.thresholds("random30", 2, 2)
    S, Tr, th = to_dev(x.reshape(2, 5, 2, 12, 20), y.reshape(5, 2, 12, 20), thr)
    whole = OB.object_tables(S, Tr, th, "above", 4, 8)
    first = OB.object_tables(S[:, :2], Tr[:2], th, "above", 4, 8)
    rest = OB.object_tables(S[:, 2:], Tr[2:], th, "above", 4, 8)
    same_tables(first.merge(rest), whole)
    second = OB.object_tables(S[:, 2:], Tr[2:], th, "above", 4, 8, area_hist=first.area_hist.clone())
    assert torch.equal(second.area_hist, whole.area_hist)


# ------------------------------------------------------------------------------------------------------------------ the public functions

def test_public_functions_on_the_device_equal_the_general_route_on_cpu_copies():
    """(M, T, F) = (3, 4, 2) at 40 x 52, smooth and random, a NaN included: every public function through the kernel against the same
    function through the general torch route on CPU copies -- equal, since the tables are the same integers and the algebra is the
    same float64 code, its one sum of non-integers taken in a fixed order"""
    M, T, F, H, W, K = 3, 4, 2, 40, 52, 3
    xs, ys = R.fields("smooth", M, T, 1, H, W)
    xr, yr = R.fields("random30", M, T, 1, H, W)
    x, y = np.concatenate([xs, xr], axis=2), np.concatenate([ys, yr], axis=1)
    x[2, 1, 0, 77] = np.nan
    thr = np.concatenate([R.thresholds("smooth", 1, K), R.thresholds("random30", 1, K)])
    S, Tr, th = to_dev(x.reshape(M, T, F, H, W), y.reshape(T, F, H, W), thr)
    names = ["above", "below", "above"]

    def everything(S, Tr, th):
        t = OB.object_tables(S[:, :1], Tr[:1], th, names, 8, 16).merge(OB.object_tables(S[:, 1:], Tr[1:], th, names, 8, 16))
        u = OB.object_tables(S, None, th, "above", 4, 0)
        out = [t.plane, t.area_hist, t.objects, t.invalid, u.plane, u.area_hist, u.objects, u.invalid, *OB.object_count_ratio(t.plane),
               OB.area_pmf(t.area_hist), OB.mean_area(t.plane), OB.area_distance(t.area_hist), *OB.largest_object_error(t.plane),
               OB.censored_share(t.plane), OB.centroid_displacement(t.plane, t.shape), OB.object_scatter(t.objects, t.plane),
               OB.location_error(t.objects, t.plane, t.shape)]
        match = OB.object_matches(t.objects, t.plane, 6.0, 2)
        out += [*match, OB.object_csi(*match)]
        rep = OB.objects_report(S, Tr, th, names, 8, 16, 6.0, 2, names=["tas", "psl"])
        for _, v in rep:
            out += [v[k] for k in sorted(v)]
        return out, rep.as_dict(), t.n_times

    kernel, kernel_flat, n = everything(S, Tr, th)
    general, general_flat, n2 = everything(S.cpu(), Tr.cpu(), th.cpu())
    assert len(kernel) == len(general) and all(t.is_cuda for t in kernel) and n == n2 == T
    for i, (a, b) in enumerate(zip(kernel, general)):
        a = a.cpu()
        assert a.dtype == b.dtype and a.shape == b.shape, i
        if a.is_floating_point():
            assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0)), i
        else:
            assert torch.equal(a, b), i
    assert set(kernel_flat) == set(general_flat) and int(kernel[3].sum()) == 1
    for key, v in kernel_flat.items():
        assert v == general_flat[key] or (v != v and general_flat[key] != general_flat[key]), key


def test_the_known_answers():
    H, W = 32, 64
    i, j = np.indices((H, W))
    ring = (np.maximum(np.abs(i - 10), np.abs(j - 20)) == 5)                                  # a square ring of side 11 around (10, 20)
    blocks = ((i < 16) & (j < 32)) | ((i >= 16) & (j >= 32))
    planes = np.stack([(i + j) % 2 == 0, np.ones((H, W), bool), blocks, ring, np.zeros((H, W), bool)]).astype(np.float32)
    S = torch.tensor(planes).view(1, 5, 1, H, W).to(dev())
    one = torch.tensor([[1.0]])
    for conn, n_checker, n_blocks in ((4, H * W // 2, 2), (8, 1, 1)):
        t = OB.object_tables(S, None, one, "above", conn, 4)
        p = t.plane[0, :, 0, 0].cpu()
        assert p[:, 0].tolist() == [n_checker, 1, n_blocks, 1, 0] and p[:, 1].tolist() == [H * W // 2, H * W, H * W // 2, 40, 0]
        assert p[:, 2].tolist() == [H * W // 2 if conn == 8 else 1, H * W, H * W // 2 if conn == 8 else H * W // 4, 40, 0]
        assert p[:, 3].tolist() == [2 * (H + W - 2) // 2 if conn == 4 else 1, 1, n_blocks, 0, 0]
        o = t.objects[0, :, 0, 0].cpu()
        assert o[1, 0].tolist() == [0, H * W, W * H * (H - 1) // 2, H * W * (W - 1) // 2, 0, H - 1, 0, W - 1] and o[1, 1].tolist() == [-1] + [0] * 7
        assert o[3, 0].tolist() == [5 * W + 15, 40, 400, 800, 5, 15, 15, 25] and o[4, :, 0].tolist() == [-1] * 4
        assert t.area_hist[0, 0, 0].sum().item() == p[:, 0].sum().item()
        c = OB.object_scatter(t.objects, t.plane)[0, :, 0, 0].cpu()
        assert c[3].item() == 0.0 and torch.isnan(c[4]).item() and (conn == 8 or torch.isnan(c[0]).item())
