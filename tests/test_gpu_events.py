"""The event-verification kernels on the MI355X (csrc/events.hip through event_ops and climate2weather_amd.events): both integer
tables EQUAL to the NumPy reference of tests/fp64_events_ref.py at the smallest shapes that can go wrong -- the tables are integers, so
no test here carries a tolerance -- then the properties the interface promises: the same integers wherever a plane lies in the launch
and on a second call, nothing written past the end, nothing written for an unsupported shape, a NaN kept in its own plane's entries,
the same table on another stream, a strided fp16 input equal to the dense route, and every public function on the device equal to the
general route."""
import numpy as np
import pytest
import torch

import fp64_events_ref as R
from climate2weather_amd import event_ops
from climate2weather_amd import events as EV

pytestmark = pytest.mark.gpu

CANARY = -7
TAIL = 64  # canary values behind each output


def dev():
    return torch.device("cuda:0")


def to_dev(*arrays):
    return [torch.tensor(np.asarray(a)).to(dev()) for a in arrays]


def _canaried(n):
    return torch.full((n + TAIL,), CANARY, dtype=torch.int64, device=dev())


def _kept(buf, n):
    return torch.equal(buf[n:], torch.full_like(buf[n:], CANARY))


def counts(x, y, thr, above, expect=True):
    """(counts (T, F, K, 2, M + 1), invalid (T, F)) from event_ops.event_counts on x (M, T, F, hw), y (T, F, hw); the TAIL values behind
    both outputs must keep the canary.  expect False: the call must answer False and leave every value of both alone."""
    M, T, F, hw = x.shape
    K = thr.shape[1]
    xd, yd, td, dd = to_dev(x, y, thr, above.astype(np.int32))
    n, ni = T * F * K * 2 * (M + 1), T * F
    c, inv = _canaried(n), _canaried(ni)
    ok = event_ops.event_counts(xd, yd, td, dd, c, inv, M, T, F, hw, K)
    assert ok is expect
    assert _kept(c, n if expect else 0) and _kept(inv, ni if expect else 0)
    return c[:n].view(T, F, K, 2, M + 1), inv[:ni].view(T, F)


def fss(x, y, thr, above, radii, H, W_, expect=True):
    """sums (T, F, K, S, M + 2, 2) from event_ops.fss_sums, canaries as above"""
    M, T, F, hw = x.shape
    K, S = thr.shape[1], len(radii)
    xd, yd, td, dd = to_dev(x, y, thr, above.astype(np.int32))
    n = T * F * K * S * (M + 2) * 2
    s = _canaried(n)
    ok = event_ops.fss_sums(xd, yd, td, dd, s, list(radii), M, T, F, H, W_, K)
    assert ok is expect
    assert _kept(s, n if expect else 0)
    return s[:n].view(T, F, K, S, M + 2, 2)


# ------------------------------------------------------------------------------------------------------------------ against the reference

@pytest.mark.parametrize("hw", [4, 4096, 4100, 16384])
def test_the_joint_table_equals_the_reference(hw):
    """M in {1, 2, 8, 9, 33, 64}, K in {1, 3, 8}, both directions, every combination; the field kinds take turns, so every kind meets
    every shape.  Variable f differs from its neighbours in offset and scale, so a wrong index map fails."""
    T, F, i = (2, 2, 0) if hw <= 4096 else (1, 2, 0)
    for M in (1, 2, 8, 9, 33, 64):
        for K in (1, 3, 8):
            kind = R.KINDS[i % len(R.KINDS)]
            i += 1
            x, y = R.fields(kind, M, T, F, hw)
            thr = R.thresholds(kind, y, K)
            for direction in ("above", "below"):
                above = R.directions(F, K, direction)
                got, inv = counts(x, y, thr, above)
                want, winv = R.counts_ref(x, y, thr, above)
                assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(inv.cpu().numpy(), winv), (kind, M, K, direction)


EIGHT = (0, 1, 2, 3, 5, 8, 13, 16)


@pytest.mark.parametrize("H,W_", [(4, 4), (8, 12), (64, 64), (68, 72), (40, 132), (128, 128)])
def test_the_fss_sums_equal_the_reference(H, W_):
    """planes whose every window is clipped on all sides, exactly one tile, remainder tiles of width 4 and 8, three tiles across, four
    tiles; radii (0,), (0, 1, 2, 16) and eight radii; M in {1, 9, 64}; every combination, mixed directions, the kinds taking turns"""
    T, F, K, i = 1, 2, 2, 0
    for M in (1, 9, 64):
        for radii in ((0,), (0, 1, 2, 16), EIGHT):
            kind = R.KINDS[i % len(R.KINDS)]
            i += 1
            x, y = R.fields(kind, M, T, F, H * W_)
            thr, above = R.thresholds(kind, y, K), R.directions(F, K, "mixed")
            got = fss(x, y, thr, above, radii, H, W_)
            assert np.array_equal(got.cpu().numpy(), R.fss_ref(x, y, thr, above, radii, H, W_)), (kind, M, radii)


# ------------------------------------------------------------------------------------------------------------------ the promises

@pytest.mark.parametrize("H,W_", [(8, 8), (41, 100), (68, 72)])
def test_the_same_plane_gives_the_same_integers_at_every_position(H, W_):
    """one plane series in the first and in the last variable, at the first and at the last time, alone, and on a second call"""
    M, T, F, K, radii = 3, 4, 3, 2, (0, 2, 16)
    hw = H * W_
    x, y = R.fields("temperature", M, T, F, hw)
    x, y = x.copy(), y.copy()
    px, py = x[:, 1, 1].copy(), y[1, 1].copy()
    for t, f in ((0, 0), (3, 2)):
        x[:, t, f], y[t, f] = px, py
    thr = np.repeat(R.thresholds("temperature", y[:, 1:2], K), F, axis=0)  # the same thresholds for every variable
    above = R.directions(F, K, "above")
    a, b = counts(x, y, thr, above), counts(x, y, thr, above)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    alone = counts(px[:, None, None], py[None, None], thr[:1], above[:1])[0][0, 0]
    for t, f in ((1, 1), (0, 0), (3, 2)):
        assert torch.equal(a[0][t, f], alone), (t, f)
    assert not torch.equal(a[0][2, 1], alone)
    if W_ % 4 == 0:
        s, s2 = fss(x, y, thr, above, radii, H, W_), fss(x, y, thr, above, radii, H, W_)
        assert torch.equal(s, s2)
        alone = fss(px[:, None, None], py[None, None], thr[:1], above[:1], radii, H, W_)[0, 0]
        for t, f in ((1, 1), (0, 0), (3, 2)):
            assert torch.equal(s[t, f], alone), (t, f)
        assert not torch.equal(s[2, 1], alone)


def test_a_nan_touches_only_its_own_planes_entries():
    M, T, F, K, H, W_, radii = 3, 3, 2, 2, 41, 100, (0, 3)
    x, y = R.fields("wind", M, T, F, H * W_)
    thr, above = R.thresholds("wind", y, K), R.directions(F, K, "above")
    clean, none = counts(x, y, thr, above)
    clean_s = fss(x, y, thr, above, radii, H, W_)
    x, y = x.copy(), y.copy()
    x[1, 2, 0, 4099] = np.nan   # the last cell: the second chunk
    y[0, 1, 0] = np.nan
    x[2, 0, 1, 0] = np.nan      # the same cell as the truth's: one invalid cell
    got, inv = counts(x, y, thr, above)
    s = fss(x, y, thr, above, radii, H, W_)
    touched = torch.zeros(T, F, dtype=torch.bool, device=dev())
    touched[2, 0] = touched[0, 1] = True
    assert int(none.sum()) == 0 and torch.equal(inv, touched.long())
    assert torch.equal(got[~touched], clean[~touched]) and torch.equal(s[~touched], clean_s[~touched])
    assert torch.equal(got.sum(dim=(-1, -2)), (H * W_ - inv)[:, :, None].expand(T, F, K))
    assert np.array_equal(got.cpu().numpy(), R.counts_ref(x, y, thr, above)[0])
    assert np.array_equal(s.cpu().numpy(), R.fss_ref(x, y, thr, above, radii, H, W_))  # a NaN is no event in its own row


def test_unsupported_shapes_write_nothing_and_take_the_general_route():
    assert not event_ops.counts_supported(6, 2, 2) and not event_ops.counts_supported(64, 65, 2) and not event_ops.counts_supported(64, 2, 9)
    assert event_ops.counts_supported(4, 1, 1) and event_ops.counts_supported(16384, 64, 8)
    assert not event_ops.fss_supported(8, 6, 2, 2, (0,)) and not event_ops.fss_supported(2, 8, 2, 2, (0,)) and not event_ops.fss_supported(8, 8, 2, 2, (17,))
    assert not event_ops.fss_supported(8, 8, 2, 2, tuple(range(9))) and not event_ops.fss_supported(1024, 1028, 2, 2, (0,))
    assert event_ops.fss_supported(4, 4, 1, 1, (0,)) and event_ops.fss_supported(1024, 1024, 64, 8, EIGHT)
    x, y = R.fields("temperature", 2, 2, 2, 18)
    thr, above = R.thresholds("temperature", y, 2), R.directions(2, 2, "mixed")
    counts(x, y, thr, above, expect=False)                 # hw = 18
    fss(x, y, thr, above, (0, 1), 3, 6, expect=False)      # W = 6
    x9, y9 = R.fields("temperature", 2, 2, 2, 64)
    thr9 = R.thresholds("temperature", y9, 9)
    counts(x9, y9, thr9, R.directions(2, 9, "above"), expect=False)   # K = 9
    fss(x9, y9, thr9[:, :2], above, (0, 17), 8, 8, expect=False)      # a radius of 17
    S, Tr, th = to_dev(x.reshape(2, 2, 2, 3, 6), y.reshape(2, 2, 3, 6), thr)
    names = R.direction_names(above)
    got, inv = EV.event_counts(S, Tr, th, names)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), R.counts_ref(x, y, thr, above)[0]) and int(inv.sum()) == 0
    s = EV.fss_sums(S, Tr, th, (0, 1, 40), names)
    assert s.is_cuda and np.array_equal(s.cpu().numpy(), R.fss_ref(x, y, thr, above, (0, 1, 40), 3, 6))


def test_a_call_on_another_stream_gives_the_same_tables():
    x, y = R.fields("pressure", 3, 3, 2, 68 * 72)
    thr = R.thresholds("pressure", y, 2)
    S, Tr, th = to_dev(x.reshape(3, 3, 2, 68, 72), y.reshape(3, 2, 68, 72), thr)
    want_c, want_s = EV.event_counts(S, Tr, th), EV.fss_sums(S, Tr, th, (0, 2, 16))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got_c, got_s = EV.event_counts(S, Tr, th), EV.fss_sums(S, Tr, th, (0, 2, 16))
    side.synchronize()
    assert torch.equal(got_c[0], want_c[0]) and torch.equal(got_c[1], want_c[1]) and torch.equal(got_s, want_s)


def test_strided_half_precision_input_agrees_with_the_dense_route():
    base = (torch.randn(3, 4, 2, 16, 64, device=dev()) * 3.0 + 1.0).to(torch.float16)
    view, truth = base[..., ::2], base[0, ..., 1::2]
    dense, dtruth = view.float().contiguous(), truth.float().contiguous()
    thr = torch.tensor([[0.5, 4.0], [1.0, -2.0]], dtype=torch.float64)
    a, b = EV.event_counts(view, truth, thr, ["above", "below"]), EV.event_counts(dense, dtruth, thr.float().to(dev()), ["above", "below"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and int(a[0].sum()) == 4 * 2 * 2 * 16 * 32
    assert torch.equal(EV.fss_sums(view, truth, thr, (0, 1, 4)), EV.fss_sums(dense, dtruth, thr.float().to(dev()), (0, 1, 4)))


# ------------------------------------------------------------------------------------------------------------------ the public functions

def test_public_functions_on_the_device_equal_the_general_route(monkeypatch):
    """(M, T, F) = (5, 4, 2) at 40 x 52, wind and pressure, a NaN included: every public function through the kernels against the same
    function through the general torch route on the same device -- equal, since the tables are the same integers and the algebra is
    the same float64 code"""
    M, T, F, H, W_, radii = 5, 4, 2, 40, 52, (0, 1, 2, 4, 8)
    xw, yw = R.fields("wind", M, T, 1, H * W_)
    xp, yp = R.fields("pressure", M, T, 1, H * W_)
    x, y = np.concatenate([xw, xp], axis=2), np.concatenate([yw, yp], axis=1)
    x[2, 1, 0, 77] = np.nan
    S, Tr = to_dev(x.reshape(M, T, F, H, W_), y.reshape(T, F, H, W_))

    def everything():
        thr = EV.thresholds_from_quantiles(Tr, (0.9, 0.99))
        c, inv = EV.event_counts(S, Tr, thr)
        s = EV.fss_sums(S, Tr, thr, radii)
        C = c.sum(dim=0)
        out = [thr, c, inv, s, EV.brier_score(c), EV.brier_score(C, fair=True), *EV.brier_decomposition(C), EV.brier_skill_score(C),
               *EV.reliability_curve(C), *EV.roc_curve(C), EV.roc_area(C), *EV.fss(s), *EV.fss(s, pooled=True), EV.fss_useful_scale(s, radii, H * W_),
               *EV.member_contingency(s, radii, H * W_).values()]
        rep = EV.events_report(S, Tr, levels=(0.9, 0.99), radii=radii, names=["sfcWind", "psl"])
        for _, v in rep:
            out += [v[k] for k in sorted(v)]
        return out, rep.as_dict()

    kernel, kernel_flat = everything()
    monkeypatch.setattr(EV, "_on_device", lambda t: False)
    general, general_flat = everything()
    assert len(kernel) == len(general) and all(t.is_cuda for t in kernel)
    for i, (a, b) in enumerate(zip(kernel, general)):
        assert a.dtype == b.dtype and a.shape == b.shape, i
        assert torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0)) if a.is_floating_point() else torch.equal(a, b), i
        if a.is_floating_point():
            assert torch.equal(torch.isnan(a), torch.isnan(b)), i
    assert kernel_flat == general_flat and int(kernel[2].sum()) == 1
