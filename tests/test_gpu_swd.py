"""The sliced-Wasserstein kernels on the MI355X (csrc/swd.hip through ops.swd_project, ops.swd_distance and
wasserstein.sliced_wasserstein): every projection entry against float64 by the rule of tests/fp64_swd_ref.py -- an entry passes if its
error is at most four times the larger of the fp32 torch.matmul route's error on that entry and 16 * 2^-24 * sum |x^ theta| -- the
distance kernel against float64 to T * 2^-52, then the properties the interface promises: the same bits wherever a field or a column
lies in the batch, nothing written past the end, nothing written for an unsupported shape, a NaN kept in its own member and variable."""
import numpy as np
import pytest
import torch

import fp64_swd_ref as R
from climate2weather_amd import ops
from climate2weather_amd import wasserstein as W

pytestmark = pytest.mark.gpu

CANARY = -7.25
TAIL = 64  # canary values behind each output


def dev():
    return torch.device("cuda:0")


def to_dev(*arrays):
    return [torch.tensor(np.asarray(a)).to(dev()) for a in arrays]


def project(x, th, shift, scale):
    """proj (n_rep, F, P, T) fp32 from ops.swd_project on x (n_rep, T, F, d); the TAIL values behind it must keep the canary"""
    n_rep, T, F, d = x.shape
    P = th.shape[0]
    n = n_rep * F * P * T
    buf = torch.full((n + TAIL,), CANARY, dtype=torch.float32, device=x.device)
    assert ops.swd_project(x, th, shift, scale, buf, n_rep, T, F, d, P)
    assert torch.equal(buf[n:], torch.full_like(buf[n:], CANARY))
    return buf[:n].view(n_rep, F, P, T)


def distance(px, py):
    """out (n_rep, F, P) float64 from ops.swd_distance; the TAIL values behind it must keep the canary"""
    n_rep, F, P, T = px.shape
    n = n_rep * F * P
    buf = torch.full((n + TAIL,), CANARY, dtype=torch.float64, device=px.device)
    assert ops.swd_distance(px, py, buf, n_rep, F, P, T)
    assert torch.equal(buf[n:], torch.full_like(buf[n:], CANARY))
    return buf[:n].view(n_rep, F, P)


# ------------------------------------------------------------------------------------------------------------------ projection

BATCHES = [(1, 1, 1), (2, 3, 2), (3, 37, 4), (1, 130, 1)]  # none fills its tiles of 64 fields; 444 and 130 fields need 7 and 3 workgroups
CASES = [(d, P, BATCHES[(i + j) % 4]) for i, d in enumerate((64, 192, 1024, 4096)) for j, P in enumerate((1, 16, 100, 128))]
CASES += [(16384, 100, (2, 5, 2)), (65536, 100, (1, 2, 1)), (4096, 33, (3, 37, 4)), (1024, 64, (1, 130, 1)), (192, 65, (2, 3, 2))]


@pytest.mark.parametrize("d,P,batch", CASES)
def test_projection_entries_against_float64(d, P, batch):
    """every field kind, pressure-like and temperature-like with their own moments as shift and scale; variable f differs from its
    neighbours in both, so a wrong i % F fails"""
    n_rep, T, F = batch
    th = R.theta32(d, P)
    thd, = to_dev(th)
    worst = {}
    for kind in R.KINDS:
        s, _, shift, scale = R.fields(kind, n_rep, T, F, d)
        got = project(*to_dev(s), thd, *to_dev(shift, scale)).cpu().numpy().astype(np.float64)
        xh = R.xhat32(s, shift, scale)
        p64 = R.project64(xh, th)
        e, b = np.abs(np.moveaxis(got, -1, 1) - p64), R.proj_bound(xh, th, p64)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst[kind] = float(np.nanmax(np.where(b > 0, e / (b / R.FACTOR), 0)))
        assert np.all(e <= b), (kind, float(np.max(e - b)))
    print(f"d {d} P {P} (n_rep, T, F) {batch}: error over max(yardstick, floor), limit {R.FACTOR}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_projection_same_bits_at_every_position():
    """one field at rows 0, 131 and 299 of 300 (three of five workgroups, three different rows of a tile), alone, and on a second call"""
    d, P = 192, 100
    g = np.random.default_rng(1)
    x = (280.0 + 10.0 * g.standard_normal((1, 300, 1, d))).astype(np.float32)
    x[0, 131, 0] = x[0, 299, 0] = x[0, 0, 0]
    thd, shift, scale = to_dev(R.theta32(d, P), np.float32([280.0]), np.float32([0.1]))
    xd, = to_dev(x)
    a, b = project(xd, thd, shift, scale), project(xd, thd, shift, scale)
    assert torch.equal(a, b)
    alone = project(xd[:, :1].contiguous(), thd, shift, scale)  # (1, 1, P, 1)
    for t in (0, 131, 299):
        assert torch.equal(a[0, 0, :, t], alone[0, 0, :, 0]), t
    assert not torch.equal(a[0, 0, :, 1], alone[0, 0, :, 0])


def test_projection_of_samples_and_truth_in_one_launch_gives_the_bits_of_two():
    n_rep, T, F, d, P = 3, 37, 2, 192, 100  # 222 and 74 fields: both end in a partly empty tile
    s, t, shift, scale = R.fields("temperature", n_rep, T, F, d)
    sd, td, thd, shd, scd = to_dev(s, t, R.theta32(d, P), shift, scale)
    nx, ny = n_rep * F * P * T, F * P * T
    bx, by = torch.full((nx + TAIL,), CANARY, device=dev()), torch.full((ny + TAIL,), CANARY, device=dev())
    assert ops.swd_project_pair(sd, td, thd, shd, scd, bx, by, n_rep, T, F, d, P)
    assert torch.equal(bx[nx:], torch.full_like(bx[nx:], CANARY)) and torch.equal(by[ny:], torch.full_like(by[ny:], CANARY))
    assert torch.equal(bx[:nx].view(n_rep, F, P, T), project(sd, thd, shd, scd))
    assert torch.equal(by[:ny].view(1, F, P, T), project(td[None], thd, shd, scd))
    buf = torch.full((8,), CANARY, device=dev())
    assert ops.swd_project_pair(torch.randn(1, 2, 1, 100, device=dev()), torch.randn(2, 1, 100, device=dev()), torch.randn(4, 100, device=dev()), shd, scd,
                                buf, buf, 1, 2, 1, 100, 4) is False and torch.equal(buf, torch.full_like(buf, CANARY))


def test_projection_nan_stays_in_its_field():
    d, P = 256, 100
    x = torch.randn(2, 70, 2, d, device=dev())
    x[1, 3, 1, 17] = float("nan")
    thd, = to_dev(R.theta32(d, P))
    p = project(x, thd, torch.zeros(2, device=dev()), torch.ones(2, device=dev()))
    bad = torch.zeros_like(p, dtype=torch.bool)
    bad[1, 1, :, 3] = True
    assert torch.equal(torch.isnan(p), bad)


# ------------------------------------------------------------------------------------------------------------------ distance

def _columns(T, n_rep, seed):
    g = np.random.default_rng(seed)
    F, P = 2, 3
    px, py = g.standard_normal((n_rep, F, P, T)).astype(np.float32), g.standard_normal((F, P, T)).astype(np.float32)
    r = n_rep - 1
    px[0, 0, 1], py[0, 1] = np.sort(px[0, 0, 1]), np.sort(py[0, 1])[::-1]           # sorted against reversed
    px[r, 1, 0], py[1, 0] = np.round(px[r, 1, 0]), np.round(py[1, 0])                 # many ties
    px[r, 1, 2], py[1, 2] = np.where(px[r, 1, 2] > 0, 0.0, -0.0), np.where(py[1, 2] > 0, -0.0, 0.0)  # +-0 only
    px[0, 1, 1] = py[1, 1]                                                             # identical
    px[r, 0, 0], py[0, 0] = np.sort(px[r, 0, 0]), np.sort(py[0, 0])                   # both already sorted
    return px, py


@pytest.mark.parametrize("n_rep", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 3, 64, 65, 257, 1000, 4097])
def test_distance_against_float64(T, n_rep):
    px, py = _columns(T, n_rep, 10 * T + n_rep)
    got, want = distance(*to_dev(px, py)).cpu().numpy(), R.d64(px, py[None])
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"T {T} n_rep {n_rep}: relative error over T 2^-52: {np.nanmax(np.where(want > 0, np.abs(got - want) / (R.D_RTOL(T) * want), 0)):.3g}")
    assert np.all(np.abs(got - want) <= R.D_RTOL(T) * want)
    assert got[n_rep - 1, 1, 2] == 0.0 and got[0, 1, 1] == 0.0


def test_distance_at_the_largest_column():
    g = np.random.default_rng(16384)
    px, py = g.standard_normal((1, 1, 1, 16384)).astype(np.float32), (0.5 + 2.0 * g.standard_normal((1, 1, 16384))).astype(np.float32)
    got, want = distance(*to_dev(px, py)).cpu().numpy(), R.d64(px, py[None])
    assert np.all(np.abs(got - want) <= R.D_RTOL(16384) * want)


@pytest.mark.parametrize("T", [1000, 4097])
def test_distance_same_bits_at_every_position(T):
    """one column pair at members 0, 2 and 4 of five, alone, and on a second call (256 threads at T = 1000, 1024 at 4097)"""
    px, py = _columns(T, 5, T)
    px[2, 0, 1] = px[4, 0, 1] = px[0, 0, 1]
    pxd, pyd = to_dev(px, py)
    a, b = distance(pxd, pyd), distance(pxd, pyd)
    assert torch.equal(a, b)
    alone = distance(*to_dev(px[:1, :1, 1:2], py[:1, 1:2]))
    for r in (0, 2, 4):
        assert a[r, 0, 1].item() == alone[0, 0, 0].item(), r


def test_distance_nan_column_is_nan_and_only_it():
    px, py = _columns(300, 3, 5)
    px[1, 0, 2, 150] = np.nan
    got = distance(*to_dev(px, py)).cpu().numpy()
    bad = np.zeros((3, 2, 3), bool)
    bad[1, 0, 2] = True
    assert np.array_equal(np.isnan(got), bad)
    py[1, 1, 299] = np.nan
    bad[:, 1, 1] = True
    assert np.array_equal(np.isnan(distance(*to_dev(px, py)).cpu().numpy()), bad)


# ------------------------------------------------------------------------------------------------------------------ the interface

def _check_e2e(got_D, s, t, th, shift, scale, tag):
    D, delta = R.e2e(s, t, th, shift, scale)
    eD, bD = np.abs(got_D - D), R.dp_bound(D, delta)
    eS, bS = np.abs(R.swd_of(got_D) - R.swd_of(D)), R.swd_bound(delta)
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"{tag}: D_p error / bound {np.nanmax(np.where(bD > 0, eD / bD, 0)):.3g}, SWD error / bound {np.nanmax(np.where(bS > 0, eS / bS, 0)):.3g}")
    assert np.all(eD <= bD) and np.all(eS <= bS)


@pytest.mark.parametrize("kind", R.KINDS)
def test_end_to_end_against_float64(kind):
    n_rep, T, F, H, W_ = 3, 37, 2, 16, 24
    s, t, shift, scale = R.fields(kind, n_rep, T, F, H * W_)
    sd, td, shd, scd = to_dev(s.reshape(n_rep, T, F, H, W_), t.reshape(T, F, H, W_), shift, scale)
    got = W.sliced_wasserstein(sd, td, shift=shd, scale=scd, per_projection=True)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (n_rep, F, 100)
    _check_e2e(got.cpu().numpy(), s, t, R.theta32(H * W_), shift, scale, kind)
    if kind == "white":
        same = W.sliced_wasserstein(td[None].expand(2, T, F, H, W_), td)
        assert torch.equal(same, torch.zeros(2, F, dtype=torch.float64, device=dev()))  # identical ensembles: exactly zero


def test_unsupported_shapes_answer_false_write_nothing_and_take_the_general_route():
    assert not ops.swd_supported(100, 16, 8) and not ops.swd_supported(64, 129, 8) and not ops.swd_supported(64, 16, 16385)
    assert ops.swd_supported(64, 1, 1) and ops.swd_supported(65536, 128, 16384)
    one = torch.ones(1, device=dev())
    for d, P in ((100, 16), (64, 129)):
        buf = torch.full((P * 4 + TAIL,), CANARY, device=dev())
        assert ops.swd_project(torch.randn(1, 4, 1, d, device=dev()), torch.randn(P, d, device=dev()), one, one, buf, 1, 4, 1, d, P) is False
        assert torch.equal(buf, torch.full_like(buf, CANARY))
    out = torch.full((2 + TAIL,), CANARY, dtype=torch.float64, device=dev())
    big = torch.randn(2, 1, 1, 16385, device=dev())
    assert ops.swd_distance(big, big[0], out, 2, 1, 1, 16385) is False
    assert torch.equal(out, torch.full_like(out, CANARY))
    for H, W_, P, T in ((10, 10, 16, 4), (8, 8, 129, 4), (8, 8, 4, 16385)):
        s, t, shift, scale = R.fields("temperature", 2, T, 1, H * W_)
        got = W.sliced_wasserstein(*to_dev(s.reshape(2, T, 1, H, W_), t.reshape(T, 1, H, W_)), n_projections=P, shift=float(shift[0]),
                                   scale=float(scale[0]), per_projection=True)
        assert got.is_cuda and got.shape == (2, 1, P)
        _check_e2e(got.cpu().numpy(), s, t, R.theta32(H * W_, P), shift, scale, f"general {H}x{W_} P {P} T {T}")


def test_nan_stays_in_its_member_and_variable():
    s, t, shift, scale = R.fields("white", 3, 40, 2, 256)
    S, Tr = to_dev(s.reshape(3, 40, 2, 16, 16), t.reshape(40, 2, 16, 16))
    S[1, 22, 0, 3, 3] = float("nan")
    bad = torch.zeros(3, 2, dtype=torch.bool, device=dev())
    bad[1, 0] = True
    assert torch.equal(torch.isnan(W.sliced_wasserstein(S, Tr)), bad)   # one sample field: exactly that (member, variable)
    Tr[7, 1, 0, 0] = float("nan")
    bad[:, 1] = True
    shd, scd = to_dev(shift, scale)
    assert torch.equal(torch.isnan(W.sliced_wasserstein(S, Tr, shift=shd, scale=scd)), bad)  # one truth field: that variable, all members
    assert torch.equal(torch.isnan(W.sliced_wasserstein(S, Tr)), bad)


def test_strided_half_precision_input_agrees_with_the_dense_route():
    base = (torch.randn(2, 9, 3, 16, 32, device=dev()) * 3.0 + 1.0).to(torch.float16)
    view, truth = base[..., ::2], base[0, ..., 1::2]  # (2, 9, 3, 16, 16) against (9, 3, 16, 16)
    got = W.sliced_wasserstein(view, truth, shift=1.0, scale=0.25, per_projection=True)
    assert got.shape == (2, 3, 100) and got.dtype == torch.float64 and got.is_cuda
    x, y = view.float().contiguous(), truth.float().contiguous()
    dense = W.sliced_wasserstein(x, y, shift=1.0, scale=0.25, per_projection=True)
    assert torch.equal(got, dense)  # the same fp32 values through the same kernels
    _check_e2e(got.cpu().numpy(), x.cpu().numpy().reshape(2, 9, 3, 256), y.cpu().numpy().reshape(9, 3, 256), R.theta32(256),
               np.full(3, 1.0, np.float32), np.full(3, 0.25, np.float32), "strided fp16")


def test_report_on_the_device_equals_the_cpu_report():
    """(M, T, F) = (2, 5, 2) at 16 x 24, de-normalised (temperature-like and pressure-like).  Both reports lie within the end-to-end
    bound of the float64 value on the fp32 operands -- the CPU one, float64 throughout, within 1/32 of it (x^ formed in float64 instead
    of fp32: 2^-23 sum |x^ theta| against the floor's 2^-18) -- and a moment that rounds to the neighbouring fp32 on the other device
    moves the score by 2^-24 of itself (the scale) or not at all (the shift)"""
    g = np.random.default_rng(9)
    off, sd = np.array([280.0, 101325.0]), np.array([10.0, 1200.0])
    truth = (off[None, :, None, None] + sd[None, :, None, None] * g.standard_normal((5, 2, 16, 24))).astype(np.float32)
    samples = (off[None, None, :, None, None] + 1.3 * sd[None, None, :, None, None] * g.standard_normal((2, 5, 2, 16, 24))).astype(np.float32)
    cpu = W.swd_report(torch.tensor(samples), torch.tensor(truth), names=["tas", "psl"])
    gpu = W.swd_report(*to_dev(samples, truth), names=["tas", "psl"])
    shift = np.float32([float(cpu[n]["shift"]) for n in ("tas", "psl")])
    scale = np.float32([float(cpu[n]["scale"]) for n in ("tas", "psl")])
    _, delta = R.e2e(samples.reshape(2, 5, 2, 384), truth.reshape(5, 2, 384), R.theta32(384), shift, scale)
    for f, (name, v) in enumerate(gpu):
        assert v["wasserstein"].is_cuda and v["wasserstein"].shape == (2,) and v["wasserstein"].dtype == torch.float64
        assert float(v["shift"]) == pytest.approx(float(cpu[name]["shift"]), rel=2e-7) and float(v["scale"]) == pytest.approx(float(cpu[name]["scale"]), rel=2e-7)
        want = cpu[name]["wasserstein"].numpy()
        e, b = np.abs(v["wasserstein"].cpu().numpy() - want), (1.0 + 1.0 / 32.0) * R.swd_bound(delta)[:, f] + 2.0 ** -23 * want
        print(f"{name}: SWD {want}, device against CPU report: error / bound {np.max(e / b):.3g}")
        assert np.all(e <= b)
    assert set(gpu.as_dict()) == set(cpu.as_dict())
