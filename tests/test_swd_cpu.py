"""CPU checks of the ensemble sliced Wasserstein distance (climate2weather_amd.wasserstein): both routes of sliced_wasserstein -- the
general float64 one and the launcher's, with tests/emu_swd_ops.py standing in for the HIP kernels -- against the float64 definition by
the rule of tests/fp64_swd_ref.py, the projection generator, the report against a line-by-line restatement of the reference's loop, the
exact cases, the rule's negative control, the argument checks, the kernels' own index maps and arithmetic compiled for the host
(csrc/swd_core.h), and the C declarations against the ctypes prototypes."""
import os
import subprocess

import numpy as np
import pytest
import torch

import c_abi
import emu_swd_ops
import fp64_swd_ref as R
import host_program
from climate2weather_amd import ops as c2w_ops
from climate2weather_amd import wasserstein as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=["general", "launcher"])
def route(request, monkeypatch):
    """both branches of wasserstein.sliced_wasserstein on CPU tensors"""
    if request.param == "launcher":
        emu_swd_ops.install(monkeypatch, c2w_ops, W)
    return request.param


def _check(got_D, samples, truth, th, shift, scale, tag):
    """got_D (n_rep, F, P) against the float64 D_p on the same fp32 operands, per projection and as the score, by the end-to-end rule"""
    D, delta = R.e2e(samples, truth, th, shift, scale)
    eD, bD = np.abs(got_D - D), R.dp_bound(D, delta)
    eS, bS = np.abs(R.swd_of(got_D) - R.swd_of(D)), R.swd_bound(delta)
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"{tag}: D_p error / bound {np.nanmax(np.where(bD > 0, eD / bD, 0)):.3g}, SWD error / bound {np.nanmax(np.where(bS > 0, eS / bS, 0)):.3g}")
    assert np.all(eD <= bD) and np.all(eS <= bS)
    return D


# ------------------------------------------------------------------------------------------------------------------ both routes

@pytest.mark.parametrize("n_rep,T,F,H,W_", [(2, 5, 2, 8, 8), (1, 3, 1, 8, 24), (3, 7, 4, 16, 16)])
def test_every_field_kind_against_float64(route, n_rep, T, F, H, W_):
    d = H * W_
    th = R.theta32(d, 16)
    for kind in R.KINDS:
        s, t, shift, scale = R.fields(kind, n_rep, T, F, d)
        got = W.sliced_wasserstein(torch.tensor(s).view(n_rep, T, F, H, W_), torch.tensor(t).view(T, F, H, W_), theta=torch.tensor(th),
                                   shift=torch.tensor(shift), scale=torch.tensor(scale), per_projection=True)
        assert got.dtype == torch.float64 and got.shape == (n_rep, F, 16)
        _check(got.numpy(), s, t, th, shift, scale, f"{route} {kind} {(n_rep, T, F, d)}")


def test_defaults_are_the_reference_s(route):
    """100 projections from seed 0, the truth's own moments; leading dimensions are kept"""
    s, t, shift, scale = R.fields("temperature", 6, 4, 2, 64)
    S, Tr = torch.tensor(s).view(2, 3, 4, 2, 8, 8), torch.tensor(t).view(4, 2, 8, 8)
    got = W.sliced_wasserstein(S, Tr)
    assert got.shape == (2, 3, 2) and got.dtype == torch.float64
    m_shift, m_scale = W.truth_moments(Tr)
    assert m_shift.dtype == torch.float32 and m_shift.shape == (2,) and m_scale.dtype == torch.float32
    assert np.allclose(m_shift.numpy(), shift, rtol=2e-7, atol=0) and np.allclose(m_scale.numpy(), scale, rtol=2e-7, atol=0)
    D, delta = R.e2e(s, t, R.theta32(64), m_shift.numpy(), m_scale.numpy())
    assert np.all(np.abs(got.numpy().reshape(6, 2) - R.swd_of(D)) <= R.swd_bound(delta))
    as_given = W.sliced_wasserstein(S, Tr, shift=0, scale=1, n_projections=7, seed=3)
    D, delta = R.e2e(s, t, R.theta32(64, 7, 3), np.zeros(2, np.float32), np.ones(2, np.float32))
    assert np.all(np.abs(as_given.numpy().reshape(6, 2) - R.swd_of(D)) <= R.swd_bound(delta))


def test_any_dtype_any_strides(route):
    base = torch.randn(2, 3, 2, 8, 16, dtype=torch.float64)
    view, tv = base[..., ::2], base[0, ..., 1::2]  # (2, 3, 2, 8, 8) and (3, 2, 8, 8), strided
    for cast in (torch.float64, torch.float16):
        got = W.sliced_wasserstein(view.to(cast), tv.to(cast), shift=0.5, scale=2.0, n_projections=5, per_projection=True)
        assert got.dtype == torch.float64 and got.shape == (2, 2, 5)
        s32, t32 = view.to(cast).float().numpy().reshape(2, 3, 2, 64), tv.to(cast).float().numpy().reshape(3, 2, 64)
        _check(got.numpy(), s32, t32, R.theta32(64, 5), np.full(2, 0.5, np.float32), np.full(2, 2.0, np.float32), f"{route} {cast}")


def test_identical_ensembles_give_exactly_zero(route):
    _, t, shift, scale = R.fields("pressure", 1, 6, 2, 64)
    Tr = torch.tensor(t).view(6, 2, 8, 8)
    got = W.sliced_wasserstein(Tr[None].expand(3, 6, 2, 8, 8), Tr)
    assert got.shape == (3, 2) and torch.equal(got, torch.zeros(3, 2, dtype=torch.float64))


def test_a_shift_along_theta_0_gives_its_square(route):
    """x = y + c theta_0 moves column 0 by c (theta_0 . theta_0 = 1) and nothing sorts differently: D_0 = c^2 to rounding -- the route's
    own bound plus the fp32 rounding of the shifted field and of theta (2^-24 sum |x theta| each) and of the unit norm (2^-24 c)"""
    d, c, T = 192, 0.75, 9
    t = np.random.default_rng(11).standard_normal((T, 1, d)).astype(np.float32)
    th = R.theta32(d)
    s = (t.astype(np.float64) + c * R.theta64(d)[:, 0]).astype(np.float32)[None]
    got = W.sliced_wasserstein(torch.tensor(s).view(1, T, 1, 8, 24), torch.tensor(t).view(T, 1, 8, 24), shift=0, scale=1, per_projection=True)
    zero, one = np.zeros(1, np.float32), np.ones(1, np.float32)
    _, delta = R.e2e(s, t, th, zero, one)
    data = R.U * (2.0 * np.sqrt((R.abs_sum(s[0, :, 0], th[:1]) ** 2).mean()) + c)
    e = abs(np.sqrt(got[0, 0, 0].item()) - c)
    print(f"{route}: |sqrt(D_0) - c| = {e:.3g}, bound {delta[0, 0, 0] + data:.3g}")
    assert e <= delta[0, 0, 0] + data


def test_nan_stays_in_its_member_and_variable(route):
    s, t, shift, scale = R.fields("white", 3, 4, 2, 64)
    S, Tr = torch.tensor(s).view(3, 4, 2, 8, 8).clone(), torch.tensor(t).view(4, 2, 8, 8).clone()
    S[1, 2, 0, 3, 3] = float("nan")
    got = W.sliced_wasserstein(S, Tr, shift=torch.tensor(shift), scale=torch.tensor(scale))
    bad = torch.zeros(3, 2, dtype=torch.bool)
    bad[1, 0] = True
    assert torch.equal(torch.isnan(got), bad)
    Tr[0, 1, 0, 0] = float("nan")
    bad[:, 1] = True
    got = W.sliced_wasserstein(S, Tr, shift=torch.tensor(shift), scale=torch.tensor(scale))
    assert torch.equal(torch.isnan(got), bad)
    got = W.sliced_wasserstein(S, Tr)  # the moments of a variable with a NaN are NaN: still that variable only
    assert torch.equal(torch.isnan(got), bad)


# ------------------------------------------------------------------------------------------------------------------ projections

def test_projections_are_the_reference_s_generator():
    th = W.projections(192)
    assert th.shape == (100, 192) and th.dtype == torch.float32 and th.is_contiguous()
    raw = np.random.RandomState(0).randn(192, 100)
    want = raw / np.linalg.norm(raw, axis=0, keepdims=True)
    assert np.array_equal(th.numpy(), want.T.astype(np.float32))
    assert np.abs(np.linalg.norm(th.numpy().astype(np.float64), axis=1) - 1.0).max() <= 2.0 ** -24  # rounded entries of a unit column
    assert W.projections(192) is th  # cached: the same directions for every variable and every call
    assert not np.array_equal(W.projections(192, seed=1).numpy(), th.numpy())
    assert W.projections(64, 7).shape == (7, 64)
    assert np.array_equal(R.theta32(192), th.numpy())


# ------------------------------------------------------------------------------------------------------------------ report

def _ensemble(H, W_, M=2, T=5, F=2, seed=5):
    """de-normalised: variable 0 temperature-like, variable 1 pressure-like"""
    rng = np.random.default_rng(seed)
    off, sd = np.array([280.0, 101325.0]), np.array([10.0, 1200.0])
    truth = off[None, :, None, None] + sd[None, :, None, None] * rng.standard_normal((T, F, H, W_))
    samples = off[None, None, :, None, None] + 1.2 * sd[None, None, :, None, None] * rng.standard_normal((M, T, F, H, W_))
    return samples.astype(np.float32), truth.astype(np.float32)


def _report_tolerance(samples, truth, f, want):
    """the route against float64 on the same fp32 operands (the end-to-end bound), plus what separates those operands from the
    reference's float64 ones: theta rounded once (a projection moves by at most 2^-24 sum |x^ theta|) and x^ formed in fp32 (two
    roundings, 2^-23 sum |x^ theta|) -- together 3/64 of the bound's floor term; the shift's rounding moves sample and truth alike and
    cancels; the scale's multiplies the score by 1 +- 2^-24"""
    M, T, F, H, W_ = samples.shape
    t64 = truth[:, f].astype(np.float64)
    shift, scale = np.float32([t64.mean()]), np.float32([1.0 / t64.std()])
    _, delta = R.e2e(samples[:, :, f].reshape(M, T, 1, H * W_), truth[:, f].reshape(T, 1, H * W_), R.theta32(H * W_), shift, scale)
    return (1.0 + 3.0 / 64.0) * R.swd_bound(delta)[:, 0] + 2.0 ** -23 * want


@pytest.mark.parametrize("H,W_", [(8, 8), (16, 24)])
def test_report_against_the_reference_loop(route, H, W_):
    samples, truth = _ensemble(H, W_)
    rep = W.swd_report(torch.tensor(samples), torch.tensor(truth), names=["tas", "psl"])
    assert rep.names == ["tas", "psl"]
    for f, (name, v) in enumerate(rep):
        want, gtmean, gtstd = R.swd_reference(samples[:, :, f], truth[:, f])
        assert set(v) == {"wasserstein", "shift", "scale"} and rep[name] is v
        assert v["wasserstein"].shape == (2,) and v["wasserstein"].dtype == torch.float64
        assert float(v["shift"]) == pytest.approx(gtmean, rel=1e-6) and float(v["scale"]) == pytest.approx(1.0 / gtstd, rel=1e-6)
        e, b = np.abs(v["wasserstein"].numpy() - want), _report_tolerance(samples, truth, f, want)
        print(f"{route} {name} {H}x{W_}: SWD {want}, error / bound {np.max(e / b):.3g}")
        assert np.all(e <= b)
    flat = rep.as_dict()
    assert set(flat) == {f"wasserstein/{n}/wasserstein{s}" for n in ("tas", "psl") for s in ("", "_std")}
    assert all(isinstance(x, float) for x in flat.values())
    w1 = rep["psl"]["wasserstein"].numpy()
    assert flat["wasserstein/psl/wasserstein"] == pytest.approx(w1.mean(), rel=1e-12) and flat["wasserstein/psl/wasserstein_std"] == pytest.approx(w1.std(), abs=1e-12)


def test_report_t_step_names_and_argument_checks(route):
    samples, truth = _ensemble(8, 8, T=7)
    rep = W.swd_report(torch.tensor(samples), torch.tensor(truth), t_step=3)
    assert rep.names == ["var0", "var1"] and set(rep.as_dict("eval")) == {f"eval/var{f}/wasserstein{s}" for f in range(2) for s in ("", "_std")}
    for f, (_, v) in enumerate(rep):
        want, gtmean, _ = R.swd_reference(samples[:, ::3, f], truth[::3, f])  # the moments too are over the kept frames only
        assert float(v["shift"]) == pytest.approx(gtmean, rel=1e-6)
        assert np.all(np.abs(v["wasserstein"].numpy() - want) <= _report_tolerance(samples[:, ::3], truth[::3], f, want))
    with pytest.raises(ValueError):
        W.swd_report(torch.tensor(samples), torch.tensor(truth[:2]))
    with pytest.raises(ValueError):
        W.swd_report(torch.tensor(samples), torch.tensor(truth), names=["only_one"])
    with pytest.raises(ValueError):
        W.swd_report(torch.tensor(samples), torch.tensor(truth), t_step=0)


# ------------------------------------------------------------------------------------------------------------------ the rule bites

def test_project_then_normalise_in_fp32_fails_the_rule_on_pressure_like_fields():
    """the reference's 128 x 128: a straight fp32 port of (theta . x - shift sum(theta)) * scale against the same loop on x^"""
    d, P = 16384, 8
    th = R.theta32(d, P)
    s, _, shift, scale = R.fields("pressure", 1, 4, 1, d)  # 32 entries
    xh = R.xhat32(s, shift, scale)
    p64 = R.project64(xh, th)
    b = R.proj_bound(xh, th, p64)
    e_naive, e_first = np.abs(R.project_naive32(s, th, shift, scale) - p64), np.abs(R.chain32(xh, th) - p64)
    raw = torch.matmul(torch.tensor(s.reshape(-1, d)), torch.tensor(th).t()).numpy().reshape(1, 4, 1, P)
    e_blocked = np.abs(((raw - shift[:, None] * th.sum(axis=1, dtype=np.float32)) * scale[:, None]).astype(np.float64) - p64)
    print(f"pressure-like, d = {d}, error / bound (limit 1): straight loop, project then normalise: median {np.median(e_naive / b):.3g} max "
          f"{np.max(e_naive / b):.3g}; straight loop on x^: max {np.max(e_first / b):.3g}; torch.matmul, project then normalise: max "
          f"{np.max(e_blocked / b):.3g}")
    assert not np.all(e_naive <= b) and np.max(e_naive / b) > 1.5  # the rule asks every entry to pass
    assert np.all(e_first <= b) and np.max(e_first / b) < 0.1      # and it is the offset that does it


# ------------------------------------------------------------------------------------------------------------------ arguments

def test_argument_checks(monkeypatch):
    x, y = torch.zeros(2, 3, 2, 8, 8), torch.zeros(3, 2, 8, 8)
    with pytest.raises(ValueError):
        W.sliced_wasserstein(x[:, :2], y)  # unequal counts
    with pytest.raises(ValueError):
        W.sliced_wasserstein(x, torch.zeros(3, 2, 8, 16))
    with pytest.raises(ValueError):
        W.sliced_wasserstein(x, torch.zeros(3, 1, 8, 8))
    with pytest.raises(ValueError):
        W.sliced_wasserstein(x[0, 0], y)
    with pytest.raises(ValueError):
        W.sliced_wasserstein(x, y, theta=torch.zeros(4, 63))
    with pytest.raises(ValueError):
        W.sliced_wasserstein(x, y, shift=0)
    with pytest.raises(ValueError):
        W.sliced_wasserstein(x, y, shift=torch.zeros(3), scale=1)
    with pytest.raises(ValueError):
        W.truth_moments(torch.zeros(3, 8, 8))
    empty = W.sliced_wasserstein(torch.zeros(0, 3, 2, 8, 8), y, shift=0, scale=1)
    assert empty.shape == (0, 2) and empty.dtype == torch.float64


def test_unsupported_shapes_take_the_general_route(monkeypatch):
    """P > 128 and d no multiple of 64: the launcher is asked, answers no, nothing is launched, the float64 route answers"""
    emu_swd_ops.install(monkeypatch, c2w_ops, W)
    for H, W_, P in ((8, 8, 129), (10, 10, 16)):
        d = H * W_
        s, t, shift, scale = R.fields("temperature", 2, 4, 2, d)
        got = W.sliced_wasserstein(torch.tensor(s).view(2, 4, 2, H, W_), torch.tensor(t).view(4, 2, H, W_), n_projections=P, per_projection=True)
        assert emu_swd_ops.CALLS == [] and got.shape == (2, 2, P)
        _check(got.numpy(), s, t, R.theta32(d, P), shift, scale, f"general {H}x{W_} P {P}")
    s, t, shift, scale = R.fields("white", 2, 4, 2, 64)
    W.sliced_wasserstein(torch.tensor(s).view(2, 4, 2, 8, 8), torch.tensor(t).view(4, 2, 8, 8), n_projections=5)
    assert emu_swd_ops.CALLS == [("project", 1, 4, 2, 64, 5), ("project", 2, 4, 2, 64, 5), ("distance", 2, 2, 5, 4)]  # the truth once


# ------------------------------------------------------------------------------------------------------------------ the kernels' maps

@pytest.fixture(scope="module")
def host_swd(tmp_path_factory):
    return host_program.build(tmp_path_factory, "swd", sanitize=False, timeout=300)


def _host_project(exe, tmp, x, th, shift, scale):
    n_rep, T, F, d = x.shape
    P = th.shape[0]
    for name, a in (("x", x), ("th", th), ("sh", shift), ("sc", scale)):
        np.ascontiguousarray(a, dtype=np.float32).tofile(tmp / f"{name}.f32")
    subprocess.run([str(exe), "project", str(n_rep), str(T), str(F), str(d), str(P)] + [str(tmp / f"{n}.f32") for n in ("x", "th", "sh", "sc", "proj")],
                   check=True, timeout=300)
    return np.fromfile(tmp / "proj.f32", dtype=np.float32).reshape(n_rep, F, P, T)


def _host_distance(exe, tmp, px, py):
    n_rep, F, P, T = px.shape
    np.ascontiguousarray(px, dtype=np.float32).tofile(tmp / "px.f32"), np.ascontiguousarray(py, dtype=np.float32).tofile(tmp / "py.f32")
    subprocess.run([str(exe), "distance", str(n_rep), str(F), str(P), str(T), str(tmp / "px.f32"), str(tmp / "py.f32"), str(tmp / "out.f64")],
                   check=True, timeout=300)
    return np.fromfile(tmp / "out.f64", dtype=np.float64).reshape(n_rep, F, P)


@pytest.mark.parametrize("n_rep,T,F,d,P", [(1, 1, 1, 64, 1), (2, 3, 2, 192, 100), (3, 65, 1, 64, 128), (3, 37, 4, 192, 16), (1, 2, 3, 1024, 33)])
def test_projection_phases_on_the_host_meet_the_rule(host_swd, tmp_path, n_rep, T, F, d, P):
    """csrc/swd_core.h compiled for the host: the staging maps, the fragment maps, the accumulator map, the fold, the epilogue's two maps
    and i % F, with several workgroups of 64 fields and a partly empty last one at 3 x 65 and 3 x 37 x 4 fields; every kind by the rule"""
    th = R.theta32(d, P)
    for kind in R.KINDS:
        s, _, shift, scale = R.fields(kind, n_rep, T, F, d)
        got = _host_project(host_swd, tmp_path, s, th, shift, scale).astype(np.float64)
        xh = R.xhat32(s, shift, scale)
        p64 = R.project64(xh, th)
        e, b = np.abs(np.moveaxis(got, -1, 1) - p64), R.proj_bound(xh, th, p64)  # (n_rep, T, F, P)
        with np.errstate(invalid="ignore", divide="ignore"):
            print(f"{kind} {(n_rep, T, F, d, P)}: error / bound {np.nanmax(np.where(b > 0, e / b, 0)):.3g}")
        assert np.all(e <= b), kind


def test_projection_on_the_host_is_the_documented_chain_bit_for_bit(host_swd, tmp_path):
    """the k order: chunks of 256 in ascending order, inside a chunk steps of 32, inside a step groups of 8 as k = 8 g + s, 8 g + 4 + s
    for s = 0 .. 3; an fmaf chain from zero per chunk, the chunk sums added in order -- restated here in NumPy (an fp32 fmaf is the
    float64 product, exact, plus the float64 sum rounded to fp32; the double rounding differs from fmaf's single one only on ties of
    the float64 sum, which random data does not produce at these sizes) and compared bit for bit, at every batch position"""
    d, P, F = 320, 5, 2
    th = R.theta32(d, P)
    s, _, shift, scale = R.fields("temperature", 1, 70, F, d)  # 140 fields: three workgroups
    s[0, 69, 1] = s[0, 0, 1]  # row 1 of workgroup 0 again as row 11 of workgroup 2
    got = _host_project(host_swd, tmp_path, s, th, shift, scale)
    xh = R.xhat32(s, shift, scale)[0].astype(np.float64)  # (T, F, d)
    t64 = th.astype(np.float64)
    order = [32 * st + 8 * g + 4 * h + q for st in range(d // 32) for g in range(4) for q in range(4) for h in range(2)]
    assert sorted(order) == list(range(d))
    tot, acc = np.zeros((70, F, P), np.float32), np.zeros((70, F, P), np.float32)
    for n, k in enumerate(order):
        acc = (xh[:, :, k, None] * t64[None, None, :, k] + acc.astype(np.float64)).astype(np.float32)
        if (n + 1) % 256 == 0 or n + 1 == d:
            tot, acc = tot + acc, np.zeros_like(acc)
    assert tot.dtype == np.float32 and np.array_equal(np.moveaxis(got[0], -1, 0), tot)
    assert np.array_equal(got[0, 1, :, 69], got[0, 1, :, 0])


@pytest.mark.parametrize("T", [1, 2, 3, 65, 300, 2500])
def test_sort_network_on_the_host(host_swd, tmp_path, T):
    """every padded size class (N = 1, 2, 4, 128, 512 at 256 threads, 4096 at 1024) on random, sorted, reversed, tied and signed-zero
    columns, three members against one truth: relative error <= T 2^-52 of the float64 value; a NaN column is NaN and only it"""
    g = np.random.default_rng(T)
    F, P = 2, 3
    px, py = g.standard_normal((3, F, P, T)).astype(np.float32), g.standard_normal((F, P, T)).astype(np.float32)
    px[0, 0, 1], py[0, 1] = np.sort(px[0, 0, 1]), np.sort(py[0, 1])[::-1]         # sorted against reversed
    px[1, 1, 0], py[1, 0] = np.round(px[1, 1, 0]), np.round(py[1, 0])               # many ties
    px[2, 1, 2], py[1, 2] = np.where(px[2, 1, 2] > 0, 0.0, -0.0), np.where(py[1, 2] > 0, -0.0, 0.0)  # +-0 only
    px[1, 1, 1] = py[1, 1]                                                            # identical
    got, want = _host_distance(host_swd, tmp_path, px, py), R.d64(px, py[None])
    assert np.all(np.abs(got - want) <= R.D_RTOL(T) * want)
    assert got[2, 1, 2] == 0.0 and got[1, 1, 1] == 0.0
    px[1, 0, 2, T // 2] = np.nan
    got = _host_distance(host_swd, tmp_path, px, py)
    bad = np.zeros((3, F, P), bool)
    bad[1, 0, 2] = True
    assert np.array_equal(np.isnan(got), bad) and np.all(np.abs(got[~bad] - want[~bad]) <= R.D_RTOL(T) * want[~bad])
    py[1, 1, 0] = np.nan
    bad[:, 1, 1] = True
    assert np.array_equal(np.isnan(_host_distance(host_swd, tmp_path, px, py)), bad)


def test_support_predicates_agree():
    for d, P, T, want in ((64, 1, 1, True), (65536, 128, 16384, True), (100, 16, 8, False), (32, 16, 8, False), (65600, 16, 8, False),
                          (64, 129, 8, False), (64, 0, 8, False), (64, 16, 16385, False), (64, 16, 0, False)):
        assert emu_swd_ops.swd_supported(d, P, T) is want
    core = open(os.path.join(ROOT, "climate2weather_amd", "csrc", "swd_core.h")).read()
    assert "MAX_D = 65536, MAX_P = BN, MAX_T = 16384" in core and "d % 64 == 0" in core


# ------------------------------------------------------------------------------------------------------------------ C ABI

def test_new_entry_points_have_matching_argument_lists():
    names = {"c2w_swd_supported": "int", "c2w_swd_project": "int", "c2w_swd_project_pair": "int", "c2w_swd_distance": "int"}
    c_abi.assert_declared(names, "swd.hip")
