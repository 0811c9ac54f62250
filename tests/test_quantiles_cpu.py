"""CPU checks of the exact quantiles (climate2weather_amd.quantiles, normalize.QuantileNormalizer.from_data): the restated definition
of tests/fp64_quantile_ref.py against numpy.quantile / numpy.nanquantile, both routes of quantiles.quantile -- the general float64 sort
and the launcher's, with tests/emu_quantile_ops.py standing in for the HIP kernels -- against that definition, the normaliser built from
the data against one built from numpy's values, the report, the argument checks, the kernels' own maps and slot logic compiled for the
host (csrc/quantile_core.h) under the address and undefined-behaviour sanitizers, and the C declarations against the ctypes prototypes.
Everything is exact: no tolerance appears."""
import os
import subprocess
import warnings

import numpy as np
import pytest
import torch

import c_abi
import emu_quantile_ops
import fp64_quantile_ref as R
import host_program
from climate2weather_amd import normalize as Nm
from climate2weather_amd import ops as c2w_ops
from climate2weather_amd import quantiles as Qt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 3, 2, 64), (1, 13, 1, 256), (1, 1, 1, 4), (2, 37, 3, 8)]  # (n_rep, T, F, hw): n = 192, 3328, 4, 296


@pytest.fixture(params=["general", "launcher"])
def route(request, monkeypatch):
    """both branches of quantiles.quantile on CPU tensors"""
    if request.param == "launcher":
        emu_quantile_ops.install(monkeypatch, c2w_ops, Qt)
    return request.param


def _t5(s, t, H, W_):
    """(n_rep, T, F, hw), (T, F, hw) arrays -> the (n_rep, T, F, H, W), (T, F, H, W) tensors of the public interface"""
    return torch.tensor(s).view(s.shape[:3] + (H, W_)), torch.tensor(t).view(t.shape[:2] + (H, W_))


# ------------------------------------------------------------------------------------------------------------------ the definition

@pytest.mark.parametrize("kind", R.KINDS)
def test_the_definition_is_numpy_s(kind):
    """numpy.quantile(x.astype(float64), q) and numpy.nanquantile with their defaults (method="linear"), every level set"""
    for shape in SHAPES:
        for level_set in R.LEVEL_SETS:
            for skipna in (True, False):
                s, t, q, out, stats, nv = R.case(kind, *shape, level_set, True, skipna)
                for i, v in enumerate(R.data_sets(s, t)):
                    with warnings.catch_warnings(), np.errstate(all="ignore"):
                        warnings.simplefilter("ignore")
                        want = (np.nanquantile if skipna else np.quantile)(v.astype(np.float64), q)
                    assert R.same_numbers(out[i], want), (shape, level_set, skipna, i)
                    assert nv[i] == np.count_nonzero(~np.isnan(v))


def test_the_key_is_monotone_and_invertible():
    v = np.array([-np.inf, -3.5, -1e-41, -0.0, 0.0, 1e-45, 1e-41, 1.0, 280.0, np.float32(280.0) + np.float32(2.0 ** -15), np.inf], np.float32)
    k = R.key_of(v.view(np.uint32))
    assert np.all(np.diff(k.astype(np.int64)) > 0)  # strictly: -0.0 below +0.0, denormals apart
    assert np.array_equal(R.bits_of(k), v.view(np.uint32)) and np.array_equal(emu_quantile_ops.key_of(v.view(np.uint32)), k)


# ------------------------------------------------------------------------------------------------------------------ both routes

@pytest.mark.parametrize("n_rep,T,F,H,W_", [(2, 3, 2, 8, 8), (1, 13, 1, 16, 16), (1, 1, 1, 2, 2), (2, 37, 3, 2, 4)])
def test_every_field_kind_against_the_reference(route, n_rep, T, F, H, W_):
    for kind in R.KINDS:
        for level_set in R.LEVEL_SETS:
            s, t, q, out, stats, nv = R.case(kind, n_rep, T, F, H * W_, level_set)
            S, Tr = _t5(s, t, H, W_)
            (go, gs, gn), (to, ts, tn) = Qt.quantile(S, q, truth=Tr, return_stats=True)
            assert go.dtype == torch.float64 and go.shape == (n_rep, F, q.size) and to.shape == (F, q.size)
            assert gs.dtype == torch.float32 and gs.shape == (n_rep, F, q.size, 2) and gn.dtype == torch.int64 and gn.shape == (n_rep, F)
            k = n_rep * F
            assert R.same_numbers(go.numpy().reshape(k, -1), out[:k]) and R.same_numbers(to.numpy(), out[k:]), (kind, level_set)
            assert R.same_stats(gs.numpy().reshape(k, -1, 2), stats[:k]) and R.same_stats(ts.numpy(), stats[k:]), (kind, level_set)
            assert np.array_equal(gn.numpy().reshape(-1), nv[:k]) and np.array_equal(tn.numpy(), nv[k:])
        alone = Qt.quantile(S, q)  # without the truth, without the stats: the same rows
        assert R.same_numbers(alone.numpy(), go.numpy())


def test_skipna_false_poisons_its_own_row_only(route):
    s, t, q, out, stats, nv = R.case("nan", 2, 3, 2, 64, "nine", True, False)
    assert np.isnan(out).all()
    s, t = R.fields("normal", 2, 3, 2, 64)
    s = s.copy()
    s[1, 2, 0, 5] = np.nan
    S, Tr = _t5(s, t, 8, 8)
    (go, gs, gn), (to, ts, tn) = Qt.quantile(S, R.NINE, truth=Tr, skipna=False, return_stats=True)
    bad = torch.zeros(2, 2, dtype=torch.bool)
    bad[1, 0] = True
    assert torch.equal(torch.isnan(go).all(dim=-1), bad) and torch.equal(torch.isnan(go).any(dim=-1), bad) and not torch.isnan(to).any()
    assert torch.isnan(gs[1, 0]).all() and gn.tolist() == [[192, 192], [191, 192]]
    want, _, _ = R.expected(s, t, R.NINE, False)
    assert R.same_numbers(go.numpy().reshape(4, -1), want[:4]) and R.same_numbers(to.numpy(), want[4:])
    skipped = Qt.quantile(S, R.NINE)  # the default leaves the NaN out
    assert R.same_numbers(skipped.numpy().reshape(4, -1), R.expected(s, None, R.NINE, True)[0])


def test_any_dtype_any_strides_and_leading_dimensions(route):
    base = 280.0 + 10.0 * torch.randn(2, 3, 4, 2, 8, 16, dtype=torch.float64)
    view = base[..., ::2]  # (2, 3, 4, 2, 8, 8), strided
    for cast in (torch.float64, torch.float16, torch.bfloat16):
        v32 = view.to(cast).float().numpy().reshape(6, 4, 2, 64)
        got = Qt.quantile(view.to(cast), R.NINE)
        assert got.shape == (2, 3, 2, 9) and got.dtype == torch.float64
        assert R.same_numbers(got.numpy().reshape(12, 9), R.expected(v32, None, R.NINE)[0]), cast
    one = Qt.quantile(view, 0.5)  # a number is one level
    assert one.shape == (2, 3, 2, 1)


# ------------------------------------------------------------------------------------------------------------------ the normaliser

def _physical(T, F, H, W_, seed=3):
    rng = np.random.default_rng(seed)
    off, sd = np.array([280.0, 101325.0, 0.0, 3e-5])[:F], np.array([10.0, 900.0, 4.0, 2e-5])[:F]
    return (off[None, :, None, None] + sd[None, :, None, None] * rng.standard_normal((T, F, H, W_))).astype(np.float32)


@pytest.mark.parametrize("mode", sorted(Nm.MODES))
def test_from_data_equals_a_normaliser_built_from_numpy_quantiles(route, mode):
    x = _physical(6, 4, 8, 12)
    levels = sorted(set(Nm.MODES[mode]))
    table = {q: [np.quantile(x[:, f].astype(np.float64), q) for f in range(4)] for q in levels}
    want = Nm.QuantileNormalizer(table, mode)
    got = Nm.QuantileNormalizer.from_data(torch.tensor(x), mode)
    assert got.mode == mode and torch.equal(got.lower, want.lower) and torch.equal(got.range, want.range)
    for inverse in (False, True):
        for a, b in zip(got._coef("cpu", inverse), want._coef("cpu", inverse)):
            assert a.dtype == torch.float32 and torch.equal(a, b)
    lead = Nm.QuantileNormalizer.from_data(torch.tensor(x).view(2, 3, 4, 8, 12), mode)  # leading indices join the time axis
    assert torch.equal(lead.lower, want.lower) and torch.equal(lead.range, want.range)


def test_from_data_argument_checks_and_nans(route):
    x = torch.tensor(_physical(4, 2, 4, 4))
    with pytest.raises(ValueError):
        Nm.QuantileNormalizer.from_data(x, "zscore")
    with pytest.raises(ValueError):
        Nm.QuantileNormalizer.from_data(x[0])
    x[1, 0, 2, 2] = float("nan")
    skip = Nm.QuantileNormalizer.from_data(x)
    v = x[:, 0].numpy().astype(np.float64)
    assert float(skip.lower[0]) == np.nanquantile(v, 0.05) and not torch.isnan(skip.range).any()
    keep = Nm.QuantileNormalizer.from_data(x, skipna=False)
    assert torch.isnan(keep.lower).tolist() == [True, False]


# ------------------------------------------------------------------------------------------------------------------ the report

def test_report_values_names_and_argument_checks(route):
    rng = np.random.default_rng(5)
    truth = _physical(5, 2, 8, 8)
    samples = (truth[None] + rng.standard_normal((3, 5, 2, 8, 8)) * np.array([3.0, 300.0])[None, None, :, None, None]).astype(np.float32)
    S, Tr = torch.tensor(samples), torch.tensor(truth)
    rep = Qt.quantile_report(S, Tr, names=["tas", "psl"])
    assert rep.names == ["tas", "psl"] and rep.levels == R.NINE == Qt.REFERENCE_LEVELS
    want, _, _ = R.expected(samples.reshape(3, 5, 2, 64), truth.reshape(5, 2, 64), R.NINE)
    for f, (name, v) in enumerate(rep):
        assert set(v) == {"truth", "samples", "diff"} and rep[name] is v
        assert R.same_numbers(v["truth"].numpy(), want[6 + f]) and R.same_numbers(v["samples"].numpy(), want[f:6:2])
        assert R.same_numbers(v["diff"].numpy(), want[f:6:2] - want[6 + f][None])
    flat = rep.as_dict()
    assert set(flat) == {f"quantiles/{n}/q{q:g}/{k}" for n in ("tas", "psl") for q in R.NINE for k in ("truth", "mean", "bias", "max_abs_diff")}
    assert all(isinstance(x, float) for x in flat.values())
    assert flat["quantiles/psl/q0.99/truth"] == want[7, 7] and flat["quantiles/tas/q0.01/max_abs_diff"] == np.abs(want[0:6:2, 1] - want[6, 1]).max()
    short = Qt.quantile_report(S, Tr, q=[0.01, 0.99])
    assert short.names == ["var0", "var1"] and set(short.as_dict("eval")) >= {"eval/var1/q0.99/bias"} and short["var0"]["samples"].shape == (3, 2)
    with pytest.raises(ValueError):
        Qt.quantile_report(S, Tr[:2])
    with pytest.raises(ValueError):
        Qt.quantile_report(S, Tr, names=["only_one"])
    with pytest.raises(ValueError):
        Qt.quantile_report(S[0], Tr)
    with pytest.raises(ValueError):
        Qt.quantile_report(S, Tr, q=[0.5, 1.5])


def test_argument_checks(monkeypatch):
    emu_quantile_ops.install(monkeypatch, c2w_ops, Qt)
    x = torch.zeros(2, 3, 2, 8, 8)
    for bad in ([1.0001], [-1e-9], [0.5, float("nan")], []):
        with pytest.raises(ValueError):
            Qt.quantile(x, bad)
    assert emu_quantile_ops.CALLS == []  # refused before any launch
    with pytest.raises(ValueError):
        Qt.quantile(x[0, 0], [0.5])
    with pytest.raises(ValueError):
        Qt.quantile(x, [0.5], truth=torch.zeros(3, 2, 8, 4))
    with pytest.raises(ValueError):
        Qt.quantile(x[:, :0], [0.5])
    empty = Qt.quantile(torch.zeros(0, 3, 2, 8, 8), [0.25, 0.5])
    assert empty.shape == (0, 2, 2) and empty.dtype == torch.float64


def test_unsupported_shapes_take_the_general_route(monkeypatch):
    """hw no multiple of 4 and Q > 16: the launcher is asked, answers no, nothing is launched, the general route answers"""
    emu_quantile_ops.install(monkeypatch, c2w_ops, Qt)
    q17 = np.concatenate([R.levels("sixteen", 3 * 64), [0.123]])
    for H, W_, q in ((5, 5, np.array(R.NINE)), (8, 8, q17)):
        s, t = R.fields("nan", 2, 3, 2, H * W_)
        S, Tr = _t5(s, t, H, W_)
        calls = []
        monkeypatch.setattr(c2w_ops, "quantiles", lambda *a, **k: calls.append(a) or emu_quantile_ops.quantiles(*a, **k))
        (go, gs, gn), (to, ts, tn) = Qt.quantile(S, q, truth=Tr, return_stats=True)
        assert calls == []  # quantile_supported said no first
        want, stats, nv = R.expected(s, t, q)
        assert R.same_numbers(torch.cat([go.reshape(4, -1), to]).numpy(), want) and R.same_stats(torch.cat([gs.reshape(4, -1, 2), ts]).numpy(), stats)
        assert np.array_equal(torch.cat([gn.reshape(-1), tn]).numpy(), nv)
    assert emu_quantile_ops.quantiles(None, None, list(q17), True, None, None, None, None, 2, 3, 2, 64) is False  # and the launcher itself
    assert emu_quantile_ops.quantiles(None, None, [0.5], True, None, None, None, None, 2, 3, 2, 66) is False
    s, t = R.fields("normal", 2, 3, 2, 64)
    Qt.quantile_report(*_t5(s, t, 8, 8))
    assert emu_quantile_ops.CALLS[-1] == (2, 3, 2, 64, 9, True, True)  # samples and truth in ONE launch


def test_support_predicates_and_constants_agree():
    for hw, Q, want in ((4, 1, True), (16384, 16, True), (66, 9, False), (0, 9, False), (64, 17, False), (64, 0, False)):
        assert emu_quantile_ops.quantile_supported(hw, Q) is want
    core = open(os.path.join(ROOT, "climate2weather_amd", "csrc", "quantile_core.h")).read()
    for text in ("THREADS = 1024", "LOCATE_THREADS = 128", "MAX_Q = 16", "BITS0 = 12, BITS1 = 10, BITS2 = 10", "NONE = 255", "WG_PER_CU = 8", "LOADS = 4",
                 "hw % 4 == 0 && Q >= 1 && Q <= MAX_Q", "bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u)",
                 "pass == 0 ? BINS0 * 4 + 16 : 2 * Q * BINS * 4 + 2 * Q * 4 + BINS0 + 16"):
        assert text in core, text
    e = emu_quantile_ops
    assert (e.THREADS, e.LOCATE_THREADS, e.MAX_Q, e.BITS0, e.BITS1, e.BITS2, e.NONE, e.WG_PER_CU, e.LOADS) == (1024, 128, 16, 12, 10, 10, 255, 8, 4)
    # both workloads fill a 256-CU chip: the reference's preprocessing (D = 4) and eight members plus truth (D = 36)
    assert e.slab_count(4, 87600) == 512 and e.slab_count(36, 1457) == 56 and e.slab_count(36, 3) == 3 and e.slab_count(5000, 9) == 1
    assert [e.slab_bounds(10, 7, s) for s in range(7)] == [(0, 2), (2, 4), (4, 6), (6, 8), (8, 10), (10, 10), (10, 10)]
    assert e.count_lds_bytes(1, 16) == 135312 <= 160 * 1024  # 32 slots fit the LDS of a compute unit
    assert e.quantile_scratch_bytes(36, 9) == (36 * (4096 * 8 + 2 * 18 * 1024 * 8 + 8 + 18 * 16 + 4 + 4096) + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------------------------ the kernels' maps

@pytest.fixture(scope="module")
def host_quantile(tmp_path_factory):
    """a stand-alone program under the address and undefined-behaviour sanitizers; it is run directly, never loaded into Python"""
    return host_program.build(tmp_path_factory, "quantile", sanitize=True, timeout=300)


@pytest.mark.parametrize("n_rep,T,F,hw,slabs", [(2, 6, 2, 100, 6), (1, 13, 1, 256, 4), (3, 7, 4, 4, 3), (1, 5, 3, 4100, 2), (2, 10, 1, 8, 7)])
def test_every_value_is_counted_exactly_once(host_quantile, tmp_path, n_rep, T, F, hw, slabs):
    """workgroups that walk one plane (6 slabs over 6 planes), several planes (13 over 4: 4, 4, 4, 1), a ragged last one (7 over 3: 3, 3,
    1), a plane of more quads than threads (4100 values) and slabs that own nothing (10 planes over 7 slabs of 2).  The fields hold
    their own indices, so what was loaded says where from; the program itself checks that every table sums to n, that no later pass
    loads a value twice, and the minimum and maximum it selected."""
    subprocess.run([str(host_quantile), "visit", str(n_rep), str(T), str(F), str(hw), str(slabs), str(tmp_path / "ox.i32"), str(tmp_path / "oy.i32")],
                   check=True, timeout=300)
    ox, oy = np.fromfile(tmp_path / "ox.i32", dtype=np.int32), np.fromfile(tmp_path / "oy.i32", dtype=np.int32)
    want_x = np.broadcast_to((np.arange(n_rep)[:, None, None, None] * F + np.arange(F)[None, None, :, None]), (n_rep, T, F, hw))
    want_y = np.broadcast_to(n_rep * F + np.arange(F)[None, :, None], (T, F, hw))
    assert np.array_equal(ox.reshape(n_rep, T, F, hw), want_x) and np.array_equal(oy.reshape(T, F, hw), want_y)


@pytest.mark.parametrize("n_rep,T,F,hw,slabs", [(2, 3, 2, 64, 1), (1, 13, 1, 256, 5), (2, 37, 3, 8, 4)])
def test_select_phases_on_the_host_match_the_reference(host_quantile, tmp_path, n_rep, T, F, hw, slabs):
    """csrc/quantile_core.h compiled for the host: all phases of all three passes, every kind and level set, both NaN rules"""
    for kind in R.KINDS:
        for level_set in R.LEVEL_SETS:
            for skipna in (1, 0) if kind in ("nan", "allnan", "normal") else (1,):
                s, t, q, out, stats, nv = R.case(kind, n_rep, T, F, hw, level_set, True, bool(skipna))
                for name, a in (("x", s), ("y", t), ("q", q)):
                    a.tofile(tmp_path / name)
                subprocess.run([str(host_quantile), "select", str(n_rep), str(T), str(F), str(hw), "1", str(q.size), str(skipna), str(slabs)] +
                               [str(tmp_path / n) for n in ("x", "y", "q", "out", "stats", "nv")], check=True, timeout=300)
                assert R.same_numbers(np.fromfile(tmp_path / "out").reshape(out.shape), out), (kind, level_set, skipna)
                assert R.same_stats(np.fromfile(tmp_path / "stats", dtype=np.float32).reshape(stats.shape), stats), (kind, level_set, skipna)
                assert np.array_equal(np.fromfile(tmp_path / "nv", dtype=np.int64), nv)


# ------------------------------------------------------------------------------------------------------------------ C ABI

def test_new_entry_points_have_matching_argument_lists():
    names = {"c2w_quantile_supported": "int", "c2w_quantile_scratch_bytes": "long long", "c2w_quantiles": "int"}
    c_abi.assert_declared(names, "quantile.hip", c2w_ops, ("quantile_supported", "quantile_scratch_bytes", "quantiles"))
