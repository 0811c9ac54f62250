"""CPU checks of the quantile mapping (climate2weather_amd.biascorrect): the nodes against numpy.nanquantile / numpy.quantile as
numbers; the exact answers of the mapping -- identity, a shift per cell, a scale, the rank property, monotonicity; the bound inside
the range against numpy.interp; groups, the calendar, the state dict, the report and the argument checks -- on both routes, the general
float64 one and the launcher's, with tests/emu_qmap_ops.py standing in for the HIP kernels; the kernels' own maps and arithmetic
compiled for the host (csrc/qmap_core.h), once plain and once under the address and undefined-behaviour sanitizers; and the C
declarations against the ctypes prototypes."""
import os
import subprocess

import numpy as np
import pytest
import torch

import c_abi
import emu_qmap_ops
import fp64_qmap_ref as R
import host_program
from climate2weather_amd import biascorrect as BC
from climate2weather_amd import qmap_ops
from climate2weather_amd.ensemble_host import VariableReport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W_ = 2, 4
HW = H * W_


@pytest.fixture(params=["general", "launcher"])
def route(request, monkeypatch):
    """both branches of biascorrect on CPU tensors"""
    if request.param == "launcher":
        emu_qmap_ops.install(monkeypatch, qmap_ops, BC)
    return request.param


def t4(x):
    """(..., T, F, hw) array -> the (..., T, F, H, W) tensor of the public interface"""
    return torch.tensor(np.ascontiguousarray(x)).view(x.shape[:-1] + (H, W_))


def flat(t):
    return t.reshape(t.shape[:-2] + (HW,)).numpy() if t.dim() >= 2 else t.numpy()


# ------------------------------------------------------------------------------------------------------------------ nodes

@pytest.mark.parametrize("kind", R.KINDS)
def test_the_nodes_equal_numpy_as_numbers(route, kind):
    """K in {2, 9, 101, 128, 200} (200: beyond the kernel) and n in {1, 2, 3, 255, 257, 1025}; with NaNs skipped against
    numpy.nanquantile, without against numpy.quantile"""
    for n in (1, 2, 3, 255, 257, 1025):
        x = R.fields(kind, 1, n, 2, HW)
        for K in (2, 9, 101, 128, 200):
            for skipna in (True, False):
                want, nv = R.nodes64(x, [0] * n, 1, R.levels_of(K), skipna)
                q, cnt = BC.cell_quantiles(t4(x), K, skipna=skipna, return_counts=True)
                assert q.dtype == torch.float64 and tuple(q.shape) == (1, 1, 2, H, W_, K) and cnt.dtype == torch.int64
                got = q.numpy().reshape(1, 1, 2, HW, K)
                assert R.same_numbers(got, want), (kind, n, K, skipna)
                assert np.array_equal(cnt.numpy().reshape(1, 1, 2, HW), nv)
    if route == "launcher":
        assert ("nodes", HW, 128, 1025) in emu_qmap_ops.CALLS and not any(c[2] == 200 for c in emu_qmap_ops.CALLS if c[0] == "nodes")


def test_leading_members_and_explicit_levels(route):
    x = R.fields("temperature", 3, 40, 2, HW)
    levels = [0.0, 0.1, 0.5, 0.99, 1.0]
    want, _ = R.nodes64(x, [0] * 40, 1, levels)
    got = BC.cell_quantiles(t4(x), torch.tensor(levels, dtype=torch.float64))
    assert tuple(got.shape) == (3, 1, 2, H, W_, 5) and R.same_numbers(got.numpy().reshape(want.shape), want)
    one = BC.cell_quantiles(t4(x[1]), levels)
    assert R.same_bits(one.numpy(), got[1].numpy())


# ------------------------------------------------------------------------------------------------------------------ exact answers

@pytest.mark.parametrize("kind", R.EXACT_KINDS)
def test_a_model_mapped_onto_itself_is_the_identity_bit_for_bit(route, kind):
    m = R.fields(kind, 1, 257, 2, HW)[0]
    x = R.fields(kind, 2, 60, 2, HW, seed=1)
    centre = m.mean(axis=0, keepdims=True)
    x = (centre + 1.6 * (x - centre)).astype(np.float32)  # beyond the sample's range on both sides
    x[0, :m.shape[0] // 8] = m[::8][:x.shape[1]][:m.shape[0] // 8]  # and the nodes' own values
    qm = BC.QuantileMapping.fit(t4(m), t4(m))
    got = qm.apply(t4(x))
    assert got.dtype == torch.float32 and R.same_bits(got.numpy(), t4(x).numpy())
    assert (x > m.max(axis=0)).any() and (x < m.min(axis=0)).any()


def _integers(shape, seed, top=40):
    return np.random.default_rng(seed).integers(-top, top + 1, shape).astype(np.float32)


def test_a_shift_per_cell_on_small_integers_is_exact_everywhere(route):
    m = _integers((120, 2, HW), 0)
    c = _integers((1, 2, HW), 1, top=9)
    qm = BC.QuantileMapping.fit(t4(m), t4(m + c), levels=21)
    x = _integers((2, 50, 2, HW), 2, top=60)  # beyond the range too
    assert R.same_bits(qm.apply(t4(x)).numpy(), t4(x + c).numpy())


@pytest.mark.parametrize("kind", R.EXACT_KINDS)
def test_a_scale_gives_2x_inside_and_the_additive_tail_above(route, kind):
    m = R.fields(kind, 1, 129, 2, HW)[0]
    qm = BC.QuantileMapping.fit(t4(m), t4(2.0 * m), levels=33)
    x = R.fields(kind, 2, 80, 2, HW, seed=3)
    x[1, :40] = x[1, :40] + (m.max(axis=0) - m.min(axis=0))  # some above the top node
    got = flat(qm.apply(t4(x)))
    top, low = m.max(axis=0), m.min(axis=0)
    inside, above = (x >= low) & (x < top), x >= top
    assert inside.any() and above.any()
    assert np.array_equal(got[inside], (2.0 * x)[inside])
    tail = (x.astype(np.float64) + np.broadcast_to(top, x.shape).astype(np.float64)).astype(np.float32)  # x + (2 max - max)
    assert np.array_equal(got[above], tail[above])


@pytest.mark.parametrize("K", [33, 65])
def test_the_rank_property(route, K):
    """n_h = n_r = K without ties: the levels k / (K - 1) are exact, every node is an order statistic, and the mapped historical
    series is the reference's values in the model's order"""
    rng = np.random.default_rng(K)
    m = np.stack([rng.permutation(K * 3)[:K] for _ in range(2 * HW)], axis=1).reshape(K, 2, HW).astype(np.float32) * 0.37 + 280.0
    r = np.stack([rng.permutation(K * 5)[:K] for _ in range(2 * HW)], axis=1).reshape(K, 2, HW).astype(np.float32) * 0.61 + 270.0
    qm = BC.QuantileMapping.fit(t4(m), t4(r), levels=K)
    got = flat(qm.apply(t4(m)))
    assert R.same_bits(np.sort(got, axis=0), np.sort(r, axis=0))
    assert R.same_bits(got, np.take_along_axis(np.sort(r, axis=0), np.argsort(np.argsort(m, axis=0), axis=0), axis=0))


@pytest.mark.parametrize("kind", ["temperature", "ties", "wind"])
def test_sorted_input_gives_non_decreasing_output(route, kind):
    """repeated nodes included ("ties": a handful of distinct values); the nodes' own values and their fp32 neighbours are among x"""
    m, r = R.fields(kind, 1, 100, 2, HW)[0], R.fields("temperature", 1, 77, 2, HW, seed=5)[0]
    qm = BC.QuantileMapping.fit(t4(m), t4(r), levels=17)
    nodes = qm.xq.numpy().reshape(2, HW, 17).astype(np.float32)                       # (F, hw, K)
    near = np.concatenate([nodes, np.nextafter(nodes, np.float32(np.inf)), np.nextafter(nodes, np.float32(-np.inf))], axis=-1)
    x = np.concatenate([np.moveaxis(near, -1, 0), R.fields(kind, 1, 300, 2, HW, seed=6)[0] * 1.3], axis=0)
    x = np.sort(x, axis=0)
    got = flat(qm.apply(t4(x)))
    assert np.all(np.diff(got, axis=0) >= 0)


@pytest.mark.parametrize("kind", R.EXACT_KINDS)
@pytest.mark.parametrize("K", [9, 101])
def test_inside_the_range_the_mapping_is_numpy_interp_within_the_bound(route, kind, K):
    m, r = R.fields(kind, 1, 257, 2, HW)[0], R.fields(kind, 1, 301, 2, HW, seed=7)[0] * 1.1 + 0.5
    qm = BC.QuantileMapping.fit(t4(m), t4(r.astype(np.float32)), levels=K)
    xq, yq = qm.xq.numpy().reshape(1, 2, HW, K), qm.yq.numpy().reshape(1, 2, HW, K)
    assert np.all(np.diff(xq, axis=-1) > 0)  # strictly increasing nodes
    x = R.fields(kind, 2, 90, 2, HW, seed=8)
    got = flat(qm.apply(t4(x))).astype(np.float64)
    want, allow = R.interp64(x, xq, yq, [0] * 90)
    inside = ~np.isnan(want)
    frac = np.abs(got - want)[inside] / allow[inside]
    print(f"{kind} K {K} {route}: worst fraction of the bound {frac.max():.3g} over {int(inside.sum())} values")
    assert inside.sum() > x.size // 2 and np.all(frac <= 1.0)
    below, above, tail = R.tails64(x, xq, yq, [0] * 90)
    assert np.array_equal(flat(qm.apply(t4(x)))[below | above], tail[below | above])


# ------------------------------------------------------------------------------------------------------------------ groups

def test_three_uneven_groups_one_empty_equal_three_separate_fits(route):
    T, Tr = 50, 41
    ids = np.array([0] * 7 + [2] * 30 + [0] * 13)            # group 1 is empty in the model ...
    ids_r = np.array([2] * 20 + [0] * 20 + [1])               # ... and has one time in the reference
    m, r = R.fields("temperature", 1, T, 2, HW)[0], R.fields("pressure", 1, Tr, 2, HW)[0]
    qm = BC.QuantileMapping.fit(t4(m), t4(r), levels=11, model_groups=torch.tensor(ids), reference_groups=torch.tensor(ids_r), n_groups=3)
    assert qm.n_groups == 3 and tuple(qm.xq.shape) == (3, 2, H, W_, 11)
    assert qm.n_valid_model[:, 0, 0, 0].tolist() == [20, 0, 30] and qm.n_valid_reference[:, 0, 0, 0].tolist() == [20, 1, 20]
    assert torch.isnan(qm.xq[1]).all() and torch.isnan(qm.yq[1]).all()  # a NaN row in one table is a NaN row in both
    x = R.fields("temperature", 2, 30, 2, HW, seed=9)
    xid = np.array([0, 1, 2] * 10)
    got = qm.apply(t4(x), torch.tensor(xid))
    for g in (0, 2):
        alone = BC.QuantileMapping.fit(t4(m[ids == g]), t4(r[ids_r == g]), levels=11)
        assert R.same_bits(alone.xq.numpy(), qm.xq[g:g + 1].numpy()) and R.same_bits(alone.yq.numpy(), qm.yq[g:g + 1].numpy())
        assert R.same_bits(alone.apply(t4(x[:, xid == g])).numpy(), got[:, xid == g].numpy())
    nan = torch.isnan(got)
    assert nan[:, xid == 1].all() and not nan[:, xid != 1].any()  # a time in the empty group maps to NaN; nothing else is NaN


def test_calendar_groups_across_a_year_end_and_a_leap_day():
    g = BC.calendar_groups("2019-12-31-22", 5)
    assert g.dtype == torch.int64 and g.tolist() == [11, 11, 0, 0, 0]
    assert BC.calendar_groups("2020-02-28-00", 4, step_hours=24).tolist() == [1, 1, 2, 2]      # 28, 29 February, 1, 2 March
    assert BC.calendar_groups("2021-02-28-00", 3, step_hours=24).tolist() == [1, 2, 2]         # no leap day
    assert BC.calendar_groups("2019-11-30-12", 4, step_hours=12, by="season").tolist() == [3, 0, 0, 0]  # SON -> DJF
    assert BC.calendar_groups("2020-02-29-23", 2, by="season").tolist() == [0, 1]              # DJF -> MAM
    assert BC.calendar_groups("2020-01-01-00", 3, by=None).tolist() == [0, 0, 0]
    year = BC.calendar_groups("2020-01-01-00", 8784)
    assert [int((year == k).sum()) // 24 for k in range(12)] == [31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]
    with pytest.raises(ValueError):
        BC.calendar_groups("2020-01-01-00", 3, by="week")
    with pytest.raises(ValueError):
        BC.calendar_groups("2020-01-01", 3)


def test_a_state_dict_round_trip_keeps_every_bit(route):
    m, r = R.fields("nans", 1, 60, 2, HW)[0], R.fields("wind", 1, 45, 2, HW)[0]
    ids = torch.tensor([0, 1] * 30)
    qm = BC.QuantileMapping.fit(t4(m), t4(r), levels=9, model_groups=ids, reference_groups=ids[:45])
    state = qm.state_dict()
    assert set(state) == {"levels", "xq", "yq", "n_valid_model", "n_valid_reference"}
    assert state["xq"].dtype == state["yq"].dtype == state["levels"].dtype == torch.float64 and state["n_valid_model"].dtype == torch.int64
    back = BC.QuantileMapping.from_state_dict({k: v.clone() for k, v in state.items()}).to("cpu")
    for k, v in back.state_dict().items():
        assert R.same_bits(v.numpy(), state[k].numpy()), k
    x = R.fields("nans", 2, 60, 2, HW, seed=4)
    a, b = qm.apply(t4(x), ids), back.apply(t4(x), ids)
    assert R.same_bits(a.numpy(), b.numpy())
    assert torch.equal(torch.isnan(a), torch.isnan(t4(x)))  # a NaN x gives NaN, and nothing else does


def test_the_bias_report_shrinks_the_bias_at_every_level(route):
    r = np.concatenate([R.fields("temperature", 1, 400, 1, HW)[0], R.fields("wind", 1, 400, 1, HW)[0]], axis=1)
    z = np.concatenate([R.fields("temperature", 1, 500, 1, HW, seed=2)[0], R.fields("wind", 1, 500, 1, HW, seed=2)[0]], axis=1)
    m = (1.3 * z + np.array([2.5, 1.0], np.float32).reshape(1, 2, 1)).astype(np.float32)  # shifted and scaled
    qm = BC.QuantileMapping.fit(t4(m), t4(r))
    rep = BC.bias_report(t4(m), t4(r), qm, names=["tas", "sfcWind"])
    assert isinstance(rep, VariableReport) and rep.names == ["tas", "sfcWind"] and len(rep.levels) == 9
    for name, v in rep:
        assert set(v) == {"reference", "before", "after", "bias_before", "bias_after"} and v["after"].dtype == torch.float64
        assert torch.all(v["bias_after"].abs() < v["bias_before"].abs()), (name, v["bias_before"], v["bias_after"])


# ------------------------------------------------------------------------------------------------------------------ interface

def test_in_place_any_dtype_any_strides(route):
    m, r = R.fields("temperature", 1, 64, 2, HW)[0], R.fields("temperature", 1, 64, 2, HW, seed=3)[0] + 2.0
    qm = BC.QuantileMapping.fit(t4(m), t4(r.astype(np.float32)), levels=11)
    x = t4(R.fields("temperature", 2, 20, 2, HW, seed=4))
    want = qm.apply(x)
    buf = x.clone()
    assert qm.apply(buf, out=buf) is buf and torch.equal(buf, want)
    wide = torch.zeros(2, 20, 2, H, 2 * W_)
    wide[..., ::2] = x
    assert torch.equal(qm.apply(wide[..., ::2]), want)
    half = x.to(torch.bfloat16)
    assert torch.equal(qm.apply(half), qm.apply(half.float()))
    assert torch.equal(BC.cell_quantiles(half, 5), BC.cell_quantiles(half.float(), 5))


def test_argument_checks(route):
    x = t4(R.fields("temperature", 1, 12, 2, HW)[0])
    bad_levels = (1, [0.5], [0.0, 1.5], [0.0, float("nan"), 1.0], [0.0, 0.5, 0.5, 1.0], [1.0, 0.0])
    for levels in bad_levels:
        with pytest.raises(ValueError):
            BC.cell_quantiles(x, levels)
    for groups, n_groups in ((torch.tensor([0] * 11 + [3]), 3), (torch.tensor([0] * 11 + [-1]), None), (torch.zeros(12), None),
                             (torch.zeros(11, dtype=torch.int64), None)):
        with pytest.raises(ValueError):
            BC.cell_quantiles(x, 5, groups=groups, n_groups=n_groups)
        with pytest.raises(ValueError):
            BC.QuantileMapping.fit(x, x, levels=5, reference_groups=groups, n_groups=n_groups)
    assert emu_qmap_ops.CALLS == [] or route == "general"  # nothing was launched before the error
    with pytest.raises(ValueError):
        BC.QuantileMapping.fit(x, x[:, :1])
    with pytest.raises(ValueError):
        BC.cell_quantiles(x.long(), 5)
    ids = torch.tensor([0, 1] * 6)
    qm = BC.QuantileMapping.fit(x, x, levels=5, model_groups=ids, reference_groups=ids)
    for call in (lambda: qm.apply(x), lambda: qm.apply(x, torch.tensor([0, 2] * 6)), lambda: qm.apply(x[:, :1], ids),
                 lambda: qm.apply(x, ids, out=torch.empty(12, 2, H, W_, dtype=torch.float64))):
        with pytest.raises(ValueError):
            call()


def test_unsupported_shapes_take_the_general_route(monkeypatch):
    """hw no multiple of 4, K = 129 and a group of 16 385 times: the launcher is asked, answers no, nothing is launched, and the
    general route answers"""
    emu_qmap_ops.install(monkeypatch, qmap_ops, BC)
    x6 = R.fields("wind", 1, 30, 2, 6)
    got = BC.cell_quantiles(torch.tensor(x6).view(1, 30, 2, 2, 3), 9)
    assert R.same_numbers(got.numpy().reshape(1, 1, 2, 6, 9), R.nodes64(x6, [0] * 30, 1, R.levels_of(9))[0])
    x = R.fields("wind", 1, 30, 2, HW)
    assert R.same_numbers(BC.cell_quantiles(t4(x), 129).numpy().reshape(1, 1, 2, HW, 129), R.nodes64(x, [0] * 30, 1, R.levels_of(129))[0])
    long_ = R.fields("temperature", 1, 16385, 1, 4)
    got = BC.cell_quantiles(torch.tensor(long_).view(1, 16385, 1, 2, 2), 5)
    assert R.same_numbers(got.numpy().reshape(1, 1, 1, 4, 5), R.nodes64(long_, [0] * 16385, 1, R.levels_of(5))[0])
    qm = BC.QuantileMapping.fit(torch.tensor(x6[0]).view(30, 2, 2, 3), torch.tensor(x6[0]).view(30, 2, 2, 3), levels=9)
    assert torch.equal(qm.apply(torch.tensor(x6).view(1, 30, 2, 2, 3)), torch.tensor(x6).view(1, 30, 2, 2, 3))
    assert emu_qmap_ops.CALLS == []  # qmap_supported said no before anything was allocated
    for hw, K, n in ((6, 9, 30), (8, 129, 30), (8, 9, 16385), (8, 1, 30)):
        assert not emu_qmap_ops.qmap_nodes(*([None] * 7), 1, n, 2, hw, n, 1, K, n, True, 0, 4)
        assert not emu_qmap_ops.qmap_apply(*([None] * 6), 1, n, 2, hw, n, 1, K, n)


def test_the_general_route_is_the_same_in_every_chunking(monkeypatch):
    m, r = R.fields("nans", 1, 33, 2, HW)[0], R.fields("pressure", 1, 29, 2, HW)[0]
    x, ids = t4(R.fields("nans", 2, 33, 2, HW, seed=1)), torch.tensor([0, 1, 2] * 11)
    whole = BC.QuantileMapping.fit(t4(m), t4(r), levels=7, model_groups=ids, reference_groups=ids[:29])
    for elems in (1, 3 * 2 * HW * 7):
        monkeypatch.setattr(BC, "chunk_step", lambda per_item, n=elems: max(1, n // max(1, per_item)))
        part = BC.QuantileMapping.fit(t4(m), t4(r), levels=7, model_groups=ids, reference_groups=ids[:29])
        assert R.same_bits(part.xq.numpy(), whole.xq.numpy()) and R.same_bits(part.yq.numpy(), whole.yq.numpy())
        assert R.same_bits(part.apply(x, ids).numpy(), whole.apply(x, ids).numpy())


def test_both_routes_give_the_same_bits(monkeypatch):
    """every kind, groups, members: the launcher's route (the restated kernels) against the general float64 route"""
    ids = torch.tensor(([0] * 5 + [1] * 3 + [3] * 9) * 3)
    for kind in R.KINDS:
        m, r = R.fields(kind, 1, 51, 2, HW)[0], R.fields(kind, 1, 51, 2, HW, seed=1)[0]
        x = t4(R.fields(kind, 2, 51, 2, HW, seed=2))
        with monkeypatch.context() as mp:
            emu_qmap_ops.install(mp, qmap_ops, BC)
            a = BC.QuantileMapping.fit(t4(m), t4(r), levels=13, model_groups=ids, reference_groups=ids)
            ya = a.apply(x, ids)
            assert [c[0] for c in emu_qmap_ops.CALLS] == ["nodes", "nodes", "apply"]
        b = BC.QuantileMapping.fit(t4(m), t4(r), levels=13, model_groups=ids, reference_groups=ids)
        assert R.same_numbers(a.xq.numpy(), b.xq.numpy()) and R.same_numbers(a.yq.numpy(), b.yq.numpy()), kind
        assert R.same_numbers(ya.numpy(), b.apply(x, ids).numpy()), kind
        if kind not in ("inf", "nans"):
            assert not torch.isnan(ya[:, ids != 2]).any()
        assert torch.isnan(ya[:, ids == 2]).all() if (ids == 2).any() else True


# ------------------------------------------------------------------------------------------------------------------ the kernels' maps

@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_qmap(request, tmp_path_factory):
    """a stand-alone program, once plain and once under the address and undefined-behaviour sanitizers; it is run directly, never loaded
    into Python.  -ffp-contract=off: the kernel fuses no multiply with an add either (qmap_core.h says so to its own compiler)."""
    return host_program.build(tmp_path_factory, "qmap", sanitize=request.param == "sanitized", fp_contract_off=True, timeout=600)


def _lists(ids, G):
    idx = R.index_lists(ids, G)
    tidx = np.array([t for i in idx for t in i], np.int32)
    goff = np.cumsum([0] + [len(i) for i in idx]).astype(np.int32)
    return tidx, goff


@pytest.mark.parametrize("hw,T,G,K,block", [(4, 1, 1, 2, 64), (8, 3, 1, 9, 64), (68, 130, 3, 101, 64), (132, 257, 2, 128, 128), (8, 1100, 2, 5, 4)])
def test_the_host_program_equals_the_emulation_bit_for_bit(host_qmap, tmp_path, hw, T, G, K, block):
    """csrc/qmap_core.h compiled for the host against tests/emu_qmap_ops.py: the gather tiles (a tile and 4 cells, two tiles of
    positions and 2), the cell blocks, the sort (N from 2 to 2048, 256 and 1024 threads), the count, the interpolation; then the
    apply in place -- cell blocks of 64 and 32, partial ones, one slab and three, every element taken up exactly once.  Every kind."""
    n_rep, F = 2, 2
    rng = np.random.default_rng(hw + T)
    ids = np.sort(rng.integers(0, G, T)) if G < 3 else np.where(np.arange(T) % 3 == 0, 0, 2)  # G = 3: group 1 is empty
    tidx, goff = _lists(ids.tolist(), G)
    max_len = int(np.diff(goff).max())
    levels = R.levels_of(K)
    tidx.tofile(tmp_path / "tidx"), goff.tofile(tmp_path / "goff"), levels.tofile(tmp_path / "levels")
    files = [str(tmp_path / n) for n in ("x", "tidx", "goff", "levels", "q", "nvalid")]
    for kind in R.KINDS:
        x = R.fields(kind, n_rep, T, F, hw)
        x.tofile(tmp_path / "x")
        for skipna in (1, 0):
            q = torch.full((n_rep, G, F, hw, K), -7.25, dtype=torch.float64)
            nv = torch.full((n_rep, G, F, hw), -7, dtype=torch.int64)
            ws = torch.empty(emu_qmap_ops.qmap_scratch_bytes(n_rep * F, hw, T) // 4, dtype=torch.float32)
            assert emu_qmap_ops.qmap_nodes(torch.tensor(x), torch.tensor(tidx), torch.tensor(goff), torch.tensor(levels), q, nv, ws, n_rep, T, F, hw,
                                           T, G, K, max_len, bool(skipna), 0, hw)
            subprocess.run([str(host_qmap), "nodes"] + [str(a) for a in (n_rep, T, F, hw, G, K, skipna, block)] + files, check=True, timeout=600)
            got = np.fromfile(tmp_path / "q", dtype=np.float64).reshape(q.shape)
            assert R.same_numbers(got, q.numpy()) and R.same_bits(got[~np.isnan(got)], q.numpy()[~np.isnan(got)]), (kind, skipna)
            assert np.array_equal(np.fromfile(tmp_path / "nvalid", dtype=np.int64).reshape(nv.shape), nv.numpy())
        # the tables a fit would hand over: a row with a NaN node is NaN in both
        xq = q.numpy().copy()
        yq = np.roll(xq, 1, axis=2) * 1.5 + 1.0 if kind not in ("inf", "nans") else xq.copy()
        bad = (np.isnan(xq).any(-1) | np.isnan(yq).any(-1))[..., None]
        xq, yq = np.where(bad, np.nan, xq)[0], np.where(bad, np.nan, yq)[0]
        xq.tofile(tmp_path / "xq"), yq.tofile(tmp_path / "yq")
        xv = R.fields(kind, n_rep, T, F, hw, seed=1)
        xv.tofile(tmp_path / "xv")
        out = torch.empty((n_rep, T, F, hw), dtype=torch.float32)
        assert emu_qmap_ops.qmap_apply(torch.tensor(xv), out, torch.tensor(xq), torch.tensor(yq), torch.tensor(tidx), torch.tensor(goff), n_rep, T, F,
                                       hw, T, G, K, max_len)
        for slabs in (1, 3):
            subprocess.run([str(host_qmap), "apply"] + [str(a) for a in (n_rep, T, F, hw, G, K, slabs)] +
                           [str(tmp_path / n) for n in ("xv", "xq", "yq", "tidx", "goff", "out")], check=True, timeout=600)
            got = np.fromfile(tmp_path / "out", dtype=np.float32).reshape(out.shape)
            assert R.same_numbers(got, out.numpy()) and R.same_bits(got[~np.isnan(got)], out.numpy()[~np.isnan(got)]), (kind, slabs)


def test_support_predicates_and_maps_agree():
    for hw, K, n, want in ((4, 2, 0, True), (16384, 128, 16384, True), (6, 9, 10, False), (64, 129, 10, False), (64, 1, 10, False), (64, 9, 16385, False),
                           (0, 9, 10, False)):
        assert emu_qmap_ops.qmap_supported(hw, K, n) is want
    core = open(os.path.join(ROOT, "climate2weather_amd", "csrc", "qmap_core.h")).read()
    for text in ("MAX_K = 128", "MAX_N = 16384", "TILE = 64", "TOP = 0xFFFFFFFFu",
                 "hw >= 4 && hw % 4 == 0 && K >= 2 && K <= MAX_K && max_len >= 0 && max_len <= MAX_N"):
        assert text in core, text
    assert BC.GATHER_TILE == 64
    assert emu_qmap_ops.qmap_scratch_bytes(8, 64, 100) == 8 * 64 * 100 * 4 and emu_qmap_ops.qmap_scratch_bytes(1, 1, 1) == 16
    # the monotone key: the order of the values, -0.0 just below +0.0, denormals kept
    v = np.array([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf], np.float32)
    keys = emu_qmap_ops.key_of(v.view(np.uint32))
    assert np.all(np.diff(keys.astype(np.int64)) > 0) and R.same_bits(emu_qmap_ops.bits_of(keys).view(np.float32), v)


# ------------------------------------------------------------------------------------------------------------------ C ABI

def test_new_entry_points_have_matching_argument_lists():
    names = {"c2w_qmap_supported": "int", "c2w_qmap_scratch_bytes": "long long", "c2w_qmap_nodes": "int", "c2w_qmap_apply": "int"}
    c_abi.assert_declared(names, "qmap.hip", qmap_ops, ("qmap_supported", "qmap_scratch_bytes", "qmap_nodes", "qmap_apply"))
