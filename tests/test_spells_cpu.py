"""CPU checks of the event spells (climate2weather_amd.spells): both routes of an update -- the general torch one and the launcher's,
with tests/emu_spell_ops.py standing in for the HIP kernel -- EQUAL to the NumPy reference of tests/fp64_spells_ref.py on every kind of
field; block splitting, also across a saved state; the known answers, all exact -- a periodic event, an all-event series, an
alternating one, time reversed, a NaN inside a spell; the identities between the tables and against events.event_counts; the algebra
on a hand-made table; every ValueError; the launcher declining what the kernel does not take; the kernel's own index maps and
arithmetic compiled for the host (csrc/spells_core.h), once plain and once under the address and undefined-behaviour sanitizers; and
the C declarations against the ctypes prototypes."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import c_abi
import emu_spell_ops
import fp64_spells_ref as R
import host_program
from climate2weather_amd import events as EV
from climate2weather_amd import spell_ops
from climate2weather_amd import spells as SP
from climate2weather_amd.ensemble_host import VariableReport

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=["general", "launcher"])
def route(request, monkeypatch):
    """both branches of SpellAccumulator.update on CPU tensors"""
    if request.param == "launcher":
        emu_spell_ops.install(monkeypatch, spell_ops, SP)
    return request.param


def _case(kind, M, T, F, H, W_, K, direction="mixed", seed=0):
    """the arrays of the reference and the tensors of the public interface"""
    x, y = R.fields(kind, M, T, F, H * W_, seed)
    thr, above = R.thresholds(kind, y, K), R.directions(F, K, direction)
    return x, y, thr, above, torch.tensor(x).view(M, T, F, H, W_), torch.tensor(y).view(T, F, H, W_), torch.tensor(thr), R.direction_names(above)


def _assert_equal_ref(t, want, what=""):
    D, F, K = want["censored"].shape
    assert t.hist.dtype == torch.int64 and t.onsets.dtype == torch.int64 and t.invalid.dtype == torch.int64 and t.censored.dtype == torch.int64
    assert t.hours.dtype == torch.int32 and t.count.dtype == torch.int32 and t.longest.dtype == torch.int32
    for name in ("hist", "onsets", "invalid", "censored"):
        assert np.array_equal(getattr(t, name).cpu().numpy(), want[name]), (name, what)
    for name in ("hours", "count", "longest"):
        got = getattr(t, name)
        assert got.dim() == 5 and np.array_equal(got.cpu().numpy().reshape(D, F, K, -1), want[name]), (name, what)


def _assert_same_tables(a, b, what=""):
    assert a.n_times == b.n_times, what
    for name in ("hist", "hours", "count", "longest", "onsets", "invalid", "censored"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (name, what)


def _series(rows):
    """rows: D lists of 0 / 1 over time -> samples (D - 1, T, 1, 1, 4), truth (T, 1, 1, 4) fp32 with the event at values >= 1, every one of
    the 4 cells the same series"""
    v = torch.tensor(rows, dtype=torch.float32)[:, :, None, None, None].expand(-1, -1, 1, 1, 4).contiguous()
    return v[1:], v[0]


ONE = torch.tensor([[1.0]])


# ------------------------------------------------------------------------------------------------------------------ against the reference

@pytest.mark.parametrize("H,W_,M,T,K,Lmax,period,t0", [(1, 4, 1, 1, 1, 1, 0, 0), (2, 6, 3, 9, 2, 3, 6, 5), (41, 100, 2, 33, 5, 48, 24, 7),
                                                        (8, 8, 2, 17, 8, 256, 1, 0)])
def test_the_tables_equal_the_reference(route, H, W_, M, T, K, Lmax, period, t0):
    """hw = 4, 12 (no multiple of 4 in W alone), 4100 (five chunks, the last of one thread) and 64; one and two threshold groups; with
    and without a truth; mixed directions; the kinds taking turns"""
    kinds = R.KINDS if H * W_ < 1000 else R.KINDS[::4]
    for i, kind in enumerate(kinds):
        with_truth = i % 2 == 0
        x, y, thr, above, S, Tr, th, names = _case(kind, M, T, 2, H, W_, K, ("mixed", "above", "below")[i % 3])
        t = SP.spell_tables(S, Tr if with_truth else None, th, names, Lmax, period, t0)
        assert t.n_times == T and t.hist.shape == (M + with_truth, 2, K, Lmax) and t.onsets.shape == (M + with_truth, 2, K, period)
        _assert_equal_ref(t, R.spells_ref(x, y if with_truth else None, thr, above, Lmax, period, t0), kind)
    if route == "launcher":
        assert len(emu_spell_ops.CALLS) == len(kinds) and emu_spell_ops.CALLS[0][:5] == (M, T, 2, H * W_, K)


def test_the_general_route_chunked_over_time_gives_the_same_tables(monkeypatch):
    monkeypatch.setattr(SP, "chunk_step", lambda per_item: 2)  # 9 times in chunks of 2: the last chunk is short, spells cross the chunks
    for kind in ("smooth", "nans", "alternating"):
        x, y, thr, above, S, Tr, th, names = _case(kind, 2, 9, 2, 2, 6, 3)
        _assert_equal_ref(SP.spell_tables(S, Tr, th, names, 4, 6, 3), R.spells_ref(x, y, thr, above, 4, 6, 3), kind)


# ------------------------------------------------------------------------------------------------------------------ block splitting

@pytest.mark.parametrize("kind", ["smooth", "nans", "periodic"])
def test_block_splitting_gives_identical_tables(route, kind):
    """T = 17 as one block, as seventeen blocks of 1, as (8, 9) and as (5, 0, 12): the smooth field's spells are long, so the splits fall
    inside them; the same across state_dict / load_state_dict; tables() in between changes nothing"""
    M, T, F, H, W_, K, Lmax, period, t0 = 2, 17, 2, 2, 6, 3, 5, 6, 5
    x, y, thr, above, S, Tr, th, names = _case(kind, M, T, F, H, W_, K)
    want = R.spells_ref(x, y, thr, above, Lmax, period, t0)
    make = lambda: SP.SpellAccumulator(M, F, H, W_, th, names, max_duration=Lmax, period=period, t0=t0)
    whole = make().update(S, Tr).tables()
    _assert_equal_ref(whole, want, kind)
    for sizes in ((1,) * 17, (8, 9), (5, 0, 12)):
        acc, at = make(), 0
        for n in sizes:
            acc.update(S[:, at:at + n], Tr[at:at + n])
            acc.tables()
            at += n
        _assert_same_tables(acc.tables(), whole, sizes)
    first = make().update(S[:, :8], Tr[:8])
    saved = first.state_dict()
    first.update(S[:, 8:], Tr[8:])                      # the saved state is a copy: going on does not change it
    resumed = make().load_state_dict(saved).update(S[:, 8:], Tr[8:])
    _assert_same_tables(resumed.tables(), whole, "resumed")
    _assert_same_tables(first.tables(), whole, "went on")
    _assert_equal_ref(make().load_state_dict(saved).tables(), R.spells_ref(x[:, :8], y[:8], thr, above, Lmax, period, t0), "the first 8")


# ------------------------------------------------------------------------------------------------------------------ known answers

@pytest.mark.parametrize("a,p,n", [(2, 6, 4), (1, 3, 5), (5, 6, 2)])
def test_an_event_for_a_of_every_p_hours(route, a, p, n):
    row = [1 if t % p < a else 0 for t in range(n * p)]
    S, Tr = _series([row, row])
    t = SP.spell_tables(S, Tr, ONE, max_duration=8, period=p)
    hist = [0] * 8
    hist[a - 1] = 4 * n
    onsets = [4 * n] + [0] * (p - 1)
    for d in range(2):
        assert t.hist[d, 0, 0].tolist() == hist and t.onsets[d, 0, 0].tolist() == onsets
        assert t.hours[d].flatten().tolist() == [n * a] * 4 and t.longest[d].flatten().tolist() == [a] * 4 and t.count[d].flatten().tolist() == [n] * 4
    assert t.censored.flatten().tolist() == [4, 4] and int(t.invalid.sum()) == 0  # the first spell touches the first time


@pytest.mark.parametrize("T,Lmax", [(5, 48), (48, 48), (7, 3), (1, 1)])
def test_an_all_event_series_is_one_spell_of_T(route, T, Lmax):
    S, Tr = _series([[1] * T, [1] * T])
    acc = SP.SpellAccumulator(1, 1, 1, 4, ONE, max_duration=Lmax, period=4, t0=6)
    t = acc.update(S, Tr).tables()
    hist = [0] * Lmax
    hist[min(T, Lmax) - 1] = 4
    assert t.hist[0, 0, 0].tolist() == hist and t.hist[1, 0, 0].tolist() == hist and (t.hist[0, 0, 0, -1].item() == 4) == (T >= Lmax)
    assert t.count.flatten().tolist() == [1] * 8 and t.longest.flatten().tolist() == [T] * 8 and t.hours.flatten().tolist() == [T] * 8
    assert t.censored.flatten().tolist() == [4, 4] and t.onsets[0, 0, 0].tolist() == [0, 0, 4, 0]  # one onset, at (6 + 0) mod 4
    assert int(acc.hist.sum()) == 0  # the kernel closes no run at a block's end: the spell is in the state alone


def test_an_alternating_series_of_odd_length(route):
    T = 9
    S, Tr = _series([[1 - t % 2 for t in range(T)], [t % 2 for t in range(T)]])
    t = SP.spell_tables(S, Tr, ONE, max_duration=3, period=2)
    assert t.hist[0, 0, 0].tolist() == [4 * (T + 1) // 2, 0, 0] and t.hist[1, 0, 0].tolist() == [4 * (T - 1) // 2, 0, 0]
    assert t.count[0].flatten().tolist() == [(T + 1) // 2] * 4 and t.longest.flatten().tolist() == [1] * 8
    assert t.onsets[0, 0, 0].tolist() == [20, 0] and t.onsets[1, 0, 0].tolist() == [0, 16]
    assert t.censored.flatten().tolist() == [8, 0]  # the truth's first and last spells; the member's touch neither end


def test_reversing_time_leaves_the_duration_tables_unchanged(route):
    for kind in ("smooth", "nans", "infinities"):
        x, y, thr, above, S, Tr, th, names = _case(kind, 2, 13, 2, 2, 4, 2)
        a, b = SP.spell_tables(S, Tr, th, names, 6), SP.spell_tables(S.flip(1), Tr.flip(0), th, names, 6)
        for name in ("hist", "hours", "count", "longest", "invalid", "censored"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (kind, name)


def test_a_nan_inside_a_spell_ends_it_and_is_counted(route):
    row = [0, 1, 1, float("nan"), 1, 1, 0]
    S, Tr = _series([[0, 1, 1, 1, 1, 1, 0], row])
    t = SP.spell_tables(S, Tr, ONE, max_duration=6)
    assert t.hist[0, 0, 0].tolist() == [0, 0, 0, 0, 4, 0] and t.hist[1, 0, 0].tolist() == [0, 8, 0, 0, 0, 0]
    assert t.invalid.tolist() == [[0], [4]] and t.count[1].flatten().tolist() == [2] * 4 and t.longest[1].flatten().tolist() == [2] * 4
    assert t.hours[1].flatten().tolist() == [4] * 4 and t.censored.flatten().tolist() == [0, 0]
    below = SP.spell_tables(S, Tr, ONE, "below", max_duration=6)  # a NaN is no event in either direction
    assert below.hist[1, 0, 0].tolist() == [0, 0, 8, 0, 0, 0] and below.invalid.tolist() == [[0], [4]]  # 0 1 1 | 1 1 0 are all <= 1


# ------------------------------------------------------------------------------------------------------------------ identities

def test_the_tables_agree_with_each_other_and_with_the_event_counts(route):
    for kind, Lmax in (("smooth", 64), ("periodic", 64), ("pressure", 64), ("ties", 64)):
        M, T, F, H, W_, K = 3, 21, 2, 2, 8, 3
        x, y, thr, above, S, Tr, th, names = _case(kind, M, T, F, H, W_, K)
        t = SP.spell_tables(S, Tr, th, names, Lmax, 6, 2)
        cells = (-1, -2)
        assert torch.equal(t.hist.sum(dim=-1), t.count.sum(dim=cells, dtype=torch.int64))
        assert int(t.hist[..., -1].sum()) == 0  # T < Lmax: the last bin is empty, so the bins give the hours
        assert torch.equal((t.hist * torch.arange(1, Lmax + 1)).sum(dim=-1), t.hours.sum(dim=cells, dtype=torch.int64))
        assert torch.equal(t.onsets.sum(dim=-1), t.count.sum(dim=cells, dtype=torch.int64))
        counts, invalid = EV.event_counts(S, Tr, th, names)                      # (T, F, K, 2, M + 1)
        assert int(invalid.sum()) == 0 and int(t.invalid.sum()) == 0
        hours = t.hours.sum(dim=cells, dtype=torch.int64)
        assert torch.equal(hours[0], counts[:, :, :, 1, :].sum(dim=(0, -1)))
        assert torch.equal(hours[1:].sum(dim=0), (counts * torch.arange(M + 1)).sum(dim=(0, -1, -2)))


# ------------------------------------------------------------------------------------------------------------------ the algebra

def test_the_algebra_on_a_hand_made_table():
    hist = torch.tensor([[[[2, 1, 0, 1]]], [[[0, 2, 2, 0]]], [[[0, 0, 0, 0]]]])               # (D, F, K, Lmax) = (3, 1, 1, 4)
    pmf = SP.duration_pmf(hist)
    assert pmf[0, 0, 0].tolist() == [0.5, 0.25, 0.0, 0.25] and pmf[1, 0, 0].tolist() == [0.0, 0.5, 0.5, 0.0] and torch.isnan(pmf[2]).all()
    assert SP.survival(hist)[0, 0, 0].tolist() == [1.0, 0.5, 0.25, 0.25] and SP.survival(hist)[1, 0, 0].tolist() == [1.0, 1.0, 0.5, 0.0]
    dist = SP.spell_duration_distance(hist)                                                    # CDFs (.5, .75, .75) and (0, .5, 1)
    assert dist.shape == (2, 1, 1) and dist[0, 0, 0].item() == 0.5 + 0.25 + 0.25 and math.isnan(dist[1, 0, 0].item())
    assert SP.spell_duration_distance(hist[None, None]).shape == (1, 1, 2, 1, 1)               # any leading shape
    # spells of 1, 2 and 9 hours at Lmax = 4: the last bin is populated and the mean is still exact
    hours, count = torch.tensor([[3, 9]], dtype=torch.int32), torch.tensor([[2, 1]], dtype=torch.int32)
    assert SP.mean_duration(hours, count).item() == 4.0 and SP.mean_duration(hours[None, None], count[None, None]).shape == (1, 1)
    assert math.isnan(SP.mean_duration(torch.zeros(1, 2), torch.zeros(1, 2)).item())
    assert SP.event_frequency(hours, 12).item() == 0.5
    longest = torch.tensor([[3, 5]], dtype=torch.int32).view(1, 1, 1, 1, 2)
    longest = torch.cat([longest, longest + torch.tensor([1, 3]).view(1, 1, 1, 1, 2), longest - 2])
    bias, rmse = SP.longest_spell_error(longest)
    assert bias.flatten().tolist() == [2.0, -2.0] and rmse.flatten().tolist() == [math.sqrt(5.0), 2.0]
    assert SP.onset_share(torch.tensor([[3, 0, 1], [0, 0, 0]]))[0].tolist() == [0.75, 0.0, 0.25]
    assert torch.isnan(SP.onset_share(torch.tensor([[3, 0, 1], [0, 0, 0]]))[1]).all()


def test_the_report(route):
    M, T, F, H, W_, K = 3, 19, 2, 2, 8, 2
    x, y, thr, above, S, Tr, th, names = _case("smooth", M, T, F, H, W_, K, "above")
    rep = SP.spells_report(S, Tr, th, "above", 12, 6, 1, names=["tas", "psl"])
    assert isinstance(rep, VariableReport) and rep.names == ["tas", "psl"]
    t = SP.spell_tables(S, Tr, th, "above", 12, 6, 1)
    for f, (name, v) in enumerate(rep):
        assert torch.equal(v["thresholds"], th[f]) and torch.equal(v["mean_duration"], SP.mean_duration(t.hours, t.count)[:, f])
        assert torch.equal(v["event_frequency"], SP.event_frequency(t.hours, T)[:, f]) and v["event_frequency"].shape == (M + 1, K)
        assert torch.equal(v["duration_distance"], SP.spell_duration_distance(t.hist)[:, f]) and v["duration_distance"].shape == (M, K)
        assert torch.equal(v["longest_bias"], SP.longest_spell_error(t.longest)[0][:, f]) and torch.equal(v["censored"], t.censored[:, f])
        assert torch.equal(v["onset_share"], SP.onset_share(t.onsets)[:, f]) and torch.equal(v["spells"], t.hist.sum(dim=-1)[:, f])
        assert torch.equal(v["survival"], SP.survival(t.hist)[:, f]) and torch.equal(v["longest_max"], t.longest.amax(dim=(-1, -2))[:, f])
    flat = rep.as_dict()
    assert set(flat) == {f"spells/{n}/{q}_k{k}{s}" for n in ("tas", "psl") for q in ("mean_duration", "duration_distance", "longest_bias")
                         for k in (0, 1) for s in ("", "_std")}
    assert flat["spells/tas/mean_duration_k1"] == pytest.approx(rep["tas"]["mean_duration"][1:, 1].mean().item(), abs=1e-15)
    assert "onset_share" not in SP.spells_report(S, Tr, th)["var0"]


# ------------------------------------------------------------------------------------------------------------------ inputs

def test_strided_and_half_precision_inputs_and_float64_thresholds(route):
    g = torch.Generator().manual_seed(3)
    base = (torch.randn(3, 11, 2, 4, 16, generator=g) * 2.0).to(torch.float16)
    view, truth = base[..., ::2], base[0, ..., 1::2]
    thr64 = torch.tensor([[0.1, 1.3], [-0.7, 0.9]], dtype=torch.float64)
    a = SP.spell_tables(view, truth, thr64, ["above", "below"], 5, 3)
    b = SP.spell_tables(view.float().contiguous(), truth.float().contiguous(), thr64.float(), ["above", "below"], 5, 3)  # rounded once to fp32
    _assert_same_tables(a, b)
    c = SP.spell_tables(view.to(torch.bfloat16).double(), truth.double(), thr64, ["above", "below"], 5, 3)
    assert c.hist.shape == a.hist.shape


def test_argument_errors_are_value_errors(route):
    S, Tr, thr = torch.zeros(2, 3, 2, 4, 8), torch.zeros(3, 2, 4, 8), torch.zeros(2, 1)
    make = lambda **kw: SP.SpellAccumulator(2, 2, 4, 8, thr, **kw)
    for name, kw in (("M", dict(M=0)), ("F", dict(F=0)), ("H", dict(H=0)), ("W", dict(W=-1))):
        args = dict(M=2, F=2, H=4, W=8)
        args.update(kw)
        with pytest.raises(ValueError, match=f"{name} .* must be an integer >= 1"):
            SP.SpellAccumulator(args["M"], args["F"], args["H"], args["W"], thr)
    with pytest.raises(ValueError, match="max_duration 0 must be an integer >= 1"):
        make(max_duration=0)
    with pytest.raises(ValueError, match="period -1 must be an integer >= 0"):
        make(period=-1)
    with pytest.raises(ValueError, match="period 2.5 must be an integer"):
        make(period=2.5)
    with pytest.raises(ValueError, match="t0 -3 must be an integer >= 0"):
        make(t0=-3)
    for bad in (torch.zeros(3, 1), torch.zeros(2), torch.zeros(2, 0)):
        with pytest.raises(ValueError, match=r"thresholds .* must be \(F, K\)"):
            SP.SpellAccumulator(2, 2, 4, 8, bad)
    with pytest.raises(ValueError, match="must be 'above' or 'below'"):
        SP.SpellAccumulator(2, 2, 4, 8, thr, "over")
    acc = make()
    with pytest.raises(ValueError, match="made with a truth"):
        acc.update(S)
    with pytest.raises(ValueError, match="made without a truth"):
        make(with_truth=False).update(S, Tr)
    with pytest.raises(ValueError, match=r"samples \(2, 3, 2, 4, 8\) must be \(M >= 1,\) \+ truth \(3, 2, 4, 4\)"):
        acc.update(S, Tr[..., :4])
    with pytest.raises(ValueError, match="must be floating point"):
        acc.update(S.long(), Tr)
    with pytest.raises(ValueError, match=r"must be floating point \(M, T, F, H, W\)"):
        make(with_truth=False).update(S[0])
    with pytest.raises(ValueError, match=r"must be \(M, T, F, H, W\) = \(2, T, 2, 4, 8\)"):
        acc.update(torch.zeros(3, 3, 2, 4, 8), Tr)
    with pytest.raises(ValueError, match=r"must be \(M, T, F, H, W\) = \(2, T, 2, 4, 8\)"):
        acc.update(torch.zeros(2, 3, 2, 8, 4), torch.zeros(3, 2, 8, 4))
    acc.n_times = SP.MAX_TIME - 2
    with pytest.raises(ValueError, match=r"the total time must stay under 2\^31"):
        acc.update(S, Tr)
    acc.n_times = 0
    assert int(acc.state.abs().sum()) == 0 and acc.update(S[:, :0], Tr[:0]).n_times == 0  # a block of no times is a no-op
    with pytest.raises(ValueError, match=r"samples \(3, 2, 4, 8\) must be \(M, T, F, H, W\)"):
        SP.spell_tables(Tr, None, thr)
    other = SP.SpellAccumulator(2, 2, 4, 8, thr, period=3)
    with pytest.raises(ValueError, match="period 0 of the state differs"):
        other.load_state_dict(acc.state_dict())
    with pytest.raises(ValueError, match="thresholds or directions of the state differ"):
        SP.SpellAccumulator(2, 2, 4, 8, thr + 1).load_state_dict(acc.state_dict())
    with pytest.raises(ValueError, match=r"state .* of the state must be"):
        SP.SpellAccumulator(3, 2, 4, 8, thr).load_state_dict(acc.state_dict())
    with pytest.raises(ValueError, match=r"must be \(\.\.\., D >= 2, F, K, Lmax\)"):
        SP.spell_duration_distance(torch.zeros(1, 2, 2, 4))
    with pytest.raises(ValueError, match=r"must be \(\.\.\., D >= 2, F, K, H, W\)"):
        SP.longest_spell_error(torch.zeros(2, 2, 4, 8))
    with pytest.raises(ValueError, match="must have one shape"):
        SP.mean_duration(torch.zeros(2, 4), torch.zeros(2, 5))
    with pytest.raises(ValueError, match=r"must be \(\.\.\., H, W\)"):
        SP.event_frequency(torch.zeros(4), 3)
    with pytest.raises(ValueError, match=r"must be \(\.\.\., Lmax\)"):
        SP.duration_pmf(torch.zeros(()))
    with pytest.raises(ValueError, match=r"must be \(\.\.\., period >= 1\)"):
        SP.onset_share(torch.zeros(2, 0))
    with pytest.raises(ValueError, match="1 names for 2 variables"):
        SP.spells_report(S, Tr, thr, names=["a"])
    with pytest.raises(ValueError, match=r"\(L, F, H, W\)"):
        SP.spells_report(S, Tr[:2], thr)


def test_the_launcher_declines_what_the_kernel_does_not_take(monkeypatch):
    """hw = 6, K = 9, Lmax = 257 and period = 25: *_supported says no before a launcher is reached, the launcher itself answers False
    and writes nothing, and the general route gives the reference's integers"""
    emu_spell_ops.install(monkeypatch, spell_ops, SP)
    for H, W_, K, Lmax, period in ((1, 6, 2, 4, 6), (2, 4, 9, 4, 6), (2, 4, 2, 257, 6), (2, 4, 2, 4, 25)):
        x, y, thr, above, S, Tr, th, names = _case("smooth", 2, 9, 1, H, W_, K)
        _assert_equal_ref(SP.spell_tables(S, Tr, th, names, Lmax, period, 2), R.spells_ref(x, y, thr, above, Lmax, period, 2), (H, W_, K, Lmax, period))
        assert emu_spell_ops.CALLS == [] and not emu_spell_ops.supported(H * W_, K, Lmax, period)
        D, hw = 3, H * W_
        xs, ys = torch.tensor(x), torch.tensor(y)
        state = torch.full((4, D, 1, K, hw), -7, dtype=torch.int32)
        hist, onsets, invalid = (torch.full(s, -7, dtype=torch.int64) for s in ((D, 1, K, Lmax), (D, 1, K, period), (D, 1)))
        assert emu_spell_ops.spell_update(xs, ys, th, torch.tensor(above.astype(np.int32)), state, hist, onsets, invalid, 2, 9, 1, hw, K, Lmax, period, 2) is False
        assert all(bool((t == -7).all()) for t in (state, hist, onsets, invalid))
        del emu_spell_ops.CALLS[:]
    assert emu_spell_ops.supported(4, 1, 1, 0) and emu_spell_ops.supported(16384, 8, 256, 24) and not emu_spell_ops.supported(0, 1, 1, 0)
    assert not emu_spell_ops.supported(8, 0, 1, 0) and not emu_spell_ops.supported(8, 1, 0, 0) and not emu_spell_ops.supported(8, 1, 1, -1)


def test_the_emulation_restates_the_constants_of_the_kernel():
    core = open(os.path.join(ROOT, "climate2weather_amd", "csrc", "spells_core.h")).read()
    for text in ("THREADS = 256", "CELLS = 4", "CHUNK = THREADS * CELLS", "GROUP = 4", "UNROLL = 8", "MAX_K = 8, MAX_LMAX = 256, MAX_PERIOD = 24",
                 "MAX_T = 1 << 20", "LDS_INTS = LDS_INVALID + 1",
                 "hw >= 4 && hw % 4 == 0 && K >= 1 && K <= MAX_K && lmax >= 1 && lmax <= MAX_LMAX && period >= 0 && period <= MAX_PERIOD"):
        assert text in core, text
    assert (emu_spell_ops.THREADS, emu_spell_ops.CELLS, emu_spell_ops.CHUNK, emu_spell_ops.GROUP) == (256, 4, 1024, 4)
    assert (emu_spell_ops.MAX_K, emu_spell_ops.MAX_LMAX, emu_spell_ops.MAX_PERIOD, emu_spell_ops.MAX_T, emu_spell_ops.LDS_INTS) == (8, 256, 24, 1 << 20, 1121)
    assert [emu_spell_ops.chunks(hw) for hw in (4, 1024, 1028, 2052, 16384)] == [1, 1, 2, 3, 16]
    assert [emu_spell_ops.groups(K) for K in (1, 4, 5, 8)] == [[(0, 1)], [(0, 4)], [(0, 4), (4, 1)], [(0, 4), (4, 4)]]
    assert SP.MAX_BLOCK == emu_spell_ops.MAX_T


# ------------------------------------------------------------------------------------------------------------------ the host program

@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_spells(request, tmp_path_factory):
    """a stand-alone program, once plain and once under the address and undefined-behaviour sanitizers; it is run directly, never loaded
    into Python"""
    return host_program.build(tmp_path_factory, "spells", sanitize=request.param == "sanitized", timeout=600)


@pytest.mark.parametrize("M,T,F,hw,K,Lmax,period,has_truth", [(1, 1, 1, 4, 1, 1, 0, 0), (2, 9, 2, 1028, 5, 3, 6, 1), (1, 8, 1, 2052, 8, 256, 24, 1),
                                                              (3, 7, 2, 1024, 4, 48, 1, 0), (1, 33, 1, 12, 3, 2, 5, 1)])
def test_every_cell_hour_is_read_once_per_group_and_every_state_entry_moves_once(host_spells, M, T, F, hw, K, Lmax, period, has_truth):
    """one thread, a chunk and a thread, three chunks, exactly one chunk; T around the unroll; one, two and full threshold groups"""
    rc = subprocess.run([str(host_spells), "visit"] + [str(a) for a in (M, T, F, hw, K, Lmax, period, has_truth)], timeout=600).returncode
    assert rc == 0, f"check {rc} of host_spells_main.cpp failed"


def test_the_host_program_equals_the_reference(host_spells, tmp_path):
    """csrc/spells_core.h compiled for the host, every kind, one block and two: the chunks, the groups, the carried state, the bins;
    the open runs are closed here as tables() closes them"""
    M, F = 2, 2
    for i, kind in enumerate(R.KINDS):
        hw, T, K, Lmax, period, t0, split = ((1028, 9, 5, 4, 6, 5, 4), (12, 17, 3, 256, 24, 0, 0), (64, 8, 8, 2, 1, 3, 7))[i % 3]
        has_truth = i % 2
        x, y = R.fields(kind, M, T, F, hw)
        thr, above = R.thresholds(kind, y, K), R.directions(F, K, "mixed")
        D = M + has_truth
        files = [str(tmp_path / n) for n in ("x.f32", "y.f32", "thr.f32", "dir.i32", "state.i32", "hist.i64", "onsets.i64", "invalid.i64")]
        for a, p in zip((x, y, thr, above.astype(np.int32)), files):
            a.tofile(p)
        args = [str(a) for a in (M, T, F, hw, K, Lmax, period, t0, has_truth, split)]
        assert subprocess.run([str(host_spells), "update"] + args + files, timeout=600).returncode == 0
        want = R.spells_ref(x, y if has_truth else None, thr, above, Lmax, period, t0)
        state = np.fromfile(files[4], np.int32).reshape(4, D, F, K, hw).astype(np.int64)
        hist = np.fromfile(files[5], np.int64).reshape(D, F, K, Lmax)
        open_ = state[0]
        for d, f, k in np.ndindex(D, F, K):
            hist[d, f, k] += np.bincount(np.minimum(open_[d, f, k][open_[d, f, k] > 0], Lmax) - 1, minlength=Lmax)
        assert np.array_equal(hist, want["hist"]), kind
        assert np.array_equal(state[2] + (open_ > 0), want["count"]) and np.array_equal(np.maximum(state[1], open_), want["longest"]), kind
        assert np.array_equal(state[3], want["hours"]) and np.array_equal(np.fromfile(files[7], np.int64).reshape(D, F), want["invalid"]), kind
        assert np.array_equal(np.fromfile(files[6], np.int64).reshape(D, F, K, period), want["onsets"]), kind


# ------------------------------------------------------------------------------------------------------------------ C ABI

def test_new_entry_points_have_matching_argument_lists():
    names = {"c2w_spell_supported": "int", "c2w_spell_update": "int"}
    c_abi.assert_declared(names, "spells.hip", spell_ops, ("supported", "spell_update"))
