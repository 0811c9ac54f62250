"""CPU checks of the held-out validation (climate2weather_amd.evaluation, Trainer.validate) with the HIP launchers replaced by
tests/emu_eval_ops.py: the plan, the fp32 bin rule, the table against the oracle's unreduced loss, no side effects on training, the EMA
copy, the two-rank all-reduce, and the C declarations against the ctypes prototypes."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import c_abi
import emu_eval_ops
from climate2weather_amd import _lib
from climate2weather_amd import ops as c2w_ops
from climate2weather_amd.data import DeviceWindowFeed, SyntheticWindowDataset
from climate2weather_amd.evaluation import LevelLoss, evaluate, level_bins, validation_plan
from climate2weather_amd.pipelines import SDAPipeline
from climate2weather_amd.score import ScoreUNet
from climate2weather_amd.training import Trainer
from oracle import diffusion as od
from oracle import unet as ou

TINY = dict(embedding_dim=64, hidden_channels=[32, 64], hidden_blocks=[1, 1], attention_levels=[1], kernel_size=3, padding_mode="zeros")


@pytest.fixture()
def emu(monkeypatch):
    emu_eval_ops.install(monkeypatch, c2w_ops)


def _tiny(seed=3):
    torch.manual_seed(seed)
    return ScoreUNet(channels=6, spatial=2, activation=torch.nn.SiLU, **TINY)


def _golden(golden_dir):
    return {k: v for k, v in np.load(os.path.join(golden_dir, "tiny_net.npz"), allow_pickle=False).items()}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


# ------------------------------------------------------------------------------------------------------------------ plan, bins

@pytest.mark.parametrize("n,world,batch", [(23, 3, 4), (10, 4, 3), (7, 2, 2), (5, 1, 8)])
def test_shards_partition_the_items(n, world, batch):
    seen = []
    for r in range(world):
        plan = validation_plan(n, batch, seed=1, shard=(r, world))
        assert [p.first for p in plan] == sorted(p.first for p in plan)
        for p in plan:
            assert 0 < p.count <= batch and p.t.shape == (p.count,) and p.t.dtype == torch.float32 and 0 <= p.noise_seed < 1 << 62
            seen += list(range(p.first, p.first + p.count))
        if plan:  # a shard is contiguous; only its last batch may be short
            assert all(p.count == batch for p in plan[:-1])
            assert plan[0].first == r * n // world and plan[-1].first + plan[-1].count == (r + 1) * n // world
    assert seen == list(range(n))


@pytest.mark.parametrize("n,K", [(60, 10), (64, 16), (64, 1), (57, 10), (200, 16), (9, 10)])
def test_stratified_t_covers_every_bin_evenly(n, K):
    """t_i = (i + u_i) / n puts exactly one item into every cell [i / n, (i + 1) / n), so the number of items below x is n x rounded
    down or up: N(x) - n x lies in (-1, 1].  Where K divides n the bin edges are cell edges and every bin holds exactly n / K items
    (well inside the n / K +- 1 this check was specified with).  Where it does not, a bin's count N(b) - N(a) can only be said to lie
    strictly within n / K +- 2: n = 57, K = 10, seed 4 puts 7 items into bin 5 (cells 28 and 34 straddle its edges and both draws fall
    inside), 1.3 above 5.7 -- so +- 1 is asserted where it is a property of the formula and the provable bound elsewhere."""
    t = torch.cat([p.t for p in validation_plan(n, 8, seed=4)])
    cnt = np.bincount(level_bins(t, K).numpy(), minlength=K)
    print(f"stratified n={n} K={K}: counts {cnt.tolist()}")
    assert cnt.sum() == n
    if n % K == 0:
        assert np.all(np.abs(cnt - n / K) <= 1.0), cnt
    else:
        assert np.all(np.abs(cnt - n / K) < 2.0), cnt
    # item i meets the same t whatever the sharding and batching
    t2 = torch.cat([p.t for r in range(3) for p in validation_plan(n, 5, seed=4, shard=(r, 3))])
    assert torch.equal(t, t2)


def test_plan_is_a_function_of_the_seed():
    a, b, c = validation_plan(40, 8, seed=7), validation_plan(40, 8, seed=7), validation_plan(40, 8, seed=8)
    assert all(p.first == q.first and p.noise_seed == q.noise_seed and torch.equal(p.t, q.t) for p, q in zip(a, b))
    assert all(p.noise_seed != q.noise_seed and not torch.equal(p.t, q.t) for p, q in zip(a, c))
    assert len({p.noise_seed for p in a}) == len(a)
    given = torch.linspace(0, 1, 40)
    assert torch.equal(torch.cat([p.t for p in validation_plan(40, 8, seed=7, t=given)]), given)
    u = torch.cat([p.t for p in validation_plan(40, 8, seed=7, t="uniform")])
    assert u.min() >= 0 and u.max() < 1 and not torch.equal(u, torch.cat([p.t for p in a]))


def test_bin_rule_is_the_fp32_one():
    assert level_bins(torch.tensor([0.7, 0.9, 1.0, 0.0, 1.5, -0.2]), 10).tolist() == [7, 9, 9, 0, 9, 0]
    # the same formula in float64 lands one bin lower at both values: the reason the rule is pinned to fp32
    assert [int(np.floor(np.float64(np.float32(v)) * 10)) for v in (0.7, 0.9)] == [6, 8]
    assert emu_eval_ops.level_bins_f32([0.7, 0.9, 1.0], 10).tolist() == [7, 9, 9]
    assert level_bins(torch.tensor([0.3, 1.0]), 1).tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------------------------ tiny net vs oracle

@pytest.mark.parametrize("batch", [2, 1])
def test_table_matches_the_oracles_unreduced_loss(emu, golden_dir, batch):
    g = _golden(golden_dir)
    net = _tiny()
    x, t, eps = (torch.from_numpy(g[k]) for k in ("x", "t", "eps"))
    K = 10
    res = evaluate(net, SDAPipeline(), x, batch=batch, bins=K, precision="fp32", t=t.reshape(-1), eps=eps, window=3)
    assert res.mean() == pytest.approx(float(g["loss"]), rel=1e-5)
    ref = ou.OracleScoreUNet(net.state_dict(), TINY["hidden_blocks"], TINY["attention_levels"])
    with torch.no_grad():
        sq = od.loss(ref, x, t.view(-1, 1, 1, 1), eps).double()
    want = torch.zeros(K, 6, dtype=torch.float64).index_add_(0, level_bins(t, K), sq.sum(dim=(2, 3)))
    assert (res.table - want).abs().max().item() <= 1e-5 * want.max().item()
    assert res.count.tolist() == np.bincount(level_bins(t, K).numpy(), minlength=K).tolist()
    # the readers: frame c // F, variable c % F
    assert (res.F, res.w, res.H, res.W) == (2, 3, 16, 16)
    tab = want.view(K, 3, 2).numpy()
    np.testing.assert_allclose(res.by_frame(), tab.sum((0, 2)) / (2 * 2 * 256), rtol=1e-5)
    np.testing.assert_allclose(res.by_variable(), tab.sum((0, 1)) / (2 * 3 * 256), rtol=1e-5)
    full = res.count.numpy() > 0
    np.testing.assert_allclose(res.centre_frame()[full], tab[full, 1, :] / (res.count.numpy()[full, None] * 256), rtol=1e-5)
    np.testing.assert_allclose(res.by_level()[full], tab[full].sum((1, 2)) / (res.count.numpy()[full] * 6 * 256), rtol=1e-5)
    assert np.isnan(res.by_level()[~full]).all()
    d = res.as_dict()
    assert d["valid/loss"] == pytest.approx(res.mean()) and d["valid/items"] == 2 and all(isinstance(v, float) for v in d.values())
    assert d["valid/centre"] == pytest.approx(tab[:, 1].sum() / (2 * 2 * 256), rel=1e-5)


def test_lazy_windows_equal_the_gathered_tensor_and_leave_the_feed_alone(emu):
    ds = SyntheticWindowDataset(9, 2, 16, 16, window=3, seed=2)
    feed = DeviceWindowFeed(ds, torch.device("cpu"), seed=1)
    cursor = feed.sampler.cursor
    net, pipe = _tiny(), SDAPipeline()
    a = evaluate(net, pipe, feed, batch=3, bins=4, seed=9, precision="fp32")
    assert feed.sampler.cursor == cursor and (a.F, a.w) == (2, 3) and int(a.count.sum()) == len(ds) == 7
    dense = torch.stack([ds[i] for i in range(len(ds))])
    b = evaluate(net, pipe, dense, batch=3, bins=4, seed=9, precision="fp32", window=3)
    c = evaluate(net, pipe, ds, batch=3, bins=4, seed=9, precision="fp32")
    d = evaluate(net, pipe, [dense[:2], dense[2:]], batch=3, bins=4, seed=9, precision="fp32", window=3)
    for o in (b, c, d):
        assert torch.equal(a.table, o.table) and torch.equal(a.count, o.count)
    # another batching draws other noise for the same items (documented: the table depends on (seed, n_items, batch, world))
    assert not torch.equal(a.table, evaluate(net, pipe, feed, batch=2, bins=4, seed=9, precision="fp32").table)
    wb = feed.ordered_batch(2, 3)
    assert torch.equal(wb.materialize(), dense[2:5]) and feed.sampler.cursor == cursor
    with pytest.raises(IndexError):
        feed.ordered_batch(5, 3)
    # max_items and out=
    e = evaluate(net, pipe, feed, batch=3, bins=4, seed=9, precision="fp32", max_items=3)
    assert int(e.count.sum()) == 3
    assert evaluate(net, pipe, feed, batch=3, bins=4, seed=9, precision="fp32", max_items=3, out=e) is e and int(e.count.sum()) == 6


def test_evaluate_consumes_no_torch_rng_and_keeps_the_mode_flag(emu):
    net = _tiny()
    net.train()
    torch.manual_seed(5)
    before = torch.get_rng_state()
    evaluate(net, SDAPipeline(), torch.rand(3, 6, 16, 16, generator=torch.Generator().manual_seed(1)), batch=2, precision="fp32", window=3)
    assert torch.equal(before, torch.get_rng_state()) and net.training


def test_short_scratch_is_refused(emu):
    y = torch.zeros(2 * 64, 8)
    with pytest.raises(_lib.C2wError, match="bad argument"):
        c2w_ops.sq_err_levels(y, torch.zeros(2, 6, 8, 8), torch.zeros(2), torch.zeros(4, 6, dtype=torch.float64), torch.zeros(4, dtype=torch.int64),
                              None, 2, 6, 64, 8, 4, torch.zeros(2), 0)


# ------------------------------------------------------------------------------------------------------------------ Trainer.validate

def _toy_run(validate: bool):
    """the toy recipe of tests/test_gpu_deterministic.py's child script, 6 steps, on the emulated launchers"""
    cfg = dict(embedding_dim=64, hidden_channels=[64, 128], hidden_blocks=[1, 1], attention_levels=[1], kernel_size=3, padding_mode="zeros")
    torch.manual_seed(11)
    net = ScoreUNet(channels=6, spatial=2, activation=torch.nn.SiLU, **cfg)
    tr = Trainer(net, lr=2e-3, precision="fp32", ema_rates=[0.999, 0.9])
    gen = torch.Generator().manual_seed(3)
    base = torch.randn(8, 6, 32, 32, generator=gen) * 0.5 + 0.5
    held = torch.randn(5, 6, 32, 32, generator=torch.Generator().manual_seed(77)) * 0.5 + 0.5
    losses, vals = [], []
    for s in range(6):
        x = base + 0.05 * torch.randn(8, 6, 32, 32, generator=gen)
        t = torch.rand(8, generator=gen)
        eps = torch.randn(8, 6, 32, 32, generator=gen)
        losses.append(float(tr.step(x, t=t, eps=eps)).hex())
        if validate and s in (2, 4):
            state = (tr.eng.flat.clone(), tr.eng.flat_grad.clone(), tr.m.clone(), tr.v.clone(), [e.clone() for e in tr.ema_flats], tr.cur_ndata,
                     tr.step_count, tr.rng_cpu.get_state().clone(), tr.rng_dev.get_state().clone())
            vals.append(tr.validate(held, weights="ema" if s == 2 else "net", batch=2, bins=4, seed=1, window=3))
            assert torch.equal(state[0], tr.eng.flat) and torch.equal(state[1], tr.eng.flat_grad) and torch.equal(state[2], tr.m)
            assert torch.equal(state[3], tr.v) and all(torch.equal(a, b) for a, b in zip(state[4], tr.ema_flats))
            assert (state[5], state[6]) == (tr.cur_ndata, tr.step_count)
            assert torch.equal(state[7], tr.rng_cpu.get_state()) and torch.equal(state[8], tr.rng_dev.get_state())
    return losses, tr, vals


def test_validation_leaves_training_bit_for_bit_unchanged(emu):
    la, ta, vals = _toy_run(True)
    lb, tb, _ = _toy_run(False)
    assert la == lb
    assert torch.equal(ta.eng.flat, tb.eng.flat) and torch.equal(ta.m, tb.m) and torch.equal(ta.v, tb.v)
    assert all(torch.equal(a, b) for a, b in zip(ta.ema_flats, tb.ema_flats))
    assert all(int(v.count.sum()) == 5 and np.isfinite(v.mean()) and v.mean() > 0 for v in vals)
    assert not torch.equal(vals[0].table, vals[1].table)  # EMA after step 2 and live weights after step 4 are different networks


def test_validate_runs_on_the_ema_weights(emu, golden_dir):
    g = _golden(golden_dir)
    net = _tiny()
    tr = Trainer(net, lr=1e-2, precision="fp32", ema_rates=[0.999, 0.9])
    x, t, eps = (torch.from_numpy(g[k]) for k in ("x", "t", "eps"))
    for _ in range(3):
        tr.step(x, t=t.reshape(-1), eps=eps)
    held = torch.randn(5, 6, 16, 16, generator=torch.Generator().manual_seed(8)) * 0.5 + 0.5
    got = tr.validate(held, weights=0.9, batch=2, bins=5, seed=3, window=3)
    fresh = _tiny(seed=99)
    fresh.load_state_dict(dict(tr.ema_state_dicts())[0.9])
    want = evaluate(fresh, tr.pipeline, held, batch=2, bins=5, seed=3, precision="fp32", window=3)
    assert torch.equal(got.count, want.count)
    assert torch.allclose(got.table, want.table, rtol=1e-10, atol=0.0)
    live = tr.validate(held, weights="net", batch=2, bins=5, seed=3, window=3)
    first = tr.validate(held, batch=2, bins=5, seed=3, window=3)  # "ema": the first rate
    assert not torch.equal(live.table, got.table) and not torch.equal(first.table, got.table)
    again = tr.validate(held, weights=0.9, batch=2, bins=5, seed=3, window=3)
    assert torch.equal(again.table, got.table)  # same weights, same plan: same bits
    with pytest.raises(ValueError):
        tr.validate(held, weights=0.5, batch=2, window=3)


def test_two_ranks_all_reduce_to_the_merge_of_their_shards(emu, tmp_path):
    from _validate_worker import CFG, held_out, run
    mp.spawn(run, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"valid{r}.pt", weights_only=False) for r in (0, 1))
    torch.manual_seed(3)
    net = ScoreUNet(**CFG)
    kw = dict(batch=2, bins=4, seed=5, precision="fp32", window=3)
    want = evaluate(net, SDAPipeline(), held_out(), shard=(0, 2), **kw).merge(evaluate(net, SDAPipeline(), held_out(), shard=(1, 2), **kw))
    for r in (r0, r1):
        assert torch.equal(r["count"], want.count) and int(r["count"].sum()) == 7
        assert torch.allclose(r["table"], want.table, rtol=1e-12, atol=0.0)
    whole = LevelLoss(4, 2, 3, 16, 16)
    with pytest.raises(ValueError):
        whole.merge(LevelLoss(5, 2, 3, 16, 16))


# ------------------------------------------------------------------------------------------------------------------ C ABI

def test_new_entry_points_have_matching_argument_lists():
    names = {"c2w_sq_err_levels_scratch_bytes": "long long", "c2w_sq_err_levels": "int", "c2w_sq_err_levels_noise": "int"}
    c_abi.assert_declared(names)
