"""CPU checks of the host logic around the network -- training step, all-reduce path (gloo, world_size 2), sampler,
score functions, data feed, construction seam -- with the HIP launchers replaced by tests/emu_ops.py."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import emu_ops
from climate2weather_amd import ops as c2w_ops
from climate2weather_amd import util as c2w_util
from climate2weather_amd.data import DeviceWindowFeed, InfiniteSampler, SyntheticWindowDataset
from climate2weather_amd.ema import StandardEMA
from climate2weather_amd.lr import linear_learning_rate_schedule
from climate2weather_amd.pipelines import SDAPipeline
from climate2weather_amd.score import ScoreUNet
from climate2weather_amd.score_fn import BatchedScoreFunction, DefaultScoreFunction, PoolStrideOperator
from climate2weather_amd.training import Trainer, load_latest_checkpoint, save_checkpoint
from oracle import diffusion as od
from oracle import host as oh
from oracle import unet as ou

TINY = dict(embedding_dim=64, hidden_channels=[32, 64], hidden_blocks=[1, 1], attention_levels=[1], kernel_size=3,
            padding_mode="zeros")


@pytest.fixture()
def emu(monkeypatch):
    emu_ops.install(monkeypatch, c2w_ops)


def _golden(golden_dir, name):
    return {k: v for k, v in np.load(os.path.join(golden_dir, name), allow_pickle=False).items()}


def _tiny(seed=3):
    torch.manual_seed(seed)
    return ScoreUNet(channels=6, spatial=2, activation=torch.nn.SiLU, **TINY)


def _oracle_step(g, lr, world_batches=1):
    """expected parameters after one AdamW step on the golden gradients"""
    out = {}
    for k in [str(n) for n in g["param_order"]]:
        p, gr = torch.from_numpy(g["sd." + k]), torch.from_numpy(g["grad." + k])
        out[k] = oh.adamw_step(p, gr, torch.zeros_like(p), torch.zeros_like(p), 1, lr)[0]
    return out


def _assert_adam_close(v, ref, grad, lr, name):
    """Adam's first step is lr * g/(|g| + eps): where |g| ~ eps (1e-8) a 1e-9 gradient difference moves the update by a
    visible fraction of lr, so compare tightly only where the gradient is well above eps."""
    big = grad.abs() > 1e-5
    assert torch.allclose(v[big], ref[big], atol=2e-6), name
    assert (v - ref).abs().max().item() <= 2.0 * lr, name


def test_training_step_matches_oracle(emu, golden_dir, tmp_path):
    g = _golden(golden_dir, "tiny_net.npz")
    net = _tiny()
    tr = Trainer(net, lr=1e-3, precision="fp32", ema_rates=[0.9, 0.999])
    x, t, eps = (torch.from_numpy(g[k]) for k in ("x", "t", "eps"))
    loss = tr.step(x, t=t.reshape(-1), eps=eps)
    assert float(loss) == pytest.approx(float(g["loss"]), rel=1e-5)
    exp = _oracle_step(g, 1e-3)
    for k, v in net.state_dict().items():
        _assert_adam_close(v, exp[k], torch.from_numpy(g["grad." + k]), 1e-3, k)
    # EMA: p_ema = r p0 + (1-r) p1
    for (rate, sd) in tr.ema_state_dicts():
        for k, v in sd.items():
            ref = oh.ema_update(torch.from_numpy(g["sd." + k]), net.state_dict()[k], rate)
            assert torch.allclose(v, ref, atol=1e-6), k
    assert tr.cur_ndata == 2 and tr.step_count == 1
    # checkpoint round trip (training-state-XXXXXXX.ckpt, latest wins)
    p = save_checkpoint(tr, str(tmp_path))
    assert os.path.basename(p) == "training-state-0000000.ckpt"
    net2 = _tiny(seed=99)
    tr2 = Trainer(net2, lr=1e-3, precision="fp32", ema_rates=[0.9, 0.999])
    assert load_latest_checkpoint(tr2, str(tmp_path)) == p
    for (k, a), (_, b) in zip(net.state_dict().items(), net2.state_dict().items()):
        assert torch.equal(a, b), k
    assert torch.equal(tr.m, tr2.m) and tr2.step_count == 1
    # the file has the reference's schema (src/thor/checkpoint.py:13-35): torch's AdamW and StandardEMA accept its parts
    ck = torch.load(p, weights_only=False)
    assert set(ck) == {"state", "net", "pipeline", "optimizer", "ema"} and ck["state"]["cur_ndata"] == 2
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3)
    opt.load_state_dict(ck["optimizer"])
    first = next(iter(net.parameters()))
    assert torch.equal(opt.state[first]["exp_avg"], tr._per_param(tr.m)[0][1])
    assert ck["ema"]["rates"] == [0.9, 0.999] and set(ck["ema"]["emas"][0]) == set(net.state_dict())


def test_gradient_accumulation_sums_rounds(emu, golden_dir):
    g = _golden(golden_dir, "tiny_net.npz")
    net = _tiny()
    tr = Trainer(net, lr=0.0, precision="fp32", ema_rates=[])
    x = torch.from_numpy(g["x"])
    torch.manual_seed(0)
    tr.step([x[:1].contiguous(), x[1:].contiguous()])
    ga = tr.eng.flat_grad.clone()
    torch.manual_seed(0)
    tr.step([x[:1].contiguous()])
    g1 = tr.eng.flat_grad.clone()
    assert ga.abs().sum() > g1.abs().sum() > 0  # two rounds accumulated into the same buffer


def test_resume_from_a_reference_made_training_state_checkpoint(emu, golden_dir):
    from _ckpt_check import resume_from_reference_checkpoint
    resume_from_reference_checkpoint(golden_dir, torch.device("cpu"), lambda seed: _tiny(seed=seed))


@pytest.mark.parametrize("bucket_mb", [48.0, 0.05])
def test_optimizer_chasing_the_backward_equals_the_update_after_it(emu, golden_dir, bucket_mb):
    """Trainer.chase_optimizer: per finished bucket of the flat gradient buffer the fused AdamW + EMA kernel runs while backward is
    still going (the rest of the backward reads copies of the weights, never the flat buffer: engine.Tape.progress).  Same
    parameters, moments, EMA and loss as the update behind the backward -- with 22 buckets cutting through layers."""
    g = _golden(golden_dir, "tiny_net.npz")
    x, t, eps = (torch.from_numpy(g[k]) for k in ("x", "t", "eps"))
    outs = []
    for chase in (False, True):
        net = _tiny()
        tr = Trainer(net, lr=1e-3, precision="fp32", ema_rates=[0.9], bucket_mb=bucket_mb)
        tr.chase_optimizer = chase
        losses = [float(tr.step(x, t=t.reshape(-1), eps=eps)) for _ in range(2)]
        outs.append((losses, tr.eng.flat.clone(), tr.m.clone(), tr.v.clone(), tr.ema_flats[0].clone()))
    assert outs[0][0] == outs[1][0]
    for a, b in zip(outs[0][1:], outs[1][1:]):
        assert torch.equal(a, b)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_fp16_training_step_runs_under_the_dynamic_loss_scale(emu):
    """precision="fp16" (the reference's Fabric "16-mixed", train.py:98): the step multiplies the loss gradient by the device-held
    scale, unscales inside the optimizer, skips the update (but not the EMA) when a gradient is non-finite and halves the scale;
    after `growth_interval` clean steps the scale doubles.  Host logic only -- the launchers are the PyTorch test double."""
    cfg = dict(TINY, hidden_channels=[64, 64])  # 16-bit modes: channel counts in whole 128-byte K chunks
    torch.manual_seed(3)
    net = ScoreUNet(channels=6, spatial=2, activation=torch.nn.SiLU, **cfg)
    torch.manual_seed(3)
    ref = ScoreUNet(channels=6, spatial=2, activation=torch.nn.SiLU, **cfg)
    tr = Trainer(net, lr=1e-3, precision="fp16", ema_rates=[0.9], init_scale=256.0, growth_interval=2)
    tr32 = Trainer(ref, lr=1e-3, precision="fp32", ema_rates=[0.9])
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(2, 6, 16, 16, generator=gen)
    t, eps = torch.rand(2, generator=gen), torch.randn(2, 6, 16, 16, generator=gen)
    assert tr.scaler.tolist() == [256.0, 0.0, 0.0, 0.0]
    l16, l32 = tr.step(x, t=t, eps=eps), tr32.step(x, t=t, eps=eps)
    assert abs(float(l16) - float(l32)) <= 5e-3 * float(l32)
    assert tr.scaler.tolist() == [256.0, 1.0, 0.0, 1.0] and tr.optimizer_steps_taken() == 1
    for (k, a), (_, b) in zip(net.named_parameters(), ref.named_parameters()):
        assert (a - b).abs().max().item() <= 2.1e-3, k  # Adam's first step is +-lr: a flipped sign of a ~0 gradient costs 2 lr
    before = {k: v.clone() for k, v in net.state_dict().items()}
    ema_before = tr.ema_flats[0].clone()
    # poison one activation-gradient path: an inf input makes every gradient non-finite -> step skipped, scale halved
    tr.step(torch.full_like(x, float("inf")), t=t, eps=eps)
    assert tr.scaler.tolist() == [128.0, 0.0, 0.0, 1.0] and tr.optimizer_steps_taken() == 1 and tr.step_count == 3 - 1
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert not torch.equal(tr.ema_flats[0], ema_before)  # ema.update still ran (training_loop.py:387-389)
    tr.step(x, t=t, eps=eps)
    tr.step(x, t=t, eps=eps)
    assert tr.scaler.tolist() == [256.0, 0.0, 0.0, 3.0] and tr.loss_scale() == 256.0
    osd = tr.optimizer_state_dict()
    assert float(osd["state"][0]["step"]) == 3.0


@pytest.mark.parametrize("bucket_mb", [48.0, 0.05])
def test_ddp_two_ranks_gloo_equals_single_process(golden_dir, tmp_path, bucket_mb):
    import torch.multiprocessing as mp
    from _ddp_worker import run
    mp.spawn(run, args=(2, _free_port(), golden_dir, str(tmp_path), bucket_mb), nprocs=2, join=True)
    g = _golden(golden_dir, "tiny_net.npz")
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt", weights_only=False) for r in (0, 1))
    if bucket_mb < 1:
        assert r0["nb"] > 4  # several buckets chased the backward
    exp = _oracle_step(g, 1e-3)  # golden grads are of the mean loss over the global batch of 2 = mean of per-rank means
    for k, v in r0["sd"].items():
        assert torch.equal(v, r1["sd"][k]), k  # ranks stay in lock step
        _assert_adam_close(v, exp[k], torch.from_numpy(g["grad." + k]), 1e-3, k)
    assert 0.5 * (r0["loss"] + r1["loss"]) == pytest.approx(float(g["loss"]), rel=1e-5)
    # identical caller-side seeding on both ranks: the trainers' noise / t streams still differ by rank
    assert r0["draws"]["seed"] != r1["draws"]["seed"] and not torch.equal(r0["draws"]["t"], r1["draws"]["t"])


def test_optimizer_chasing_the_backward_equals_the_update_behind_it_two_ranks_gloo(golden_dir, tmp_path):
    """Trainer.chase_optimizer with several buckets on two ranks: all-reduce + fused AdamW + EMA per finished bucket,
    issued from inside the backward, against the whole-buffer update behind it -- same weights and EMA after two steps, on both
    ranks; the chasing run really updated bucket by bucket."""
    import torch.multiprocessing as mp
    from _ddp_worker import run_chase
    mp.spawn(run_chase, args=(2, _free_port(), golden_dir, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"chase{r}.pt", weights_only=False) for r in (0, 1))
    for r in (r0, r1):
        assert r[True]["update_calls"] > 2 * 4 and r[False]["update_calls"] == 2
        for k, v in r[False]["sd"].items():
            assert torch.equal(v, r[True]["sd"][k]), k
        assert torch.equal(r[False]["ema"], r[True]["ema"])
        assert r[False]["loss"] == r[True]["loss"]
    for k, v in r0[True]["sd"].items():
        assert torch.equal(v, r1[True]["sd"][k]), k  # ranks in lock step


@pytest.mark.parametrize("wire,chase", [(None, False), ("bf16", False), (None, True), ("bf16", True)])
def test_bucket_collectives_never_make_the_compute_stream_wait(emu, golden_dir, monkeypatch, wire, chase):
    """training_loop.py:116,373-378 on one backward stream (the default since round 5): every bucket's cast / all-reduce / stream-side
    wait / cast back / chased update is enqueued on the COMMUNICATION stream, ordered behind the bucket's weight gradients by
    comm.wait_stream(compute); the compute stream waits for the communication stream exactly once, behind the last bucket.  Streams
    and the collective are recording stand-ins (no GPU here); the step's numbers must equal the step without a process group."""
    import torch.distributed as dist
    from climate2weather_amd import training as tmod
    g = _golden(golden_dir, "tiny_net.npz")
    x, t, eps = (torch.from_numpy(g[k]) for k in ("x", "t", "eps"))
    log = []

    class FakeStream:
        def __init__(self, name):
            self.name = name

        def wait_stream(self, other):
            log.append(("wait_stream", self.name, other.name))

    main, comm = FakeStream("compute"), FakeStream("comm")
    stack = [main]

    class Ctx:
        def __init__(self, st):
            self.st = st

        def __enter__(self):
            stack.append(self.st)

        def __exit__(self, *a):
            stack.pop()

    class FakeWork:
        def wait(self):
            log.append(("work.wait", stack[-1].name))

    def fake_all_reduce(tensor, op=None, group=None, async_op=False):
        log.append(("all_reduce", stack[-1].name, str(tensor.dtype)))
        return FakeWork()

    ref = Trainer(_tiny(), lr=1e-3, precision="fp32", ema_rates=[0.9], bucket_mb=0.05)
    ref.step(x, t=t.reshape(-1), eps=eps)

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    try:
        monkeypatch.setenv("C2W_FORCE_DIST", "1")
        tr = Trainer(_tiny(), lr=1e-3, precision="fp32", ema_rates=[0.9], bucket_mb=0.05, allreduce_dtype=wire)
        assert tr.sync_grads and len(tr.buckets) > 4
        tr.chase_optimizer = chase
        monkeypatch.setattr(tmod, "_current_stream", lambda dev: stack[-1])
        monkeypatch.setattr(tmod, "_stream_ctx", Ctx)
        want_comm = bool(wire) or chase  # plain fp32 wire: asynchronous collectives from the compute stream, waited for at the end only
        monkeypatch.setattr(Trainer, "_comm_stream", lambda self: comm if self._wants_comm_stream() else None)  # the product's decision, a stand-in stream
        assert (tr.wire is not None) == bool(wire)
        monkeypatch.setattr(dist, "all_reduce", fake_all_reduce)
        updates = []
        orig_update = Trainer._update_range
        monkeypatch.setattr(Trainer, "_update_range", lambda self, s, e, *a: (updates.append(stack[-1].name), orig_update(self, s, e, *a))[1])
        tr.step(x, t=t.reshape(-1), eps=eps)
    finally:
        dist.destroy_process_group()
    nb = len(tr.buckets)
    ars = [i for i, ev in enumerate(log) if ev[0] == "all_reduce"]
    waits = [i for i, ev in enumerate(log) if ev[0] == "work.wait"]
    assert len(ars) == nb and len(waits) == nb
    assert {log[i][2] for i in ars} == {"torch.bfloat16" if wire else "torch.float32"}
    if want_comm:
        assert all(log[i][1] == "comm" for i in ars) and all(log[i][1] == "comm" for i in waits)  # never the compute stream
        joins = [i for i, ev in enumerate(log) if ev == ("wait_stream", "compute", "comm")]
        assert len(joins) == 1 and joins[0] > ars[-1]  # the one join sits behind the last bucket's collective
        orders = [i for i, ev in enumerate(log) if ev == ("wait_stream", "comm", "compute")]
        assert len(orders) > 4 and orders[0] < ars[0]  # buckets were handed over during the backward, each behind an event of the compute stream
        for a in ars:  # every collective is preceded by a hand-over
            assert any(o < a for o in orders)
        assert waits[0] < ars[-1]  # the waits sit next to their collectives (inside the backward) -- on the communication stream
    else:  # asynchronous collectives from the compute stream: no wait of any kind before the last bucket's collective is out
        assert all(log[i][1] == "compute" for i in ars) and waits[0] > ars[-1]
        assert not [ev for ev in log if ev[0] == "wait_stream"]
    assert (len(updates) == nb and set(updates) == {"comm"}) if chase else updates == ["compute"]
    if wire is None:
        assert torch.equal(tr.eng.flat, ref.eng.flat) and torch.equal(tr.ema_flats[0], ref.ema_flats[0])
    else:  # the gradients went through 8 mantissa bits: one Adam step of lr 1e-3 moves a weight by at most a flipped sign
        assert not torch.equal(tr.eng.flat_grad, ref.eng.flat_grad) and (tr.eng.flat - ref.eng.flat).abs().max().item() <= 2.1e-3


def _check_wire(outs):
    """bf16 wire vs fp32 wire of the gradient all-reduce (tests/_ddp_worker.py::run_wire): per-bucket bf16 collectives, summed gradients
    within bf16's resolution of the fp32 sum (scale-relative per 4096-element block of the flat buffer), untouched loss, ranks in lock step."""
    for r in outs:
        f, b = r["fp32"], r["bf16"]
        assert f["dtypes"] == ["torch.float32"] and b["dtypes"] == ["torch.bfloat16"] and b["all_reduces"] == f["all_reduces"] == f["nb"] > 4
        assert abs(f["loss"] - b["loss"]) <= 1e-6 * abs(f["loss"])  # computed before any gradient moves (GPU: fp32 atomics in the loss sum)
        gf, gb = f["grad"], b["grad"]
        n = gf.numel() // 4096 * 4096
        blocks_f, blocks_b = gf[:n].view(-1, 4096), gb[:n].view(-1, 4096)
        scale = blocks_f.abs().amax(dim=1).clamp_min(1e-30)
        assert ((blocks_f - blocks_b).abs().amax(dim=1) / scale).max().item() <= 2 ** -7
        assert not torch.equal(gf, gb)  # it really went through 8 mantissa bits
        assert (f["flat"] - b["flat"]).abs().max().item() <= 2.1e-3  # one Adam step of lr 1e-3: at most a sign flip where |g| ~ 0
    for r in outs[1:]:
        assert torch.equal(outs[0]["bf16"]["flat"], r["bf16"]["flat"])  # every rank applied the same reduced gradient


def test_bf16_wire_format_of_the_gradient_all_reduce_two_ranks_gloo(golden_dir, tmp_path):
    """Trainer(allreduce_dtype="bf16"): 144 MB instead of 288 MB per step on the xGMI links for the default network."""
    import torch.multiprocessing as mp
    from _ddp_worker import run_wire
    mp.spawn(run_wire, args=(2, _free_port(), golden_dir, str(tmp_path)), nprocs=2, join=True)
    _check_wire([torch.load(tmp_path / f"wire{r}.pt", weights_only=False) for r in (0, 1)])


def test_score_function_and_sampler_match_golden(emu, golden_dir):
    s = _golden(golden_dir, "sampler.npz")
    net = _tiny().eval()
    pipe = SDAPipeline()
    k = 1
    x = torch.from_numpy(s["score_x"])
    for sf in (DefaultScoreFunction(net, markov_order=k, noise_process=pipe),
               BatchedScoreFunction(net, markov_order=k, batch_size=4, device=torch.device("cpu"), noise_process=pipe)):
        with torch.no_grad():
            y = sf(x, torch.tensor(0.7))
        assert torch.allclose(y, torch.from_numpy(s["score_y"]), atol=2e-5)
        # reference helper methods keep working
        assert torch.equal(sf.fold(sf.unfold(x)), x)
    y_obs, std, gamma = torch.from_numpy(s["y_obs"]), torch.from_numpy(s["std"]), float(s["gamma"])

    def A_generic(z):
        return F.avg_pool2d(z[::2], 8)

    for name, corrections, cond, exact, A in [("uncond_c0", 0, False, False, None), ("uncond_c1", 1, False, False, None),
                                              ("cond_c0", 0, True, False, PoolStrideOperator(8, 2)),  # fused guidance kernel
                                              ("cond_c0", 0, True, False, A_generic),  # generic operator -> autograd
                                              ("cond_c1_exact", 1, True, True, PoolStrideOperator(8, 2))]:
        sf = BatchedScoreFunction(net, markov_order=k, batch_size=4, device=torch.device("cpu"), noise_process=pipe)
        if cond:
            sf.condition_on(A=A, y=y_obs, std=std, gamma=gamma, exact_grad=exact)
        zs = [torch.from_numpy(z) for z in s[name + ".z"]] if corrections else None
        for fused in (True, False):
            sf.device_resident = fused  # fused HIP update kernels vs the reference's torch update rule
            dev = torch.device("cpu")
            xs = _sample(pipe, sf, torch.from_numpy(s[name + ".noise"]), corrections, zs, dev, fused)
            ref = torch.from_numpy(s[name + ".x"])
            assert (xs - ref).abs().max().item() <= 3e-4 * ref.abs().max().item(), (name, fused)


def test_condition_on_per_variable_gamma_matches_reference(emu, golden_dir):
    """condition_on(gamma=<(1, F, 1, 1) tensor>) -- what exp/downscaling.py:228-233 builds for a list-valued likelihood_gamma and
    src/thor/score.py:55 broadcasts -- on the fused guidance kernel, on the generic operator route and with exact_grad=True, against
    trajectories of the imported reference (tests/golden/sampler_gamma.npz)."""
    s, sg = _golden(golden_dir, "sampler.npz"), _golden(golden_dir, "sampler_gamma.npz")
    net = _tiny().eval()
    pipe = SDAPipeline()
    y_obs, std, gamma = torch.from_numpy(s["y_obs"]), torch.from_numpy(s["std"]), torch.from_numpy(sg["gamma"])

    def A_generic(z):
        return F.avg_pool2d(z[::2], 8)

    for name, corrections, exact, A, fused_kernel in [("cond_c0_gvec", 0, False, PoolStrideOperator(8, 2), True),
                                                      ("cond_c0_gvec", 0, False, A_generic, False),
                                                      ("cond_c1_gvec_exact", 1, True, PoolStrideOperator(8, 2), False)]:
        sf = BatchedScoreFunction(net, markov_order=1, batch_size=4, device=torch.device("cpu"), noise_process=pipe)
        sf.condition_on(A=A, y=y_obs, std=std, gamma=gamma, exact_grad=exact)
        assert (sf._fused_guidance is not None) == fused_kernel
        zs = [torch.from_numpy(z) for z in sg[name + ".z"]] if corrections else None
        for fused in (True, False):
            sf.device_resident = fused
            xs = _sample(pipe, sf, torch.from_numpy(s["cond_c0.noise"]), corrections, zs, torch.device("cpu"), fused)
            ref = torch.from_numpy(sg[name + ".x"])
            assert (xs - ref).abs().max().item() <= 3e-4 * ref.abs().max().item(), (name, fused)
    # one guided evaluation; a gamma that is neither a scalar nor per variable (here per pixel) takes the autograd route
    sf = BatchedScoreFunction(net, markov_order=1, batch_size=4, device=torch.device("cpu"), noise_process=pipe)
    sf.condition_on(A=PoolStrideOperator(8, 2), y=y_obs, std=std, gamma=gamma, exact_grad=False)
    out = sf(torch.from_numpy(s["score_x"]), torch.tensor(0.7))
    ref = torch.from_numpy(sg["score_guided_gvec"])
    assert (out - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()
    sf.condition_on(A=PoolStrideOperator(8, 2), y=y_obs, std=std, gamma=torch.full((1, 1, 4, 4), 0.01), exact_grad=False)
    assert sf._fused_guidance is None
    sf(torch.from_numpy(s["score_x"]), torch.tensor(0.7))


def test_fused_guidance_only_for_per_variable_std(emu, golden_dir):
    """The guidance kernel indexes std by variable.  Any other broadcastable shape (src/thor/score.py:55 broadcasts ``std**2``
    like any tensor) must take the generic autograd route and give what the reference's formula gives -- here a per-pixel std
    of shape (1, 1, h, w), and a 1-D (w,) std that broadcasts along the LAST axis, not over the variables."""
    from climate2weather_amd.score_fn import per_channel_std
    s = _golden(golden_dir, "sampler.npz")
    net = _tiny().eval()
    pipe = SDAPipeline()
    y_obs, gamma = torch.from_numpy(s["y_obs"]), float(s["gamma"])
    nobs, Fv, h, w = y_obs.shape
    assert per_channel_std(torch.rand(1, Fv, 1, 1), y_obs).shape == (Fv,) and per_channel_std(0.3, y_obs).shape == (1,)
    x = torch.from_numpy(s["score_x"])
    t = torch.tensor(0.6)
    gen = torch.Generator().manual_seed(0)
    for std in (torch.rand(1, 1, h, w, generator=gen) + 0.1, torch.rand(w, generator=gen) + 0.1):
        assert per_channel_std(std, y_obs) is None
        A = PoolStrideOperator(8, 2)
        sf = BatchedScoreFunction(net, markov_order=1, batch_size=4, device=torch.device("cpu"), noise_process=pipe)
        sf.condition_on(A=A, y=y_obs, std=std, gamma=gamma, exact_grad=False)
        assert sf._fused_guidance is None
        out = sf(x, t)
        with torch.no_grad():
            eps = sf.score_fn(x, t)
        mu, sigma = pipe.mu(t), pipe.sigma(t)
        xg = x.clone().requires_grad_(True)
        err = y_obs - F.avg_pool2d(((xg - sigma * eps) / mu)[::2], 8)
        logp = -(err ** 2 / (std ** 2 + gamma * (sigma / mu) ** 2)).sum() / 2
        (J,) = torch.autograd.grad(logp, xg)
        assert torch.allclose(out, eps - sigma * J, atol=1e-5 * float((eps - sigma * J).abs().max()))
    from climate2weather_amd.sharded import TimeShardedScoreFunction
    ts = TimeShardedScoreFunction(net, 1, length=9, batch_size=4, device=torch.device("cpu"), noise_process=pipe, rank=0, world=1)
    with pytest.raises(NotImplementedError):
        ts.condition_on(A=PoolStrideOperator(8, 2), y=y_obs, std=torch.rand(1, 1, h, w) + 0.1, gamma=gamma)


def _sample(pipe, sf, noise, corrections, zs, dev, fused):
    import climate2weather_amd.pipelines as pl
    if fused:  # the fused branch is gated on a cuda device; exercise its logic on the emulator
        class _Dev:
            type = "cuda"
        orig = torch.device
        try:
            pl.torch.device = lambda d: _Dev() if not isinstance(d, _Dev) else d  # type: ignore
            sf.device = orig("cpu")
            return _run_fused(pipe, sf, noise, corrections, zs)
        finally:
            pl.torch.device = orig
    return pipe.sample(sf, noise, steps=4, corrections=corrections, tau=0.5, device=dev, show_progressbar=False, z_draws=zs)


def _run_fused(pipe, sf, noise, corrections, zs):
    # same loop as SDAPipeline.sample's fused branch, driven directly (tensors stay on the CPU emulator)
    import math
    x = noise.clone()
    steps, tau, dt = 4, 0.5, 0.25
    ts = torch.linspace(1, 0, steps + 1).tolist()
    flag = torch.zeros(1, dtype=torch.int32)
    sumsq = torch.zeros(1)
    zi = iter(zs) if zs else None
    n = x.numel()
    with torch.no_grad():
        for i in range(steps):
            t = torch.tensor(ts[i])
            eps = sf(x, t)
            mu_t, sg_t = pipe._mu_sigma_f(ts[i])
            mu_n, sg_n = pipe._mu_sigma_f(ts[i] - dt)
            c2w_ops.sampler_predict(x, eps, flag, n, mu_n / mu_t, sg_n - mu_n * sg_t / mu_t)
            for _ in range(corrections):
                z = next(zi)
                eps = sf(x, t - dt)
                sumsq.zero_()
                c2w_ops.sumsq(eps, sumsq, n)
                c2w_ops.sampler_correct(x, eps, z, sumsq, flag, n, tau, sg_n)
    assert int(flag) == 0
    return x


def test_time_sharded_sampler_two_ranks_equals_reference_trajectory(golden_dir, tmp_path):
    """the trajectory's time axis split over 2 ranks (k-frame halo exchange, scalar all-reduce for the
    corrector, frame-local guidance) reproduces the single-process trajectories of the imported reference."""
    import torch.multiprocessing as mp
    from _shard_worker import run
    mp.spawn(run, args=(2, _free_port(), golden_dir, str(tmp_path)), nprocs=2, join=True)
    s = _golden(golden_dir, "sampler.npz")
    r0, r1 = (torch.load(tmp_path / f"shard{r}.pt", weights_only=False) for r in (0, 1))
    assert r0["uncond_c0.bounds"] == [(0, 5), (5, 9)]
    sg = _golden(golden_dir, "sampler_gamma.npz")  # per-variable gamma as exp/downscaling.py:228-233 builds it
    for name in ("uncond_c0", "uncond_c1", "cond_c0", "cond_c0_gvec", "cond_c1_exact"):
        ref = torch.from_numpy(sg[name + ".x"] if name.endswith("_gvec") else s[name + ".x"])
        assert torch.equal(r0[name], r1[name]), name  # gather=True: every rank holds the whole trajectory
        assert (r0[name] - ref).abs().max().item() <= 3e-4 * ref.abs().max().item(), name
        if name == "cond_c0":  # interior windows evaluated while the halos were in flight == halos waited for first
            assert (r0[name] - r0[name + ".no_overlap"]).abs().max().item() <= 1e-5 * ref.abs().max().item(), name


def test_time_sharded_partition_and_single_rank(emu, golden_dir):
    from climate2weather_amd.sharded import TimeShardedScoreFunction, partition_frames, sample_time_sharded
    assert partition_frames(49, 4, 6) == [(0, 13), (13, 25), (25, 37), (37, 49)]
    assert partition_frames(8737, 8, 6)[-1] == (7645, 8737)
    with pytest.raises(ValueError):
        partition_frames(20, 8, 6)  # a rank would own fewer than k frames
    s = _golden(golden_dir, "sampler.npz")
    net = _tiny().eval()
    pipe = SDAPipeline()
    noise = torch.from_numpy(s["uncond_c0.noise"])
    sf = TimeShardedScoreFunction(net, markov_order=1, length=9, batch_size=4, device=torch.device("cpu"), noise_process=pipe, rank=0, world=1)
    x = sample_time_sharded(pipe, sf, noise, steps=4)
    ref = torch.from_numpy(s["uncond_c0.x"])
    assert (x - ref).abs().max().item() <= 3e-4 * ref.abs().max().item()
    with pytest.raises(NotImplementedError):
        sf.condition_on(A=lambda z: z, y=None, std=1.0)


def test_nan_detection_raises(emu):
    net = _tiny().eval()
    pipe = SDAPipeline()
    sf = DefaultScoreFunction(net, markov_order=1, noise_process=pipe)
    sf.device_resident = False
    noise = torch.randn(5, 2, 16, 16)
    noise[0, 0, 0, 0] = float("nan")
    with pytest.raises(ValueError, match="NaN detected"):
        pipe.sample(sf, noise, steps=2, show_progressbar=False)


def test_ema_module_api(emu, golden_dir):
    g = _golden(golden_dir, "ema.npz")
    torch.manual_seed(4)
    lin = torch.nn.Linear(4, 3)
    ema = StandardEMA(lin, rates=[0.9, 0.999])
    with torch.no_grad():
        for p in lin.parameters():
            p.add_(1.0)
    ema.update()
    assert torch.allclose(ema.emas[0].weight, torch.from_numpy(g["ema_0.9"]), atol=1e-6)
    assert torch.allclose(ema.emas[1].weight, torch.from_numpy(g["ema_0.999"]), atol=1e-6)
    assert [tag for _, tag in ema.get()] == ["-0.900000", "-0.999000"]
    # engine-backed network: fused flat update gives the same numbers
    net = _tiny()
    e2 = StandardEMA(net, rates=[0.5])
    before = {k: v.clone() for k, v in net.state_dict().items()}
    net._get_engine()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(3.0)
    e2.update()
    for k, v in e2.emas[0].state_dict().items():
        assert torch.allclose(v, 0.5 * before[k] + 0.5 * 3.0 * before[k], atol=1e-6), k
    sd = e2.state_dict()
    e2.load_state_dict(sd)


@pytest.mark.parametrize("N,rank,R,seed,start", [(10, 0, 1, 0, 0), (7, 1, 3, 5, 2), (13, 3, 4, 42, 100), (5, 0, 7, 1, 3), (1, 0, 1, 0, 0), (64, 1, 2, 0, 0)])
def test_cursor_sampler_is_the_reference_index_stream(N, rank, R, seed, start):
    """InfiniteSampler as a vectorised cursor (take / positions / iteration in blocks) yields exactly the stream oracle/host.py restates
    from dataset.py:28-40 -- across epoch boundaries, for strides larger than the dataset, ragged take() sizes, and through the
    device-side gather of DeviceWindowFeed (an epoch's permutation uploaded once, a batch = perm[off + arange * stride])."""
    class _D:
        data = torch.zeros(N + 2, 1, 2, 2)
        window = 3

        def __len__(self):
            return N
    want = oh.infinite_order(N, rank, R, seed, start, 200)
    s = InfiniteSampler(_D(), rank, R, True, seed, start)
    got = []
    for k in (1, 3, 17, 64, 115):
        got += s.take(k).tolist()
    assert got == want
    it = iter(InfiniteSampler(_D(), rank, R, True, seed, start))
    assert [next(it) for _ in range(200)] == want
    it2 = iter(s)  # a fresh iterator starts over (dataset.py:28: idx = self.start_idx), whatever take() has consumed
    assert [next(it2) for _ in range(50)] == want[:50] and s.take(1).tolist() == oh.infinite_order(N, rank, R, seed, start, 201)[200:]
    feed = DeviceWindowFeed(_D(), torch.device("cpu"), rank=rank, num_replicas=R, seed=seed, start_idx=start)
    got = []
    for k in (5, 1, 30, 64):
        got += feed.next_batch(k, lazy=True).first.tolist()
    assert got == want[:100]


def test_data_feed_and_seam(golden_dir):
    kat = json.load(open(os.path.join(golden_dir, "kat.json")))
    ds = SyntheticWindowDataset(n_frames=12, n_vars=2, height=8, width=8, window=3, seed=0)
    assert len(ds) == 10
    it = iter(InfiniteSampler(ds, rank=0, num_replicas=1, seed=0))
    assert [next(it) for _ in range(10)] == kat["shuffle10_seed0_epoch0"]
    it1 = iter(InfiniteSampler(ds, rank=1, num_replicas=2, seed=0, start_idx=2))
    full = kat["shuffle10_seed0_epoch0"]
    assert [next(it1) for _ in range(3)] == [full[3], full[5], full[7]]
    item = ds[4]
    assert item.shape == (6, 8, 8) and torch.equal(item, oh.window_item(ds.data, 4, 3))
    feed = DeviceWindowFeed(ds, torch.device("cpu"), rank=0, num_replicas=1, seed=0)
    batch = feed.next_batch(4)
    for j, idx in enumerate(full[:4]):
        assert torch.equal(batch[j], ds[idx])
    lazy = DeviceWindowFeed(ds, torch.device("cpu"), rank=0, num_replicas=1, seed=0).next_batch(4, lazy=True)  # indices only
    assert tuple(lazy.shape) == (4, 6, 8, 8) and lazy.first.tolist() == full[:4] and torch.equal(lazy.materialize(), batch)
    assert lazy.offsets().tolist() == [i * 2 * 64 for i in full[:4]]  # float offset of each window inside the (N, F, H, W) array
    assert c2w_util.set_random_seed(42, 0) == kat["seed_hash"]["42,0"]
    assert linear_learning_rate_schedule(250, 1000, 1e-4) == pytest.approx(kat["lr_linear"][1])
    net = c2w_util.construct_class_by_name(class_name="climate2weather_amd.score.ScoreUNet", channels=6, spatial=2,
                                           activation=torch.nn.SiLU, **TINY)
    assert isinstance(net, ScoreUNet)
    pipe = c2w_util.construct_class_by_name(class_name="climate2weather_amd.pipelines.SDAPipeline")
    t = torch.tensor(kat["timestep_embedding_t"])
    assert torch.allclose(pipe.mu(t), torch.tensor(kat["mu"]), atol=1e-7)
    assert torch.allclose(pipe.sigma(t), torch.tensor(kat["sigma"]), atol=1e-7)
    for tv, m, sg in zip(kat["timestep_embedding_t"], kat["mu"], kat["sigma"]):
        a, b = pipe._mu_sigma_f(tv)
        assert a == pytest.approx(m, abs=1e-6) and b == pytest.approx(sg, abs=1e-6)


def test_c_abi_library_exports_every_declared_symbol():
    import re
    from climate2weather_amd import _lib
    from climate2weather_amd import build as c2w_build
    c2w_build.build(verbose=False)  # no-op when libc2w_hip.so is up to date; hipcc cross-compiles gfx950 without a GPU
    lib = _lib.load()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "c2w_hip.h")).read()
    declared = set(re.findall(r"\b(c2w_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.exported_symbols()), declared ^ set(_lib.exported_symbols())
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.c2w_target() == b"gfx950"
    with pytest.raises(_lib.C2wError):
        c2w_ops.silu(torch.zeros(8), torch.zeros(8), 8, 0)  # CPU tensors are refused: no fallback path


def test_reference_network_snapshot_import_and_round_trip(emu, golden_dir, tmp_path):
    """a `network-snapshot-*.pkl` written by the reference (fixture made by tests/golden/make_snapshot.py
    from the imported reference classes) loads without the reference's packages; an own snapshot round-trips; pickles that
    reach outside the allow-list are refused."""
    import pickle
    from climate2weather_amd.snapshot import infer_config, load_network_snapshot, save_network_snapshot
    g = _golden(golden_dir, "tiny_net.npz")
    snap = load_network_snapshot(os.path.join(golden_dir, "ref_snapshot_tiny.pkl"))
    assert isinstance(snap.ema, ScoreUNet) and isinstance(snap.pipeline, SDAPipeline)
    assert snap.markov_order == 1 and snap.pipeline.eta == pytest.approx(1e-3)
    assert snap.dataset_kwargs["train"]["window"] == 3
    sd = snap.ema.state_dict()
    assert list(sd.keys()) == [str(n) for n in g["param_order"]] or set(sd.keys()) == {str(n) for n in g["param_order"]}
    for k, v in sd.items():
        ref = torch.from_numpy(g["sd." + k]).to(torch.float16).float()  # the reference stores fp16 (training_loop.py:259)
        assert torch.equal(v, ref), k
    assert infer_config(sd) == dict(channels=6, spatial=2, **TINY)
    # the imported network runs (emulated launchers here, HIP on the GPU) and is close to the fp32 golden output
    with torch.no_grad():
        y = snap.ema(torch.from_numpy(g["xt"]), torch.from_numpy(g["t"]))
    assert (y - torch.from_numpy(g["y"])).abs().max().item() <= 2e-2 * float(np.abs(g["y"]).max())
    # own snapshot: same container, this package's classes
    p = save_network_snapshot(str(tmp_path / "network-snapshot-0000001.pkl"), snap.ema, snap.pipeline, snap.dataset_kwargs)
    again = load_network_snapshot(p)
    for (k, a), (_, b) in zip(sd.items(), again.ema.state_dict().items()):
        assert torch.equal(a, b), k
    evil = tmp_path / "evil.pkl"
    with open(evil, "wb") as f:
        pickle.dump(dict(ema=os.system), f)
    with pytest.raises(pickle.UnpicklingError):
        load_network_snapshot(str(evil))
    # protocol-4 STACK_GLOBAL with a dotted name through an allowed module ("torch.serialization", "os.system"), and getattr chains
    marker = tmp_path / "pwned"
    for mod, name in (("torch.serialization", "os.system"), ("torch", "serialization.os.system"), ("builtins", "getattr"),
                      ("builtins", "eval"), ("torch.hub", "load"), ("numpy", "load"), ("torch", "load")):
        arg = f"touch {marker}"
        payload = (b"\x80\x04" + b"\x8c" + bytes([len(mod)]) + mod.encode() + b"\x8c" + bytes([len(name)]) + name.encode() + b"\x93"
                   + b"\x8c" + bytes([len(arg)]) + arg.encode() + b"\x85R.")
        with open(evil, "wb") as f:
            f.write(payload)
        with pytest.raises(pickle.UnpicklingError):
            load_network_snapshot(str(evil))
        assert not marker.exists()
    # a storage payload is a nested torch.save stream: it must go through the weights-only loader, not a second full unpickler
    class _Boom:
        def __reduce__(self):
            return (os.system, (f"touch {marker}",))
    import io
    inner = io.BytesIO()
    torch.save(_Boom(), inner, _use_new_zipfile_serialization=False)
    mod, name = "torch.storage", "_load_from_bytes"
    blob = inner.getvalue()
    payload = (b"\x80\x04" + b"\x8c" + bytes([len(mod)]) + mod.encode() + b"\x8c" + bytes([len(name)]) + name.encode() + b"\x93"
               + b"B" + len(blob).to_bytes(4, "little") + blob + b"\x85R.")
    with open(evil, "wb") as f:
        f.write(payload)
    with pytest.raises(Exception):
        load_network_snapshot(str(evil))
    assert not marker.exists()


def test_quantile_normalizer_and_measurement_operator(emu):
    """data/pipeline.py:183-244 (five affine modes) and exp/downscaling.py:129-132 against the oracle and
    hand-computed values."""
    from climate2weather_amd.normalize import QuantileNormalizer
    q = {0.0: [-5.0, 0.0], 0.01: [-4.0, 0.5], 0.05: [2.0, 1.0], 0.25: [4.0, 2.0], 0.5: [6.0, 3.0], 0.75: [9.0, 5.0], 0.95: [12.0, 9.0],
         0.99: [16.0, 10.5], 1.0: [20.0, 12.0]}
    x = torch.full((3, 2, 4, 4), 7.0)
    expect = {"minmax": [(7 + 5) / 25, 7 / 12], "robust": [(7 - 6) / 5, (7 - 3) / 3], "robust95": [(7 - 6) / 10, (7 - 3) / 8],
              "quant95": [(7 - 2) / 10, (7 - 1) / 8], "quant99": [(7 + 4) / 20, (7 - 0.5) / 10]}
    gen = torch.Generator().manual_seed(0)
    xr = torch.randn(5, 2, 8, 8, generator=gen) * 3 + 4
    for mode, vals in expect.items():
        qn = QuantileNormalizer(q, mode)
        y = qn.normalize(x)
        assert torch.allclose(y[:, 0], torch.full_like(y[:, 0], vals[0]), atol=1e-6), mode
        assert torch.allclose(y[:, 1], torch.full_like(y[:, 1], vals[1]), atol=1e-6), mode
        assert torch.allclose(oh.normalize(x, q, mode), y, atol=1e-6)
        assert torch.allclose(qn.normalize(xr), oh.normalize(xr, q, mode), atol=1e-5)
        assert torch.allclose(qn.unnormalize(xr), oh.unnormalize(xr, q, mode), atol=1e-5)
        assert torch.allclose(qn.unnormalize(qn.normalize(xr)), xr, atol=1e-4)
    with pytest.raises(ValueError, match="Invalid mode"):
        QuantileNormalizer(q, "zscore")
    A = PoolStrideOperator(4, 2)
    assert torch.allclose(A(xr), oh.measure(xr, 4, 2), atol=1e-6) and A(xr).shape == (3, 2, 2, 2)


def test_cosmo_dataset_contract(tmp_path):
    """dataset.py:60-126 item contract over an in-memory / .npy array, feeding the device-resident feed."""
    from climate2weather_amd.data import COSMODataset
    arr = np.random.RandomState(0).randn(20, 4, 16, 16).astype(np.float32)
    np.save(tmp_path / "train.npy", arr)
    for src in (str(tmp_path / "train.npy"), arr):
        ds = COSMODataset(src, num_features=4, spatial_res=16, window=13, flatten=True)
        assert len(ds) == 8 and ds.window == 13 and ds.num_features == 4 and ds.raw_data_shape == (20, 4, 16, 16)
        assert torch.equal(ds[3], oh.window_item(torch.from_numpy(arr), 3, 13))
        assert ds[3].shape == (52, 16, 16)
    with pytest.raises(AssertionError):
        COSMODataset(arr, num_features=5, spatial_res=16)
    feed = DeviceWindowFeed(ds, torch.device("cpu"), rank=1, num_replicas=2, seed=0)
    b = feed.next_batch(3)
    it = iter(InfiniteSampler(ds, rank=1, num_replicas=2, seed=0))
    for j in range(3):
        assert torch.equal(b[j], ds[next(it)])


def test_ensemble_driver_shards_members_by_rank(emu):
    """exp/downscaling.py:96-103,208-265: num_samples % world == 0, rank r generates members r*n .. (r+1)*n - 1, the RNG stream
    differs by rank through the seed, every member is a full trajectory; no collective."""
    from climate2weather_amd.sampling import run_ensemble
    net = _tiny().eval()
    kw = dict(length=5, n_vars=2, height=16, width=16, markov_order=1, num_samples=4, steps=2, batch_size=4, seed=7,
              device=torch.device("cpu"), precision="fp32")
    r0 = run_ensemble(net, world=2, rank=0, **kw)
    r1 = run_ensemble(net, world=2, rank=1, **kw)
    assert [i for i, _ in r0] == [0, 1] and [i for i, _ in r1] == [2, 3]
    for _, x in r0 + r1:
        assert x.shape == (5, 2, 16, 16) and torch.isfinite(x).all()
    assert not torch.equal(r0[0][1], r1[0][1]) and not torch.equal(r0[0][1], r0[1][1])
    again = run_ensemble(net, world=2, rank=1, **kw)
    assert all(torch.equal(a[1], b[1]) for a, b in zip(r1, again))  # same seed and rank -> same members
    seen = []
    run_ensemble(net, world=1, rank=0, on_sample=lambda i, x: seen.append(i), **dict(kw, num_samples=2))
    assert seen == [0, 1]
    with pytest.raises(AssertionError, match="divisible"):
        run_ensemble(net, world=2, rank=0, **dict(kw, num_samples=3))
    # conditioned members (the shipped experiment's operator)
    A = PoolStrideOperator(8, 2)
    truth = torch.rand(5, 2, 16, 16)
    rc = run_ensemble(net, world=1, rank=0, A=A, y=A(truth), std=torch.tensor([0.5, 0.5]).view(1, 2, 1, 1), gamma=1e-2, **dict(kw, num_samples=1))
    assert rc[0][1].shape == (5, 2, 16, 16)


def _oracle_members(sd, kw, rank, world, A=None, y=None, std=None, gamma=1e-2):
    """oracle/host.py::ensemble_members over the oracle's network, score function and sampler (CPU, fp32)."""
    fwd = lambda a, b: ou.score_unet_forward(sd, a, b, hidden_blocks=[1, 1], attention_levels=[1])
    score = od.GuidedScore(fwd, kw["markov_order"], A=(lambda z: oh.measure(z, A.s_step, A.t_step)) if A is not None else None, y=y, std=std,
                           gamma=gamma, exact_grad=False, batch_size=kw["batch_size"])
    shape = (kw["length"], kw["n_vars"], kw["height"], kw["width"])
    return oh.ensemble_members(lambda noise, zs: od.sample(score, noise, steps=kw["steps"], corrections=kw.get("corrections", 0),
                                                           tau=kw.get("tau", 0.5), z_draws=zs),
                               seed=kw["seed"], rank=rank, world=world, num_samples=kw["num_samples"], shape=shape, steps=kw["steps"],
                               corrections=kw.get("corrections", 0))


@pytest.mark.parametrize("corrections,cond", [(0, False), (1, False), (0, True)])
def test_ensemble_members_are_the_reference_members(emu, corrections, cond):
    """a14 parity: seed s, rank r, member i -> the member the reference's loop generates (exp/downscaling.py:96-103,248-265):
    process seeded with hash((seed, rank)), one CPU randn(L, C, H, W) per member in member order, corrector normals from the same
    CPU stream in the sampler's order.  2 ranks x 2 members, against oracle/host.py::ensemble_members, <= 3e-4 of scale."""
    from climate2weather_amd.sampling import run_ensemble
    net = _tiny().eval()
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    kw = dict(length=5, n_vars=2, height=16, width=16, markov_order=1, num_samples=4, steps=3, batch_size=2, seed=7, corrections=corrections,
              tau=0.5)
    cnd = {}
    if cond:
        A = PoolStrideOperator(8, 2)
        truth = torch.rand(5, 2, 16, 16, generator=torch.Generator().manual_seed(9))
        cnd = dict(A=A, y=A(truth), std=torch.tensor([0.5, 0.3]).view(1, 2, 1, 1), gamma=1e-2)
    for rank in (0, 1):
        mine = run_ensemble(net, world=2, rank=rank, device=torch.device("cpu"), precision="fp32", exact_grad=False, **kw, **cnd)
        ref = _oracle_members(sd, kw, rank, 2, **cnd)
        assert [i for i, _ in mine] == [i for i, _ in ref] == [2 * rank, 2 * rank + 1]
        for (_, a), (_, b) in zip(mine, ref):
            assert (a - b).abs().max().item() <= 3e-4 * b.abs().max().item()
    # the device stream is a different (opt-in) stream
    dev = run_ensemble(net, world=2, rank=0, device=torch.device("cpu"), precision="fp32", rng="device", **kw, **cnd)
    assert dev[0][1].shape == (5, 2, 16, 16)
    with pytest.raises(ValueError):
        run_ensemble(net, world=2, rank=0, device=torch.device("cpu"), precision="fp32", rng="philox", **kw)


@pytest.mark.parametrize("cond", [False, True])
def test_co_sampled_members_equal_members_sampled_one_by_one(emu, cond):
    """members_per_batch > 1 (extension for short trajectories: the members' windows share the network batches) changes
    nothing a member can see: same seed -> the same members as the reference's one-by-one loop (exp/downscaling.py:248-265),
    unconditioned and under the experiment's operator; with a corrector, given the same normals, each member's step size
    comes from its own mean(eps^2) (src/thor/pipelines.py:84)."""
    from climate2weather_amd.sampling import run_ensemble
    net = _tiny().eval()
    kw = dict(length=6, n_vars=2, height=16, width=16, markov_order=1, num_samples=3, steps=3, batch_size=5, seed=11,
              device=torch.device("cpu"), precision="fp32", world=1, rank=0)
    if cond:
        A = PoolStrideOperator(8, 2)
        kw.update(A=A, y=A(torch.rand(6, 2, 16, 16, generator=torch.Generator().manual_seed(2))),
                  std=torch.tensor([0.5, 0.3]).view(1, 2, 1, 1), gamma=1e-2, exact_grad=False)
    one = run_ensemble(net, members_per_batch=1, **kw)
    for group in (2, 3, 8, None):  # None = the default: without a corrector, as many members as reach the window floor
        co = run_ensemble(net, members_per_batch=group, **kw)
        assert [i for i, _ in co] == [0, 1, 2]
        for (_, a), (_, b) in zip(one, co):
            assert a.shape == b.shape == (6, 2, 16, 16)
            assert torch.allclose(a, b, atol=1e-5, rtol=1e-5)
    # the default really co-samples when the score function has a window floor (the suite runs with the floor off), and does not under a corrector
    shapes = []

    class Spy(SDAPipeline):
        def sample(self, score_fn, noise, **k2):
            shapes.append(tuple(noise.shape))
            return super().sample(score_fn, noise, **k2)
    monkey = pytest.MonkeyPatch()
    try:
        monkey.setenv("C2W_WINDOW_BATCH_FLOOR", "64")
        co = run_ensemble(net, Spy(), **kw)
        assert shapes == [(3, 6, 2, 16, 16)], shapes
        for (_, a), (_, b) in zip(one, co):
            assert torch.allclose(a, b, atol=1e-5, rtol=1e-5)
        shapes.clear()
        run_ensemble(net, Spy(), **dict(kw, corrections=1, steps=1))
        assert shapes == [(6, 2, 16, 16)] * 3, shapes
    finally:
        monkey.undo()
    # corrector: same normals -> same members
    pipe = SDAPipeline()
    sf = BatchedScoreFunction(net, markov_order=1, batch_size=4, device=torch.device("cpu"), noise_process=pipe)
    if cond:
        sf.condition_on(A=kw["A"], y=kw["y"], std=kw["std"], gamma=1e-2, exact_grad=False)
    g = torch.Generator().manual_seed(5)
    noise = torch.randn(2, 6, 2, 16, 16, generator=g)
    zs = [torch.randn(2, 6, 2, 16, 16, generator=g) for _ in range(2)]
    both = pipe.sample(sf, noise, steps=2, corrections=1, tau=0.4, device=torch.device("cpu"), show_progressbar=False, z_draws=zs)
    assert both.shape == (2, 6, 2, 16, 16)
    for m in range(2):
        alone = pipe.sample(sf, noise[m], steps=2, corrections=1, tau=0.4, device=torch.device("cpu"), show_progressbar=False,
                            z_draws=[z[m] for z in zs])
        assert torch.allclose(both[m], alone, atol=1e-5, rtol=1e-5)


def test_output_convolution_folds_inside_the_engine(emu):
    """engine.py::_fold_output: where the kernel's domain allows (top level of 64 / 128 channels, 8 x 16-pixel tiles) the sampler's
    network calls compute only the frames src/thor/score.py:76-88 keeps -- the centre frame of every window through ops.conv_center,
    the first / last window's other frames through the full convolution of that window -- and write them into the trajectory.  Same
    eps as scattering the full output rows, for one trajectory, for co-sampled members sharing batches, and for window ranges."""
    torch.manual_seed(5)
    net = ScoreUNet(channels=6, spatial=2, activation=torch.nn.SiLU, embedding_dim=32, hidden_channels=[64, 64], hidden_blocks=[1, 1],
                    attention_levels=[1], kernel_size=3, padding_mode="zeros").eval()
    eng = net._get_engine()
    calls = []
    real = c2w_ops.conv_center

    def spy(*a, **kw):
        calls.append(a[4])  # windows per launch
        return real(*a, **kw)
    c2w_ops.conv_center = spy
    try:
        sf = BatchedScoreFunction(net, markov_order=1, batch_size=3, device=torch.device("cpu"), noise_process=SDAPipeline())
        g = torch.Generator().manual_seed(9)
        for shape in ((7, 2, 16, 16), (2, 6, 2, 16, 16)):
            x = torch.randn(*shape, generator=g)
            eng.use_center_conv = True
            del calls[:]
            a = sf.score_fn(x, 0.6).clone()
            assert calls and sum(calls) == (shape[-4] - 2) * (shape[0] if len(shape) == 5 else 1)
            eng.use_center_conv = False
            del calls[:]
            b = sf.score_fn(x, 0.6).clone()
            assert not calls
            assert torch.allclose(a, b, atol=1e-5, rtol=1e-5)
        x = torch.randn(9, 2, 16, 16, generator=g)
        eng.use_center_conv = False
        want = sf.score_fn(x, 0.3).clone()
        eng.use_center_conv = True
        out = torch.zeros_like(x)
        sf.score_fn(x, 0.3, ranges=[(0, 2), (5, 2)], out=out)
        sf.score_fn(x, 0.3, ranges=[(2, 3)], out=out)
        assert torch.allclose(out, want, atol=1e-5, rtol=1e-5)
    finally:
        c2w_ops.conv_center = real
        eng.use_center_conv = True


@pytest.mark.parametrize("fused_loss", [False, True])
def test_parameter_gradients_are_delivered_in_segments_during_the_backward_pass(emu, monkeypatch, fused_loss):
    """score.py::_GradSegment: under torch's DistributedDataParallel (fabric.setup_module, training_loop.py:116) the reducer can only
    all-reduce a bucket once autograd has delivered its gradients.  With ``grad_segments`` the module's backward is a chain of nodes
    that hand finished ranges of the flat gradient buffer over while the rest of the pass is still to be enqueued: same gradients bit
    for bit as the single node, the output side's parameters first, and weight-gradient launches still to come when the first hooks fire."""
    x = torch.randn(2, 6, 16, 16, generator=torch.Generator().manual_seed(1))
    t = torch.tensor([0.3, 0.7])
    pipe = SDAPipeline()

    def run(net, xin):
        if fused_loss:
            torch.manual_seed(11)
            return pipe.loss(net=net, x=xin).mean()
        return net(xin, t).square().sum()
    a, b = _tiny().train(), _tiny().train()
    xa = x.clone().requires_grad_(not fused_loss)
    la = run(a, xa)
    la.backward()
    launches = []
    real = c2w_ops.conv_wgrad
    monkeypatch.setattr(c2w_ops, "conv_wgrad", lambda *a_, **kw: (launches.append(1), real(*a_, **kw))[1])
    b.grad_segments = 4
    order = []
    for n, p in b.named_parameters():
        p.register_hook(lambda g, n=n: order.append((n, len(launches))))
    xb = x.clone().requires_grad_(not fused_loss)
    lb = run(b, xb)
    assert torch.equal(la.detach(), lb.detach())
    lb.backward()
    total = len(launches)
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p.grad, q.grad), n
    if not fused_loss:
        assert torch.equal(xa.grad, xb.grad)
    names = [n for n, _ in order]
    assert sorted(names) == sorted(n for n, _ in b.named_parameters())  # every parameter exactly once
    first, last = order[0], order[-1]
    assert first[1] < total, "the first gradients are handed over before the last weight-gradient launch is enqueued"
    assert first[0].startswith("unet.") and last[1] == total
    assert any(n.startswith("map_layer") for n in names[-8:])  # the time-embedding MLP is differentiated last
    seen_at = sorted({k for _, k in order})
    assert len(seen_at) >= 3, seen_at  # at least three distinct points of the pass at which gradients arrived
    # a frozen network and functorch transforms keep the single node
    b.requires_grad_(False)
    assert b._segments(list(b.parameters()), x) == 1
    b.requires_grad_(True)
    assert b._segments(list(b.parameters()), x) == 4 and a._segments(list(a.parameters()), x) == 1


def test_input_gradient_of_a_frozen_network_launches_no_weight_gradient(emu, monkeypatch):
    """Exact guidance (src/thor/score.py:28-33, the API default exact_grad=True) differentiates the network with respect to its INPUT;
    the reference's sampler runs it on a snapshot saved with requires_grad_(False) (training_loop.py:253-265).  For such a network the
    backward pass runs the input-gradient chain only: same dx as with trainable parameters, no weight-gradient launch, no parameter
    .grad."""
    net = _tiny().eval()
    x = torch.randn(2, 6, 16, 16, generator=torch.Generator().manual_seed(1))
    t = torch.tensor([0.3, 0.7])
    xa = x.clone().requires_grad_(True)
    net(xa, t).square().sum().backward()
    assert all(p.grad is not None for p in net.parameters())
    calls = []
    real = c2w_ops.conv_wgrad
    monkeypatch.setattr(c2w_ops, "conv_wgrad", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    net.zero_grad(set_to_none=True)
    net.requires_grad_(False)
    xb = x.clone().requires_grad_(True)
    net(xb, t).square().sum().backward()
    assert not calls and all(p.grad is None for p in net.parameters())
    assert torch.equal(xa.grad, xb.grad)
    (gx,) = torch.autograd.grad(net(xb, t).square().sum(), xb)
    assert torch.equal(gx, xa.grad) and not calls
    net.requires_grad_(True)
    xc = x.clone().requires_grad_(True)
    net(xc, t).square().sum().backward()
    assert calls and all(p.grad is not None for p in net.parameters()) and torch.equal(xc.grad, xa.grad)


def test_window_batch_floor_is_a_lower_bound_on_the_launch_size(emu, monkeypatch):
    """score_fn.py::window_batch_floor: ``batch_size`` (src/thor/score.py:156-185, a memory bound) is a LOWER bound on the windows
    per network call on the engine path -- scaled by the field size, never more than the trajectory has -- and 0 restores exactly
    ``batch_size`` windows per call.  Same trajectory either way."""
    net = _tiny().eval()
    pipe = SDAPipeline()
    noise = torch.randn(9, 2, 16, 16, generator=torch.Generator().manual_seed(4))  # 7 windows of 3 frames
    eng = net._get_engine()
    calls = []
    real = eng.forward

    def spy(*a, **kw):
        calls.append(kw["shape"][0])
        return real(*a, **kw)
    monkeypatch.setattr(eng, "forward", spy)
    sf = BatchedScoreFunction(net, markov_order=1, batch_size=2, device=torch.device("cpu"), noise_process=pipe)
    assert sf.window_batch_floor == 0  # tests/conftest.py pins the suite to the reference's meaning
    exact = sf.score_fn(noise, 0.5)
    assert calls == [2, 2, 2, 1]
    del calls[:]
    sf.window_batch_floor = 256  # the product default: 256 windows of 128x128 = 16384 windows of 16x16 -> everything in one call
    assert sf._window_floor(16 * 16) == 256 * 64 and sf._window_floor(128 * 128) == 256 and sf._window_floor(256 * 256) == 64
    one = sf.score_fn(noise, 0.5)
    assert calls == [7]
    assert torch.allclose(one, exact, atol=1e-6, rtol=1e-6)
    del calls[:]
    monkeypatch.setattr(sf, "_window_floor", lambda pixels: 3)  # a floor between batch_size and the trajectory
    three = sf.score_fn(noise, 0.5)
    assert calls == [3, 3, 1]
    assert torch.allclose(three, exact, atol=1e-6, rtol=1e-6)
    del calls[:]
    monkeypatch.setattr(sf, "_window_floor", lambda pixels: 5)  # 7 windows in launches of at least 5: two equal ones, not 5 + 2
    two = sf.score_fn(noise, 0.5)
    assert calls == [4, 3]
    assert torch.allclose(two, exact, atol=1e-6, rtol=1e-6)
    assert type(sf).window_batch_floor == 256


def test_module_under_torch_ddp_matches_golden_gradients(golden_dir, tmp_path):
    """INTEGRATION.md section 1, "nothing else changes": ScoreUNet wrapped in torch's DistributedDataParallel (what
    fabric.setup_module does, training_loop.py:116), autograd backward, torch.optim.AdamW.  Two gloo ranks, one item each:
    the averaged gradients equal the golden gradients of the mean loss over the batch of 2, and the ranks stay identical."""
    import torch.multiprocessing as mp
    from _ddp_worker import run_module_ddp
    mp.spawn(run_module_ddp, args=(2, _free_port(), golden_dir, str(tmp_path)), nprocs=2, join=True)
    g = _golden(golden_dir, "tiny_net.npz")
    r0, r1 = (torch.load(tmp_path / f"mod{r}.pt", weights_only=False) for r in (0, 1))
    assert 0.5 * (r0["loss"] + r1["loss"]) == pytest.approx(float(g["loss"]), rel=1e-5)
    for n, gr in r0["grads"].items():
        ref = torch.from_numpy(g["grad." + n])
        assert torch.equal(gr, r1["grads"][n]), n  # DDP averaged them
        assert torch.allclose(gr, ref, atol=1e-5 + 2e-4 * ref.abs().max().item()), n
    for k, v in r0["sd"].items():
        assert torch.equal(v, r1["sd"][k]), k
        assert not torch.equal(v, torch.from_numpy(g["sd." + k])) or v.numel() == 0  # the optimizer moved the weights


@pytest.mark.parametrize("bucket_view", [False, True])
def test_five_strings_under_torch_ddp_two_ranks(golden_dir, tmp_path, bucket_view):
    """The reference's own configuration end to end on two gloo ranks: DDP-wrapped module, the loop of training_loop.py:369-391, fused
    SDAPipeline.loss called through the wrapper, climate2weather_amd.optim.AdamW on the DDP-averaged gradients (flat path), EMA.  The
    ranks stay identical and follow a single process that trains on the whole batch with torch.optim.AdamW and the reference's loss
    arithmetic (mean over the batch of 2 = DDP's average of the per-rank means).  bucket_view: DDP(gradient_as_bucket_view=True) -- the
    gradients are then views of the reducer's buckets, not of one flat buffer, and the optimizer must still take its fused step."""
    import torch.multiprocessing as mp
    from _ddp_worker import run_five_strings_ddp
    mp.spawn(run_five_strings_ddp, args=(2, _free_port(), golden_dir, str(tmp_path), bucket_view), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"five{r}.pt", weights_only=False) for r in (0, 1))
    assert r0["flat"] and r1["flat"] and all(r0["fused"]) and all(r1["fused"])
    assert np.allclose(0.5 * (np.array(r0["losses"]) + np.array(r1["losses"])), r0["ref_losses"], rtol=2e-5)
    for k, v in r0["sd"].items():
        assert torch.equal(v, r1["sd"][k]), k  # ranks in lock step
        assert torch.equal(r0["ema"][k], r1["ema"][k]), k
        d = (v - r0["ref_sd"][k]).abs()
        assert d.max().item() <= 3 * 1e-3 * 1.05, (k, d.max().item())  # Adam on a vanishing gradient: at most the three steps (see test_reference_seam)
        if not k.endswith("qkv.bias"):
            assert d.mean().item() <= 2e-6, (k, d.mean().item())
