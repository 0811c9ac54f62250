"""The seam the other way round: what the REFERENCE's own sampler / loss / EMA / training-loop code (src/thor/score.py,
src/thor/pipelines.py, src/thor/ema.py, src/thor/lr.py) computes when it drives THIS package's ScoreUNet, i.e. a user who changes nothing
but `network_kwargs.class_name`.  Those results are stored in tests/golden/seam.npz (tests/golden/make_seam.py runs the reference to
make them) where sampler.npz does not already hold them; the tests drive the same network through this package's drop-in classes and
must land on them.  The training loop's reference side is rerun here with the in-repository oracle (oracle/) and tied to the reference by
the fingerprints seam.npz keeps of its result.  HIP launchers are replaced by tests/emu_ops.py (CPU)."""
import os

import numpy as np
import torch

import emu_ops
from climate2weather_amd import ops as c2w_ops
from climate2weather_amd.score import ScoreUNet

TINY = dict(embedding_dim=64, hidden_channels=[32, 64], hidden_blocks=[1, 1], attention_levels=[1], kernel_size=3, padding_mode="zeros")


def _npz(golden_dir, name):
    return {k: v for k, v in np.load(os.path.join(golden_dir, name), allow_pickle=False).items()}


def _rel(a, ref):
    return (a - ref).abs().max().item() / ref.abs().max().item()


def test_reference_sampler_drives_this_network(monkeypatch, golden_dir):
    emu_ops.install(monkeypatch, c2w_ops)
    from climate2weather_amd.pipelines import SDAPipeline
    from climate2weather_amd.score_fn import BatchedScoreFunction
    s = _npz(golden_dir, "sampler.npz")
    seam = {k: torch.from_numpy(v) for k, v in _npz(golden_dir, "seam.npz").items() if k.startswith("drive.")}  # the reference's guided score
    torch.manual_seed(3)
    net = ScoreUNet(channels=6, spatial=2, activation=torch.nn.SiLU, **TINY).eval()
    pipe = SDAPipeline()
    sf = BatchedScoreFunction(net, markov_order=1, batch_size=4, device=torch.device("cpu"), noise_process=pipe)
    with torch.no_grad():
        y = sf(torch.from_numpy(s["score_x"]), torch.tensor(0.7))
    assert torch.allclose(y, torch.from_numpy(s["score_y"]), atol=2e-5)  # what the reference's score function gives over this network
    # unconditioned trajectory (no corrector draws needed)
    x = pipe.sample(sf, torch.from_numpy(s["uncond_c0.noise"]), steps=4, corrections=0, tau=0.5, show_progressbar=False)
    ref = torch.from_numpy(s["uncond_c0.x"])
    assert _rel(x, ref) <= 3e-4
    # guided trajectory: the reference's torch.func.jacrev wraps this network's forward (exact_grad False and True)
    A = lambda z: torch.nn.functional.avg_pool2d(z[::2], 8)  # noqa: E731
    for name, exact in (("cond_c0", False),):
        sfc = BatchedScoreFunction(net, markov_order=1, batch_size=4, device=torch.device("cpu"), noise_process=pipe)
        sfc.condition_on(A=A, y=torch.from_numpy(s["y_obs"]), std=torch.from_numpy(s["std"]), gamma=float(s["gamma"]), exact_grad=exact)
        xc = pipe.sample(sfc, torch.from_numpy(s[name + ".noise"]), steps=4, corrections=0, tau=0.5, show_progressbar=False)
        refc = torch.from_numpy(s[name + ".x"])
        assert _rel(xc, refc) <= 3e-4, name
    # exact_grad=True differentiates through the network inside jacrev: one guided score evaluation against the reference's
    mine = BatchedScoreFunction(net, markov_order=1, batch_size=4, device=torch.device("cpu"), noise_process=SDAPipeline())
    mine.device_resident = False
    mine.condition_on(A=A, y=torch.from_numpy(s["y_obs"]), std=torch.from_numpy(s["std"]), gamma=float(s["gamma"]), exact_grad=True)
    e_mine = mine(torch.from_numpy(s["score_x"]), torch.tensor(0.7))
    assert torch.allclose(seam["drive.exact_score"], e_mine, rtol=1e-4, atol=1e-5)


def test_reference_loss_ema_and_default_score_function_with_this_network(monkeypatch, golden_dir):
    """src/thor/pipelines.py::SDAPipeline.loss, src/thor/ema.py::StandardEMA (deep copies + zip over parameters()) and
    src/thor/score.py::DefaultScoreFunction: this package's drop-ins over this package's ScoreUNet, against what the reference's
    classes computed over it."""
    emu_ops.install(monkeypatch, c2w_ops)
    from climate2weather_amd.ema import StandardEMA
    from climate2weather_amd.pipelines import SDAPipeline
    from climate2weather_amd.score_fn import DefaultScoreFunction
    g = _npz(golden_dir, "tiny_net.npz")
    seam = _npz(golden_dir, "seam.npz")
    torch.manual_seed(3)
    net = ScoreUNet(channels=6, spatial=2, activation=torch.nn.SiLU, **TINY)
    ema = StandardEMA(net, rates=[0.9, 0.999])
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-3)
    pipe = SDAPipeline()
    x = torch.from_numpy(g["x"])
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    torch.manual_seed(0)
    losses = []
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        loss = pipe.loss(net, x).mean()  # draws t ~ U(0,1) and eps itself (src/thor/pipelines.py:27-35)
        loss.backward()
        opt.step()
        ema.update()
        losses.append(loss.item())
    assert all(np.isfinite(losses))
    assert np.allclose(losses, seam["loss_ema.losses"], rtol=2e-5), (losses, seam["loss_ema.losses"])
    for (rate, m) in zip(ema.rates, ema.emas):
        for n, p in m.named_parameters():
            assert not torch.equal(p, before[n]) or p.numel() == 0, n
    for m, tag in ema.get():
        assert isinstance(m, ScoreUNet) and tag.startswith("-0.")
    # the deep copies are independent networks with their own engines: same input, different (averaged) weights
    xt, t = torch.from_numpy(g["xt"]), torch.from_numpy(g["t"])
    with torch.no_grad():
        assert not torch.allclose(net(xt, t), ema.emas[0](xt, t), atol=1e-7)
    s = _npz(golden_dir, "sampler.npz")
    torch.manual_seed(3)
    fresh = ScoreUNet(channels=6, spatial=2, activation=torch.nn.SiLU, **TINY).eval()
    dsf = DefaultScoreFunction(fresh, markov_order=1, noise_process=pipe)
    with torch.no_grad():
        y = dsf(torch.from_numpy(s["score_x"]), torch.tensor(0.7))
    assert torch.allclose(y, torch.from_numpy(s["score_y"]), atol=2e-5)


def test_member_random_stream_is_the_reference_drivers(monkeypatch, golden_dir):
    """exp/downscaling.py:100-103,248-265 restated by oracle/host.py::ensemble_members: the driver itself is not importable here
    (fire / xarray / lightning), but the two things it does with random numbers are -- seed the process, `torch.randn(L,C,H,W)` per
    member, then the REFERENCE's `pipeline.sample`, whose corrector fills `z.normal_()` from the same CPU stream.  Those statements run
    with the reference's sampler classes gave the members in seam.npz; `run_ensemble(rng="reference")` must give the same members."""
    emu_ops.install(monkeypatch, c2w_ops)
    from climate2weather_amd.sampling import run_ensemble
    seam = _npz(golden_dir, "seam.npz")
    torch.manual_seed(3)
    net = ScoreUNet(channels=6, spatial=2, activation=torch.nn.SiLU, **TINY).eval()
    L, C, H, W, rank, world, n, seed = 5, 2, 16, 16, 1, 2, 4, 7
    mine = run_ensemble(net, world=world, rank=rank, device=torch.device("cpu"), precision="fp32", length=L, n_vars=C, height=H, width=W,
                        markov_order=1, num_samples=n, steps=3, corrections=1, tau=0.5, batch_size=2, seed=seed)
    per = n // world
    assert len(mine) == per
    for i in range(per):  # exp/downscaling.py:248-258
        x = torch.from_numpy(seam[f"member.{i}"])
        assert x.shape == (L, C, H, W)
        sid, xm = mine[i]
        assert sid == rank * per + i
        assert (xm - x).abs().max().item() <= 3e-4 * x.abs().max().item()


FINGERPRINT_ENTRIES = 64  # tests/golden/make_seam.py::fingerprint


def _fingerprint(t):
    """float64 sum, sum of magnitudes and FINGERPRINT_ENTRIES evenly spaced entries of a tensor (make_seam.py stores the same of the
    reference's)."""
    f = t.detach().reshape(-1).double()
    k = min(f.numel(), FINGERPRINT_ENTRIES)
    return torch.cat([torch.stack([f.sum(), f.abs().sum()]), f[torch.arange(k) * f.numel() // k]])


def _oracle_loop():
    """The reference side of the training-loop test with the in-repository oracle: its plain-PyTorch restatement of model.score.ScoreUNet
    under torch autograd, torch.optim.AdamW, the draws of src/thor/pipelines.py::SDAPipeline.loss in their order (t, then eps) with
    oracle.diffusion.loss, src/thor/lr.py (oracle.host.linear_lr) and src/thor/ema.py's blend at its default rate.  The initial weights
    are those this package's ScoreUNet draws from the same seed (the reference's: the fingerprints check the result)."""
    from oracle import diffusion as od
    from oracle import host as oh
    from oracle.unet import OracleScoreUNet
    torch.manual_seed(42)
    init = ScoreUNet(channels=6, spatial=2, activation=torch.nn.SiLU, **TINY).state_dict()
    net = OracleScoreUNet(init, TINY["hidden_blocks"], TINY["attention_levels"])
    ema = OracleScoreUNet(init, TINY["hidden_blocks"], TINY["attention_levels"])
    optimizer = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-3, betas=[0.9, 0.999])
    g = torch.Generator().manual_seed(7)
    cur_ndata, batch_size, losses = 0, 2, []
    for _ in range(3):
        optimizer.zero_grad()
        data = torch.randn(batch_size, 6, 16, 16, generator=g) * 0.5 + 0.5
        t = torch.rand(batch_size, 1, 1, 1)
        eps = torch.randn_like(data)
        loss = od.loss(net, data, t, eps).mean().mul(1.0)
        loss.backward()
        for grp in optimizer.param_groups:
            grp["lr"] = oh.linear_lr(cur_ndata, 40, 1e-3)
        optimizer.step()
        losses.append(loss.detach().item())
        cur_ndata += batch_size
        with torch.no_grad():
            for p_ema, p_net in zip(ema.parameters(), net.parameters()):
                p_ema.copy_(oh.ema_update(p_ema, p_net, 0.9999))
    return losses, {k: v.detach() for k, v in net.sd().items()}, {k: v.detach() for k, v in ema.sd().items()}


def test_the_training_loop_with_five_strings_changed_follows_the_reference(golden_dir, monkeypatch):
    """training_loop.py:85-131,369-391 with the five class_name / func_name strings of train.py:164-193 pointing at this package --
    everything resolved by name through construct_class_by_name the way the loop does it -- against the same loop from the same seed
    with the reference's own classes (model.score.ScoreUNet over the zuko shim, torch.optim.AdamW, thor.pipelines.SDAPipeline,
    thor.ema.StandardEMA, thor.lr).  Same draws (CPU tensors take the reference's loss arithmetic), so after three optimizer steps the
    losses, the 228-key state_dict, the EMA copy and the optimizer's state_dict must agree.  seam.npz holds the reference run's losses,
    optimizer state and a fingerprint of every tensor; the oracle reruns that loop here (_oracle_loop), must match the fingerprints, and
    is the tensor-by-tensor reference this package's loop is compared with."""
    emu_ops.install(monkeypatch, c2w_ops)
    from climate2weather_amd import util as c2w_util
    seam = _npz(golden_dir, "seam.npz")

    def run(strings):
        net_kw = c2w_util.EasyDict(class_name=strings["net"], channels=6, spatial=2, activation=torch.nn.SiLU, **TINY)
        opt_kw = c2w_util.EasyDict(class_name=strings["opt"], lr=1e-3, weight_decay=1e-3, betas=[0.9, 0.999])  # train.py:175-180
        pipe_kw = c2w_util.EasyDict(class_name=strings["pipe"])
        ema_kw = c2w_util.EasyDict(class_name=strings["ema"])
        lr_kw = c2w_util.EasyDict(func_name=strings["lr"], ref_lr=1e-3, total_ndata=40)
        torch.manual_seed(42)
        net = c2w_util.construct_class_by_name(**net_kw)  # training_loop.py:88-89
        net.train()
        pipeline = c2w_util.construct_class_by_name(**pipe_kw)
        optimizer = c2w_util.construct_class_by_name(params=net.parameters(), **opt_kw)  # training_loop.py:119-121
        ema = c2w_util.construct_class_by_name(net=net, **ema_kw)
        state = c2w_util.EasyDict(cur_ndata=0)
        batch_size, losses = 2, []
        g = torch.Generator().manual_seed(7)
        for _ in range(3):  # training_loop.py:369-391
            optimizer.zero_grad()
            data = torch.randn(batch_size, 6, 16, 16, generator=g) * 0.5 + 0.5
            loss = pipeline.loss(net=net, x=data).mean().mul(1.0)
            loss.backward()
            lr = c2w_util.call_func_by_name(cur_ndata=state.cur_ndata, **lr_kw)
            for grp in optimizer.param_groups:
                grp["lr"] = lr
            optimizer.step()
            losses.append(loss.detach().item())
            state.cur_ndata += batch_size
            ema.update(cur_ndata=state.cur_ndata, batch_size=batch_size)
        return losses, net.state_dict(), ema.emas[0].state_dict(), optimizer.state_dict()

    ref_fp = {k[len("loop.net."):]: torch.from_numpy(v) for k, v in seam.items() if k.startswith("loop.net.")}
    ref_ema_fp = {k[len("loop.ema."):]: torch.from_numpy(v) for k, v in seam.items() if k.startswith("loop.ema.")}
    orc = _oracle_loop()
    mine = run(dict(net="climate2weather_amd.score.ScoreUNet", opt="climate2weather_amd.optim.AdamW", pipe="climate2weather_amd.pipelines.SDAPipeline",
                    ema="climate2weather_amd.ema.StandardEMA", lr="climate2weather_amd.lr.linear_learning_rate_schedule"))
    assert np.allclose(seam["loop.losses"], orc[0], rtol=2e-5), (seam["loop.losses"], orc[0])
    assert np.allclose(seam["loop.losses"], mine[0], rtol=2e-5), (seam["loop.losses"], mine[0])
    keys = list(ref_fp)  # zuko's LayerNorm registers eps as a buffer: make_seam.py left those out
    assert keys == list(mine[1].keys()) and len(keys) == len(list(mine[1])) and keys == list(ref_ema_fp) == list(orc[1]) == list(orc[2])
    # Two independent differentiations (torch autograd over the reference's modules / this package's hand-written backward) agree to
    # fp32 round-off; Adam turns the round-off of a vanishing gradient (the attention key bias has none at all; single entries
    # elsewhere) into a full step of lr = 1e-3 per iteration.  So: essentially every entry equal, none further apart than the three steps.
    # The oracle against the reference, through the fingerprints: the same bounds on the sampled entries, the mean bound on the sums.
    for k in keys:
        for fr, o in ((ref_fp[k], orc[1][k]), (ref_ema_fp[k], orc[2][k])):
            fo = _fingerprint(o)
            assert fo.shape == fr.shape, k
            d, dsum = (fo[2:] - fr[2:]).abs(), (fo[:2] - fr[:2]).abs()
            assert d.max().item() <= 3 * 1e-3 * 1.05 and dsum.max().item() <= 3 * 1e-3 * 1.05 * o.numel(), (k, d.max().item())
            if not k.endswith("qkv.bias"):
                assert d.max().item() <= 1e-5 and dsum.max().item() <= 2e-6 * o.numel(), (k, d.max().item(), dsum.tolist())
    # this package's loop against the oracle's, tensor by tensor
    for k in keys:
        for a, b in ((orc[1][k], mine[1][k]), (orc[2][k], mine[2][k])):
            d = (a - b).abs()
            assert d.max().item() <= 3 * 1e-3 * 1.05, (k, d.max().item())
            if not k.endswith("qkv.bias"):
                assert d.mean().item() <= 2e-6 and (d > 1e-5).float().mean().item() <= 0.02, (k, d.mean().item())
    so_m = mine[3]
    assert sorted(so_m["state"]) == seam["loop.opt_state_ids"].tolist() and all(float(so_m["state"][i]["step"]) == 3.0 for i in so_m["state"])
    assert np.all(seam["loop.opt_steps"] == 3.0)
    assert float(seam["loop.lr"]) == so_m["param_groups"][0]["lr"]
