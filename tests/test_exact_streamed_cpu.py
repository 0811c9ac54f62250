"""CPU checks of the window-streamed exact guidance (score_fn.py::_guided_exact_streamed): the window list, the route against the
autograd route and the imported reference's trajectories, its bounded work and memory, and when it engages -- with the HIP launchers
replaced by tests/emu_ops.py + tests/emu_exact_ops.py."""
import numpy as np
import pytest
import torch

import emu_exact_ops
from climate2weather_amd import ops as c2w_ops
from climate2weather_amd.engine import Engine
from climate2weather_amd.pipelines import SDAPipeline
from climate2weather_amd.score_fn import BatchedScoreFunction, PoolStrideOperator, exact_window_list
from test_host_emulated import _golden, _sample, _tiny


@pytest.fixture()
def emu(monkeypatch):
    emu_exact_ops.install(monkeypatch, c2w_ops)


def _brute_force(L, k, t_step, nobs):
    """Selected windows by enumerating what fold keeps of every window and which frames the likelihood observes."""
    w = 2 * k + 1
    nwin = L - w + 1
    observed = {l for l in range(L) if l % t_step == 0 and l // t_step < nobs}
    first, kind = [], []
    for i in range(nwin):
        kept = {i + k}
        if i == 0:
            kept |= set(range(k))
        if i == nwin - 1:
            kept |= set(range(nwin + k, L))
        if kept & observed:
            first.append(i)
            kind.append((1 if i == 0 else 0) | (2 if i == nwin - 1 else 0))
    return first, kind


# (L, k, t_step, nobs, expected list or None = every window)
CASES = [(9, 1, 2, 5, [0, 1, 3, 5, 6]), (14, 1, 6, 3, [0, 5, 11]), (14, 1, 1, 14, None), (14, 1, 3, 2, [0, 2]), (3, 1, 2, 2, [0]),
         (4, 1, 5, 1, [0]), (25, 6, 6, 5, [0, 6, 12])]


@pytest.mark.parametrize("L,k,t_step,nobs,expected", CASES)
def test_exact_window_list_against_brute_force(L, k, t_step, nobs, expected):
    first, kind = exact_window_list(1, L, k, t_step, nobs)
    nwin = L - 2 * k
    assert (first, kind) == _brute_force(L, k, t_step, nobs)
    assert first == (list(range(nwin)) if expected is None else expected)
    assert kind[0] & 1 and all(not kd & 1 for kd in kind[1:])  # window 0 keeps frame 0, which is always observed
    for i, kd in zip(first, kind):
        assert bool(kd & 2) == (i == nwin - 1)
    # two members: the per-member list offset by m * L
    first2, kind2 = exact_window_list(2, L, k, t_step, nobs)
    assert first2 == first + [L + i for i in first] and kind2 == kind + kind


def _scale_rel(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


def _setup(golden_dir, frozen=True, batch_size=4, gamma=None, exact=True, A=None):
    s = _golden(golden_dir, "sampler.npz")
    net = _tiny().eval()
    if frozen:
        net.requires_grad_(False)
    sf = BatchedScoreFunction(net, markov_order=1, batch_size=batch_size, device=torch.device("cpu"), noise_process=SDAPipeline())
    sf.condition_on(A=A or PoolStrideOperator(8, 2), y=torch.from_numpy(s["y_obs"]), std=torch.from_numpy(s["std"]),
                    gamma=float(s["gamma"]) if gamma is None else gamma, exact_grad=exact)
    return s, sf


def test_one_guided_evaluation_matches_the_autograd_route(emu, golden_dir):
    s, sf = _setup(golden_dir)
    x, t = torch.from_numpy(s["score_x"]), torch.tensor(0.7)
    sf.exact_streamed = False
    ref = sf(x, t)
    sf.exact_streamed = True
    got = sf(x, t)
    assert sf._fused_guidance is None
    print("streamed vs autograd route, scale-relative:", _scale_rel(got, ref))
    assert _scale_rel(got, ref) <= 1e-5
    # the network term is there: exact_grad=False leaves it out
    _, sf0 = _setup(golden_dir, exact=False)
    assert _scale_rel(sf0(x, t), ref) > 1e-2 and _scale_rel(sf0(x, t), got) > 1e-2


def test_trajectories_match_the_reference(emu, golden_dir):
    s, sg = _golden(golden_dir, "sampler.npz"), _golden(golden_dir, "sampler_gamma.npz")
    for name, src, gamma, noise in [("cond_c1_exact", s, None, s["cond_c1_exact.noise"]),
                                    ("cond_c1_gvec_exact", sg, torch.from_numpy(sg["gamma"]), s["cond_c0.noise"])]:
        _, sf = _setup(golden_dir, gamma=gamma)
        sf.exact_streamed = True
        zs = [torch.from_numpy(z) for z in src[name + ".z"]]
        for fused in (True, False):
            sf.device_resident = fused
            xs = _sample(sf.noise_process, sf, torch.from_numpy(noise), 1, zs, torch.device("cpu"), fused)
            ref = torch.from_numpy(src[name + ".x"])
            assert (xs - ref).abs().max().item() <= 3e-4 * ref.abs().max().item(), (name, fused)


def test_work_and_tape_memory_are_bounded_by_the_batch(emu, golden_dir, monkeypatch):
    """L = 14, t_step = 6: 3 of 12 windows are differentiated, 2 at a time; a tape is consumed before the next one is recorded."""
    net = _tiny().eval().requires_grad_(False)
    sf = BatchedScoreFunction(net, markov_order=1, batch_size=2, device=torch.device("cpu"), noise_process=SDAPipeline())
    gen = torch.Generator().manual_seed(5)
    A = PoolStrideOperator(8, 6)
    truth = torch.randn(14, 2, 32, 32, generator=gen)
    sf.condition_on(A=A, y=A(truth), std=0.1, gamma=1e-2, exact_grad=True)
    sf.exact_streamed = True
    log = []
    fwd, bwd = Engine.forward, Engine.backward

    def spy_forward(self, x, t, dt, tape=None, **kw):
        if tape is not None:
            log.append(("forward", id(tape), kw["shape"][0]))
        return fwd(self, x, t, dt, tape=tape, **kw)

    def spy_backward(self, tape, gy, want_dx=False, want_dw=True):
        log.append(("backward", id(tape), want_dw))
        return bwd(self, tape, gy, want_dx=want_dx, want_dw=want_dw)

    monkeypatch.setattr(Engine, "forward", spy_forward)
    monkeypatch.setattr(Engine, "backward", spy_backward)
    x = torch.randn(14, 2, 32, 32, generator=gen)
    out = sf(x, torch.tensor(0.6))
    assert torch.isfinite(out).all()
    taped = [e for e in log if e[0] == "forward"]
    assert sum(e[2] for e in taped) == 3 and [e[2] for e in taped] == [2, 1]  # not 12
    assert [e[0] for e in log] == ["forward", "backward"] * len(taped)
    for f, b in zip(log[0::2], log[1::2]):
        assert f[1] == b[1]  # the tape just recorded is the one handed to backward, before the next taped forward starts
    assert not any(e[2] for e in log if e[0] == "backward")  # never want_dw=True
    # and the numbers are those of the autograd route
    monkeypatch.setattr(Engine, "forward", fwd)
    monkeypatch.setattr(Engine, "backward", bwd)
    sf.exact_streamed = False
    assert _scale_rel(out, sf(x, torch.tensor(0.6))) <= 1e-5


def test_when_the_route_engages(emu, golden_dir, monkeypatch):
    s, sf = _setup(golden_dir)
    x, t = torch.from_numpy(s["score_x"]), torch.tensor(0.7)
    calls = []
    orig = BatchedScoreFunction._guided_exact_streamed
    monkeypatch.setattr(BatchedScoreFunction, "_guided_exact_streamed", lambda self, x, t: calls.append(1) or orig(self, x, t))
    assert sf.exact_streamed is None and sf.exact_tape_windows == 1024
    ref = sf(x, t)  # 7 windows: today's route
    assert not calls and sf._fused_guidance is None
    sf.exact_tape_windows = 4
    got = sf(x, t)
    assert len(calls) == 1 and _scale_rel(got, ref) <= 1e-5
    sf.exact_streamed = False
    sf(x, t)
    assert len(calls) == 1
    # exact_streamed=True never falls back silently
    _, sf_l = _setup(golden_dir, A=lambda z: torch.nn.functional.avg_pool2d(z[::2], 8))
    sf_l.exact_streamed = True
    with pytest.raises(ValueError, match="PoolStrideOperator"):
        sf_l(x, t)
    _, sf_g = _setup(golden_dir, frozen=False)
    sf_g.exact_streamed = True
    with pytest.raises(ValueError, match="requires a gradient"):
        sf_g(x, t)
    sf_g.exact_streamed = None  # not eligible and not forced: today's route, whatever the threshold
    sf_g.exact_tape_windows = 4
    sf_g(x, t)
    assert len(calls) == 1 and sf_g._fused_guidance is None and sf_l._fused_guidance is None


def test_co_sampled_members_equal_the_members_alone(emu, golden_dir):
    s, sf = _setup(golden_dir)
    sf.exact_streamed = True
    x = torch.from_numpy(s["score_x"])
    x2 = torch.stack([x, torch.from_numpy(np.ascontiguousarray(s["score_x"][::-1])) * 0.9], 0)
    t = torch.tensor(0.7)
    both = sf(x2, t)
    for m in range(2):
        alone = sf(x2[m], t)
        assert _scale_rel(both[m], alone) <= 1e-6
