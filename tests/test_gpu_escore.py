"""The energy-score and variogram-score kernels on the MI355X (csrc/escore.hip through escore_ops and climate2weather_amd.multivariate):
every entry against float64 by the rules of tests/fp64_escore_ref.py -- a D2 entry within 3 * 2^-24 of itself; V[.., 0] within
(2 M + 8) 2^-24 sum (g_y + g_x)^2 over its pairs, V[.., 1] within 3 * 2^-24 and V[.., 2] within (M + 4) 2^-24 of themselves -- then the
properties the interface promises: the same bits wherever a plane lies in the launch, nothing written past the end, nothing written
for an unsupported shape, a non-finite value kept in its own entries, and the public functions on the device against the general
float64 route.

Observed on the MI355X, worst error over its rule (limit 1) over every M and shape below: D2 0.865 (non-finite kind, M = 17; 0.86 on
normalised fields at M = 9), variogram terms 0.29 (pressure biased, M = 9); profiles/escore_measurements.md has the table per M and kind."""
import numpy as np
import pytest
import torch

import fp64_crps_ref as CR
import fp64_escore_ref as R
from climate2weather_amd import escore_ops
from climate2weather_amd import multivariate as MV

pytestmark = pytest.mark.gpu

CANARY = -7.25
TAIL = 64  # canary values behind each output
SIXTEEN_CHUNKS_AND_FOUR = 4096 + 4


def dev():
    return torch.device("cuda:0")


def to_dev(*arrays):
    return [torch.tensor(np.asarray(a)).to(dev()) for a in arrays]


def pairs(x, y, expect=True):
    """D2 (T, F, P) float64 from escore_ops.escore_pairs on x (M, T, F, hw), y (T, F, hw); the TAIL values behind D2 and the scratch
    must keep the canary.  expect False: the call must answer False and leave every value of both buffers alone."""
    M, T, F, hw = x.shape
    xd, yd = to_dev(x, y)
    n = T * F * M * (M + 1) // 2
    nd = escore_ops.escore_scratch_bytes(T * F, hw, M) // 8 if expect else 1024
    d2 = torch.full((n + TAIL,), CANARY, dtype=torch.float64, device=dev())
    scratch = torch.full((nd + TAIL,), CANARY, dtype=torch.float64, device=dev())
    ok = escore_ops.escore_pairs(xd, yd, d2, scratch[:nd] if nd else None, M, T * F, hw)
    assert ok is expect
    assert torch.equal(d2[n if expect else 0:], torch.full_like(d2[n if expect else 0:], CANARY))
    assert torch.equal(scratch[nd if expect else 0:], torch.full_like(scratch[nd if expect else 0:], CANARY))
    return d2[:n].view(T, F, -1)


def vario(x, y, Rr, p, expect=True):
    """V (T, F, O, 3) float64 from escore_ops.vario_terms on x (M, T, F, H, W), y (T, F, H, W), with the same canaries"""
    M, T, F, H, W_ = x.shape
    xd, yd = to_dev(x, y)
    O = ((2 * Rr + 1) ** 2 - 1) // 2
    n = T * F * O * 3
    nd = escore_ops.vario_scratch_bytes(T * F, H, W_, Rr) // 8 if expect else 1024
    V = torch.full((n + TAIL,), CANARY, dtype=torch.float64, device=dev())
    scratch = torch.full((nd + TAIL,), CANARY, dtype=torch.float64, device=dev())
    ok = escore_ops.vario_terms(xd, yd, V, scratch[:nd] if nd else None, M, T * F, H, W_, Rr, MV.KERNEL_ORDERS.get(p, 3))
    assert ok is expect
    assert torch.equal(V[n if expect else 0:], torch.full_like(V[n if expect else 0:], CANARY))
    assert torch.equal(scratch[nd if expect else 0:], torch.full_like(scratch[nd if expect else 0:], CANARY))
    return V[:n].view(T, F, O, 3)


# ------------------------------------------------------------------------------------------------------------------ against float64

PAIR_SHAPES = [(1, 1, 4), (3, 2, 64), (2, 3, 192), (2, 2, SIXTEEN_CHUNKS_AND_FOUR)]
PAIR_MEMBERS = [1, 2, 3, 7, 8, 9, 16, 17, 33, 64]  # both sides of every row-block boundary the tile counts 1, 3, 6, 15, 45, 153 hang on


@pytest.mark.parametrize("M", PAIR_MEMBERS)
def test_pair_distances_against_float64(M):
    """every field kind at every shape; variable f differs from its neighbours in offset and scale, so a wrong index map fails"""
    worst = {}
    for T, F, hw in PAIR_SHAPES:
        for kind in R.KINDS:
            x, y, d2 = R.pairs_reference(kind, M, T, F, hw)
            got = pairs(x, y)
            r, ok = R.worst_d2(got.cpu().numpy(), d2)
            worst[kind] = max(worst.get(kind, 0.0), r)
            assert ok, (kind, (T, F, hw), r)
    print(f"M {M}: D2 error over 3 * 2^-24 D2, limit 1: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


VARIO_FIELDS = [(8, 8), (16, 24), (24, 16), (40, 8)]  # one tile; tiles in a column; (40, 8): 5 tiles, narrower than 2 R + 1 and than a tile
VARIO_RADII = [1, 3, 8]
VARIO_MEMBERS = [1, 2, 8, 9, 16]
ORDERS = [0.5, 1.0, 2.0]


@pytest.mark.parametrize("M", VARIO_MEMBERS)
def test_variogram_terms_against_float64(M):
    """every field, radius and order; the field kinds take turns (every kind meets every order and radius), pressure rides along at p = 0.5"""
    worst, k = {}, 0
    for H, W_ in VARIO_FIELDS:
        for Rr in VARIO_RADII:
            for p in ORDERS:
                kinds = [R.KINDS[k % len(R.KINDS)]] + (["pressure"] if p == 0.5 and R.KINDS[k % len(R.KINDS)] != "pressure" else [])
                k += 1
                for kind in kinds:
                    x, y, V, S = R.vario_reference(kind, M, 1, 2, H, W_, Rr, p)
                    got = vario(x, y, Rr, p)
                    r, ok = R.worst_vario(got.cpu().numpy(), V, S, M)
                    worst[kind] = max(worst.get(kind, 0.0), r)
                    assert ok, (kind, (H, W_), Rr, p, r)
    print(f"M {M}: variogram error over the rules, limit 1: " + ", ".join(f"{k_} {v:.3g}" for k_, v in worst.items()))


# ------------------------------------------------------------------------------------------------------------------ the promises

@pytest.mark.parametrize("M,hw", [(3, 192), (8, SIXTEEN_CHUNKS_AND_FOUR), (17, 516), (64, 260)])
def test_pairs_same_bits_at_every_position(M, hw):
    """one plane first, in the middle and last in the launch, alone, and on a second call"""
    T, F = 3, 2
    x, y = CR.fields("temperature", M, T, F, hw)
    x, y = x.copy(), y.copy()
    x[:, 1, 1] = x[:, 2, 1] = x[:, 0, 0]
    y[1, 1] = y[2, 1] = y[0, 0]
    a, b = pairs(x, y), pairs(x, y)
    assert torch.equal(a, b)
    alone = pairs(x[:, :1, :1], y[:1, :1])
    for t, f in ((0, 0), (1, 1), (2, 1)):
        assert torch.equal(a[t, f], alone[0, 0]), (t, f)
    assert not torch.equal(a[0, 1], alone[0, 0])


@pytest.mark.parametrize("M,H,W_,Rr,p", [(2, 8, 8, 1, 0.5), (8, 16, 24, 3, 1.0), (16, 40, 8, 8, 0.5), (9, 24, 72, 8, 2.0)])
def test_variogram_same_bits_at_every_position(M, H, W_, Rr, p):
    T, F = 3, 2
    x, y = R.fields("temperature", M, T, F, H, W_)
    x, y = x.copy(), y.copy()
    x[:, 1, 1] = x[:, 2, 1] = x[:, 0, 0]
    y[1, 1] = y[2, 1] = y[0, 0]
    a, b = vario(x, y, Rr, p), vario(x, y, Rr, p)
    assert torch.equal(a, b)
    alone = vario(x[:, :1, :1], y[:1, :1], Rr, p)
    for t, f in ((0, 0), (1, 1), (2, 1)):
        assert torch.equal(a[t, f], alone[0, 0]), (t, f)
    assert not torch.equal(a[0, 1], alone[0, 0])


def test_unsupported_shapes_write_nothing_and_take_the_general_route():
    assert not escore_ops.escore_supported(6, 8) and not escore_ops.escore_supported(64, 65) and not escore_ops.escore_supported(64, 0)
    assert escore_ops.escore_supported(4, 1) and escore_ops.escore_supported(16384, 64)
    assert escore_ops.escore_scratch_bytes(6, 256, 8) == 0 and escore_ops.escore_scratch_bytes(6, 260, 8) == 6 * 2 * 36 * 8
    assert not escore_ops.vario_supported(8, 8, 9, 8, 1) and not escore_ops.vario_supported(8, 8, 2, 17, 1) and not escore_ops.vario_supported(12, 8, 2, 8, 1)
    assert not escore_ops.vario_supported(8, 8, 2, 8, 3) and escore_ops.vario_supported(128, 128, 8, 16, 4)
    assert escore_ops.vario_scratch_bytes(6, 8, 32, 2) == 0 and escore_ops.vario_scratch_bytes(6, 16, 40, 2) == 6 * 4 * 12 * 3 * 8
    for M, H, W_ in ((8, 2, 3), (65, 2, 4)):  # hw = 6; M = 65
        x, y = CR.fields("temperature", M, 2, 2, H * W_)
        pairs(x, y, expect=False)
        got = MV.pair_sqdist(*to_dev(x.reshape(M, 2, 2, H, W_), y.reshape(2, 2, H, W_)))
        assert got.is_cuda and np.allclose(got.cpu().numpy(), R.d2_64(x, y), rtol=1e-13, atol=0)  # the general route: float64
    for M, Rr, p in ((8, 9, 0.5), (17, 2, 0.5), (8, 2, 0.75)):  # R = 9; M = 17; an order the kernel does not have
        x, y = R.fields("temperature", M, 1, 2, 8, 16)
        vario(x, y, Rr, p, expect=False)
        got = MV.variogram_terms(*to_dev(x, y), radius=Rr, p=p)
        V, _ = R.vario64(x, y, Rr, p)
        assert got.is_cuda and np.allclose(got.cpu().numpy(), V, rtol=1e-12, atol=0)


def test_a_non_finite_value_poisons_its_own_entries_only():
    M, T, F, H, W_, Rr = 9, 3, 2, 16, 40, 3
    x, y = R.fields("wind", M, T, F, H, W_)
    flat = lambda a: a.reshape(a.shape[:-2] + (H * W_,))
    clean_d2, clean_v = pairs(flat(x), flat(y)), vario(x, y, Rr, 0.5)
    x, y = x.copy(), y.copy()
    x[4, 1, 0, 15, 39] = np.nan      # the last cell: the third chunk of the pairs kernel, the last tile of the variogram kernel
    x[0, 2, 1, 0, 0] = -np.inf
    y[0, 1, 8, 32] = np.inf          # first cell of a tile: its pairs reach into three other tiles
    d2, V = pairs(flat(x), flat(y)), vario(x, y, Rr, 0.5)
    bad = torch.zeros(T, F, M * (M + 1) // 2, dtype=torch.bool, device=dev())
    for (t, f), row in (((1, 0), 5), ((2, 1), 1), ((0, 1), 0)):
        for other in range(M + 1):
            if other != row:
                bad[t, f, MV.pair_index(M, min(row, other), max(row, other))] = True
    assert torch.equal(torch.isnan(d2), bad) and torch.equal(d2[~bad], clean_d2[~bad])
    vbad = torch.zeros(T, F, len(MV.offsets(Rr)), dtype=torch.bool, device=dev())
    for (t, f), (i, j) in (((1, 0), (15, 39)), ((2, 1), (0, 0)), ((0, 1), (8, 32))):
        for o, (di, dj) in enumerate(MV.offsets(Rr)):
            vbad[t, f, o] = (i + di < H and 0 <= j + dj < W_) or (i - di >= 0 and 0 <= j - dj < W_)
    assert torch.equal(torch.isnan(V).all(-1), vbad) and torch.equal(torch.isnan(V).any(-1), vbad) and torch.equal(V[~vbad], clean_v[~vbad])
    assert bool(vbad[0, 1].all()) and not bool(vbad[1, 0].all())
    S, Tr = to_dev(x, y)
    assert torch.equal(torch.isnan(MV.energy_score(S, Tr)), bad.any(-1)) and torch.equal(torch.isnan(MV.variogram_score(S, Tr, radius=Rr)), vbad.any(-1))


def test_strided_half_precision_input_agrees_with_the_dense_route():
    base = (torch.randn(5, 3, 2, 16, 64, device=dev()) * 3.0 + 1.0).to(torch.float16)
    view, truth = base[..., ::2], base[0, ..., 1::2]
    dense, dtruth = view.float().contiguous(), truth.float().contiguous()
    assert torch.equal(MV.pair_sqdist(view, truth), MV.pair_sqdist(dense, dtruth))
    assert torch.equal(MV.variogram_terms(view, truth, radius=2), MV.variogram_terms(dense, dtruth, radius=2))


# ------------------------------------------------------------------------------------------------------------------ the public functions

def test_public_functions_on_the_device_equal_the_cpu_general_route():
    """(M, T, F) = (8, 3, 2) at 16 x 24, de-normalised (temperature-like and pressure-like): the device products against the CPU general
    route -- float64 -- by the rules; the scores and the report are the same algebra on those products"""
    M, T, F, H, W_, Rr = 8, 3, 2, 16, 24, 3
    rng = np.random.default_rng(9)
    off, sd = np.array([280.0, 101325.0]), np.array([10.0, 1200.0])
    ii, jj = np.meshgrid(np.arange(H), np.arange(W_), indexing="ij")
    wave = np.sin(0.3 * ii + 0.2 * jj)[None, None]
    centre = off[None, :, None, None] + sd[None, :, None, None] * (wave + 0.2 * rng.standard_normal((T, F, H, W_)))
    truth = (centre + 0.01 * sd[None, :, None, None] * rng.standard_normal((T, F, H, W_))).astype(np.float32)
    samples = (centre[None] + 0.012 * sd[None, None, :, None, None] * rng.standard_normal((M, T, F, H, W_))).astype(np.float32)
    Sc, Tc = torch.tensor(samples), torch.tensor(truth)
    S, Tr = to_dev(samples, truth)
    cpu_d2, gpu_d2 = MV.pair_sqdist(Sc, Tc), MV.pair_sqdist(S, Tr)
    d2 = R.d2_64(samples.reshape(M, T, F, -1), truth.reshape(T, F, -1))
    assert np.allclose(cpu_d2.numpy(), d2, rtol=1e-12, atol=0)  # the CPU route is the definition
    r, ok = R.worst_d2(gpu_d2.cpu().numpy(), cpu_d2.numpy())
    print(f"device D2 against the CPU general route: error over the bound {r:.3g} (limit 1)")
    assert ok
    for p in ORDERS:
        cpu_v, gpu_v = MV.variogram_terms(Sc, Tc, radius=Rr, p=p), MV.variogram_terms(S, Tr, radius=Rr, p=p)
        V, Sy = R.vario64(samples, truth, Rr, p)
        assert np.allclose(cpu_v.numpy(), V, rtol=1e-11, atol=0)
        r, ok = R.worst_vario(gpu_v.cpu().numpy(), cpu_v.numpy(), Sy, M)
        print(f"device variogram terms p = {p} against the CPU general route: error over the rules {r:.3g} (limit 1)")
        assert ok
        w = np.array([1.0 / np.hypot(di, dj) for di, dj in MV.offsets(Rr)])
        vs = MV.variogram_score(S, Tr, radius=Rr, p=p)
        assert vs.is_cuda and np.all(np.abs(vs.cpu().numpy() - MV.variogram_score(Sc, Tc, radius=Rr, p=p).numpy()) <= 1.01 * R.v0_factor(M) * (Sy * w).sum(-1))
    # ES is a sum of square roots of D2 entries: a square root halves a relative error
    for kw in (dict(), dict(fair=True), dict(beta=0.5), dict(joint=True)):
        got, want = MV.energy_score(S, Tr, **kw), MV.energy_score(Sc, Tc, **kw)
        dist = np.sqrt(d2 if not kw.get("joint") else (d2 / truth.astype(np.float64).std(axis=(0, 2, 3))[None, :, None] ** 2).sum(1)) ** kw.get("beta", 1.0)
        allow = 1.01 * 0.5 * R.D2_C * R.EPS * (dist[..., :M].sum(-1) / M + dist[..., M:].sum(-1) / (M * (M - 1)))
        assert got.is_cuda and got.dtype == torch.float64 and np.all(np.abs(got.cpu().numpy() - want.numpy()) <= allow), kw
    cpu, gpu = MV.multivariate_report(Sc, Tc, names=["tas", "psl"], radius=Rr), MV.multivariate_report(S, Tr, names=["tas", "psl"], radius=Rr)
    for name, v in gpu:
        assert all(t.is_cuda and t.dtype == torch.float64 for t in v.values())
        for key in ("energy", "energy_fair", "variogram"):
            assert float(v[key]) == pytest.approx(float(cpu[name][key]), rel=1e-5)
        assert torch.allclose(v["variogram_truth"].cpu(), cpu[name]["variogram_truth"], rtol=1e-6)
    assert set(gpu.as_dict()) == set(cpu.as_dict()) and float(gpu.joint["energy"]) == pytest.approx(float(cpu.joint["energy"]), rel=1e-6)
