"""The quantile kernels on the MI355X (csrc/quantile.hip through ops.quantiles and climate2weather_amd.quantiles): the order statistics
bit for bit (-0.0 == +0.0 allowed), the results numerically equal with NaN equal to NaN and the counts exactly equal to the CPU
reference of tests/fp64_quantile_ref.py -- a numpy sort and numpy's own interpolation, no tolerance anywhere -- then the properties the
interface promises: the same bits wherever a data set lies in the launch, nothing written past the end, nothing written for an
unsupported shape, a NaN kept in its own row, a scratch that can be used again."""
import numpy as np
import pytest
import torch

import fp64_quantile_ref as R
from climate2weather_amd import normalize as Nm
from climate2weather_amd import ops
from climate2weather_amd import quantiles as Qt

pytestmark = pytest.mark.gpu

CANARY = -7.25
TAIL = 64  # canary values behind each output
SCRATCH_FILL = 0xA5


def dev():
    return torch.device("cuda:0")


def to_dev(*arrays):
    return [torch.tensor(np.asarray(a)).to(dev()) for a in arrays]


def new_scratch(D, Q, supported=True):
    nbytes = ops.quantile_scratch_bytes(D, Q) if supported else 1 << 16
    return torch.full((nbytes + TAIL,), SCRATCH_FILL, dtype=torch.uint8, device=dev()), nbytes


def select(x, y, q, skipna=True, expect=True, scratch=None):
    """(out (D, Q) float64, stats (D, Q, 2) fp32, n_valid (D,) int64) as numpy from ops.quantiles on x (n_rep, T, F, hw), y (T, F, hw) or
    None; the TAIL values behind each of them and behind the scratch must keep the canary.  expect False: the call must answer False
    and leave every value of all four buffers alone."""
    n_rep, T, F, hw = x.shape
    Q = len(q)
    D = n_rep * F + (F if y is not None else 0)
    xd = to_dev(x)[0]
    yd = None if y is None else to_dev(y)[0]
    scratch, nbytes = new_scratch(D, Q, expect) if scratch is None else scratch
    out = torch.full((D * Q + TAIL,), CANARY, dtype=torch.float64, device=dev())
    stats = torch.full((D * Q * 2 + TAIL,), CANARY, dtype=torch.float32, device=dev())
    nv = torch.full((D + TAIL,), -7, dtype=torch.int64, device=dev())
    ok = ops.quantiles(xd, yd, [float(v) for v in q], skipna, scratch[:nbytes], out, stats, nv, n_rep, T, F, hw)
    assert ok is expect
    for buf, used in ((out, D * Q), (stats, D * Q * 2), (nv, D), (scratch, nbytes)):
        keep = buf[used if expect else 0:]
        fill = SCRATCH_FILL if buf is scratch else (-7 if buf is nv else CANARY)
        assert torch.equal(keep, torch.full_like(keep, fill))
    return out[:D * Q].view(D, Q).cpu().numpy(), stats[:D * Q * 2].view(D, Q, 2).cpu().numpy(), nv[:D].cpu().numpy()


# (n_rep, T, F, hw, with truth): n = 4; the smallest plane of two loads; samples and truth in one launch; four variables, three
# replicas; many planes of one variable; a large plane; more planes than workgroups per data set on a 256-CU chip (409 slabs of up to
# 11 planes: 372 full ones, a ragged one of 8, and slabs that own nothing); D = 36
SHAPES = [(1, 1, 1, 4, False), (1, 1, 1, 8, False), (2, 3, 2, 64, True), (3, 5, 4, 192, True), (1, 13, 1, 256, False), (1, 2, 1, 1024, False),
          (1, 4100, 5, 4, False), (8, 130, 4, 16, True)]


@pytest.mark.parametrize("n_rep,T,F,hw,with_truth", SHAPES)
def test_every_kind_and_level_set_against_the_cpu_reference(n_rep, T, F, hw, with_truth):
    """variable f differs from its neighbours in offset and scale, so a wrong i % F fails"""
    for kind in R.KINDS:
        for level_set in R.LEVEL_SETS:
            s, t, q, out, stats, nv = R.case(kind, n_rep, T, F, hw, level_set, with_truth)
            go, gs, gn = select(s, t, q)
            assert R.same_stats(gs, stats), (kind, level_set)
            assert R.same_numbers(go, out), (kind, level_set)
            assert np.array_equal(gn, nv), (kind, level_set)


def test_unsupported_shapes_write_nothing_and_take_the_general_route():
    assert not ops.quantile_supported(66, 9) and not ops.quantile_supported(64, 17) and not ops.quantile_supported(64, 0)
    assert ops.quantile_supported(4, 1) and ops.quantile_supported(16384, 16)
    q17 = np.concatenate([R.levels("sixteen", 3 * 64), [0.123]])
    for hw, q in ((66, np.array(R.NINE)), (64, q17)):
        s, t = R.fields("nan", 2, 3, 2, hw)
        select(s, t, q, expect=False)
        H, W_ = (6, 11) if hw == 66 else (8, 8)
        (go, gs, gn), (to, ts, tn) = Qt.quantile(to_dev(s.reshape(2, 3, 2, H, W_))[0], q, truth=to_dev(t.reshape(3, 2, H, W_))[0], return_stats=True)
        assert go.is_cuda and go.shape == (2, 2, q.size) and to.shape == (2, q.size)
        want, stats, nv = R.expected(s, t, q)
        assert R.same_numbers(torch.cat([go.reshape(4, -1), to]).cpu().numpy(), want)
        assert R.same_stats(torch.cat([gs.reshape(4, -1, 2), ts]).cpu().numpy(), stats)
        assert np.array_equal(torch.cat([gn.reshape(-1), tn]).cpu().numpy(), nv)


def test_same_bits_at_every_position_and_alone():
    """one data set first, in the middle and last among the samples, as the truth, and alone"""
    T, hw = 13, 256
    s, t = R.fields("normal", 3, T, 2, hw)
    s, t = s.copy(), t.copy()
    s[1, :, 1] = s[2, :, 1] = t[:, 0] = s[0, :, 0]  # data sets 0, 3, 5 of the samples and 6, the truth's first
    q = R.levels("sixteen", T * hw)
    go, gs, gn = select(s, t, q)
    alone_o, alone_s, alone_n = select(s[:1, :, :1], None, q)
    for ds in (0, 3, 5, 6):
        assert np.array_equal(go[ds].view(np.uint64), alone_o[0].view(np.uint64)), ds
        assert np.array_equal(gs[ds].view(np.uint32), alone_s[0].view(np.uint32)) and gn[ds] == alone_n[0]
    assert not np.array_equal(go[1], alone_o[0])


def test_skipna_false_poisons_its_own_row_only():
    s, t = R.fields("normal", 3, 4, 2, 256)
    s, t = s.copy(), t.copy()
    s[1, 2, 0, 3] = np.nan
    t[3, 1, 255] = np.float32(np.nan)
    q = np.array(R.NINE)
    for skipna in (False, True):
        go, gs, gn = select(s, t, q, skipna=skipna)
        want, stats, nv = R.expected(s, t, q, skipna)
        assert R.same_numbers(go, want) and R.same_stats(gs, stats) and np.array_equal(gn, nv)
        bad = np.zeros(8, bool)
        bad[[2, 7]] = not skipna
        assert np.array_equal(np.isnan(go).all(axis=1), bad) and np.array_equal(np.isnan(go).any(axis=1), bad)
        assert gn.tolist() == [1024, 1024, 1023, 1024, 1024, 1024, 1024, 1023]


def test_two_calls_on_one_scratch_back_to_back():
    """the second call zeroes on the stream what the first one left"""
    a, ta = R.fields("pressure", 2, 5, 2, 64)
    b, tb = R.fields("ties", 2, 5, 2, 64, seed=1)
    q = np.array(R.NINE)
    shared = new_scratch(6, 9)
    first = select(a, ta, q, scratch=shared)
    second = select(b, tb, q, scratch=shared)
    third = select(a, ta, q, scratch=shared)
    fresh = select(b, tb, q)
    for x, y in zip(first, third):
        assert np.array_equal(x, y, equal_nan=True)
    for x, y in zip(second, fresh):
        assert np.array_equal(x, y, equal_nan=True)
    assert R.same_numbers(second[0], R.expected(b, tb, q)[0])


def test_public_functions_on_the_device_equal_their_cpu_results():
    rng = np.random.default_rng(9)
    off, sd = np.array([280.0, 101325.0]), np.array([10.0, 1200.0])
    truth = (off[None, :, None, None] + sd[None, :, None, None] * rng.standard_normal((5, 2, 16, 24))).astype(np.float32)
    samples = (off[None, None, :, None, None] + 1.3 * sd[None, None, :, None, None] * rng.standard_normal((3, 5, 2, 16, 24))).astype(np.float32)
    samples[1, 2, 0, 3, 3] = np.nan
    S, Tr = to_dev(samples, truth)
    for skipna in (True, False):
        (co, cs, cn), (cto, cts, ctn) = Qt.quantile(torch.tensor(samples), R.NINE, truth=torch.tensor(truth), skipna=skipna, return_stats=True)
        (go, gs, gn), (gto, gts, gtn) = Qt.quantile(S, R.NINE, truth=Tr, skipna=skipna, return_stats=True)
        assert go.is_cuda and go.dtype == torch.float64 and go.shape == (3, 2, 9) and gto.shape == (2, 9)
        assert R.same_numbers(go.cpu().numpy(), co.numpy()) and R.same_numbers(gto.cpu().numpy(), cto.numpy())
        assert R.same_stats(gs.cpu().numpy(), cs.numpy()) and R.same_stats(gts.cpu().numpy(), cts.numpy())
        assert torch.equal(gn.cpu(), cn) and torch.equal(gtn.cpu(), ctn)
    half = S.to(torch.float16)[..., ::2]  # strided and 16-bit: one dense fp32 copy, then the kernels
    assert R.same_numbers(Qt.quantile(half, [0.01, 0.99]).cpu().numpy(), Qt.quantile(half.cpu(), [0.01, 0.99]).numpy())
    cpu = Qt.quantile_report(torch.tensor(samples), torch.tensor(truth), names=["tas", "psl"])
    gpu = Qt.quantile_report(S, Tr, names=["tas", "psl"])
    for name, v in gpu:
        assert all(t.is_cuda for t in v.values())
        for k in ("truth", "samples", "diff"):
            assert R.same_numbers(v[k].cpu().numpy(), cpu[name][k].numpy()), (name, k)
    assert gpu.as_dict() == cpu.as_dict()


@pytest.mark.parametrize("mode", sorted(Nm.MODES))
def test_from_data_on_the_device_reproduces_the_numpy_normaliser(mode):
    """to the last bit of its fp32 coefficients"""
    rng = np.random.default_rng(3)
    off, sd = np.array([280.0, 101325.0, 0.0, 3e-5]), np.array([10.0, 900.0, 4.0, 2e-5])
    x = (off[None, :, None, None] + sd[None, :, None, None] * rng.standard_normal((6, 4, 16, 24))).astype(np.float32)
    levels = sorted(set(Nm.MODES[mode]))
    want = Nm.QuantileNormalizer({q: [np.quantile(x[:, f].astype(np.float64), q) for f in range(4)] for q in levels}, mode)
    got = Nm.QuantileNormalizer.from_data(to_dev(x)[0], mode)
    assert got.lower.is_cuda and torch.equal(got.lower.cpu(), want.lower) and torch.equal(got.range.cpu(), want.range)
    for inverse in (False, True):
        for a, b in zip(got._coef(dev(), inverse), want._coef(dev(), inverse)):
            assert a.dtype == torch.float32 and torch.equal(a, b)
    fields = to_dev(x)[0]
    assert torch.equal(got.unnormalize(got.normalize(fields)), want.unnormalize(want.normalize(fields)))
