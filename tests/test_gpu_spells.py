"""The event-spell kernel on the MI355X (csrc/spells.hip through spell_ops and climate2weather_amd.spells): the state and the tables
EQUAL to the NumPy reference of tests/fp64_spells_ref.py at the smallest shapes that can go wrong -- everything is integers, so no test
here carries a tolerance -- then the properties the interface promises: block splitting, the same integers wherever a row lies in the
launch and on a second accumulator, nothing written past the end, nothing written for unsupported arguments, a NaN or an infinity kept
in its own series, the same tables on another stream, a strided fp16 input equal to the dense route, every public function on the
device equal to the general route on CPU copies, and the known answers."""
import numpy as np
import pytest
import torch

import fp64_spells_ref as R
from climate2weather_amd import spell_ops
from climate2weather_amd import spells as SP

pytestmark = pytest.mark.gpu

CANARY = -7
TAIL = 64  # canary values behind each output


def dev():
    return torch.device("cuda:0")


def to_dev(*arrays):
    return [torch.tensor(np.asarray(a)).to(dev()) for a in arrays]


def _canaried(n, dtype):
    buf = torch.full((n + TAIL,), CANARY, dtype=dtype, device=dev())
    buf[:n] = 0  # the accumulators are zeroed by whoever makes them, not by the call
    return buf


def _kept(buf, n):
    return torch.equal(buf[n:], torch.full_like(buf[n:], CANARY))


def update(x, y, thr, above, Lmax, period, t0, expect=True):
    """One spell_ops.spell_update on x (M, T, F, hw), y (T, F, hw) or None from a zeroed state: (state (4, D, F, K, hw), hist, onsets,
    invalid) as int64 arrays; the TAIL values behind all four must keep the canary.  expect False: the call must answer False and leave
    every value alone."""
    M, T, F, hw = x.shape
    K, D = thr.shape[1], M + (0 if y is None else 1)
    xd, td, dd = to_dev(x, thr, above.astype(np.int32))
    yd = None if y is None else to_dev(y)[0]
    sizes = (4 * D * F * K * hw, D * F * K * Lmax, D * F * K * period, D * F)
    state, hist, onsets, invalid = (_canaried(n, torch.int32 if i == 0 else torch.int64) for i, n in enumerate(sizes))
    if not expect:
        for buf in (state, hist, onsets, invalid):
            buf.fill_(CANARY)
    ok = spell_ops.spell_update(xd, yd, td, dd, state, hist, onsets if period else None, invalid, M, T, F, hw, K, Lmax, period, t0)
    assert ok is expect
    for buf, n in zip((state, hist, onsets, invalid), sizes):
        assert _kept(buf, n if expect else 0)
    shapes = ((4, D, F, K, hw), (D, F, K, Lmax), (D, F, K, period), (D, F))
    return [buf[:n].view(s).cpu().numpy().astype(np.int64) for buf, n, s in zip((state, hist, onsets, invalid), sizes, shapes)]


def closed(state, hist, Lmax):
    """the tables with the open runs closed, as the definition says: (hist, hours, count, longest)"""
    open_, hist = state[0], hist.copy()
    for d, f, k in np.ndindex(*hist.shape[:3]):
        hist[d, f, k] += np.bincount(np.minimum(open_[d, f, k][open_[d, f, k] > 0], Lmax) - 1, minlength=Lmax)
    return hist, state[3], state[2] + (open_ > 0), np.maximum(state[1], open_)


def assert_tables(t, want, what=""):
    D, F, K = want["censored"].shape
    for name in ("hist", "onsets", "invalid", "censored"):
        assert np.array_equal(getattr(t, name).cpu().numpy(), want[name]), (name, what)
    for name in ("hours", "count", "longest"):
        assert np.array_equal(getattr(t, name).cpu().numpy().reshape(D, F, K, -1), want[name]), (name, what)


def same_tables(a, b, what=""):
    assert a.n_times == b.n_times
    for name in ("hist", "hours", "count", "longest", "onsets", "invalid", "censored"):
        assert torch.equal(getattr(a, name).cpu(), getattr(b, name).cpu()), (name, what)


# ------------------------------------------------------------------------------------------------------------------ against the reference

TS, KS, LS, PS = (1, 7, 8, 9, 33), (1, 3, 4, 5, 8), (1, 2, 48, 256), (0, 1, 6, 24)


@pytest.mark.parametrize("hw", [4, 1024, 1028, 2052])
def test_the_state_and_the_tables_equal_the_reference(hw):
    """one thread, one full chunk, a remainder chunk of one thread, three chunks; T around the unroll of 8; M in {1, 3} with and
    without a truth; K of one group, a full group and two groups; Lmax in {1, 2, 48, 256}; period in {0, 1, 6, 24}; t0 in {0, 5}.  Ten
    deals a shape: every value of every list meets every hw, the pairings shift, the kinds take turns.  Variable f differs from its
    neighbours in offset and scale, so a wrong index map fails."""
    F = 2
    for i in range(10):
        T, K, Lmax, period = TS[i % 5], KS[(i + i // 5) % 5], LS[(i + i // 4) % 4], PS[(i + 2 * (i // 4)) % 4]
        M, with_truth, t0 = (1, 3)[i % 2], (i // 2) % 2 == 0, (0, 5)[(i // 3) % 2]
        kind = R.KINDS[(i + [4, 1024, 1028, 2052].index(hw) * 3) % len(R.KINDS)]
        x, y = R.fields(kind, M, T, F, hw)
        thr, above = R.thresholds(kind, y, K), R.directions(F, K, ("mixed", "above", "below")[i % 3])
        y = y if with_truth else None
        state, hist, onsets, invalid = update(x, y, thr, above, Lmax, period, t0)
        want = R.spells_ref(x, y, thr, above, Lmax, period, t0)
        got = closed(state, hist, Lmax)
        what = (kind, T, K, Lmax, period, M, with_truth, t0)
        for g, name in zip(got, ("hist", "hours", "count", "longest")):
            assert np.array_equal(g, want[name]), (name,) + what
        assert np.array_equal(onsets, want["onsets"]) and np.array_equal(invalid, want["invalid"]), what


# ------------------------------------------------------------------------------------------------------------------ the promises

def test_block_splitting_on_the_device_equals_the_single_call_and_the_reference():
    """T = 17 as one block, as seventeen blocks of 1, as (8, 9) and as (5, 0, 12), at hw = 1028 and K = 5 (two chunks, two groups); the
    smooth field's spells are long, so the splits fall inside them; and across state_dict / load_state_dict"""
    M, T, F, H, W_, K, Lmax, period, t0 = 2, 17, 2, 4, 257, 5, 6, 6, 5
    x, y = R.fields("smooth", M, T, F, H * W_)
    thr, above = R.thresholds("smooth", y, K), R.directions(F, K, "mixed")
    S, Tr, th = to_dev(x.reshape(M, T, F, H, W_), y.reshape(T, F, H, W_), thr)
    names = R.direction_names(above)
    make = lambda: SP.SpellAccumulator(M, F, H, W_, th, names, max_duration=Lmax, period=period, t0=t0, device=dev())
    whole = make().update(S, Tr).tables()
    assert whole.hist.is_cuda
    assert_tables(whole, R.spells_ref(x, y, thr, above, Lmax, period, t0))
    for sizes in ((1,) * 17, (8, 9), (5, 0, 12)):
        acc, at = make(), 0
        for n in sizes:
            acc.update(S[:, at:at + n], Tr[at:at + n])
            at += n
        same_tables(acc.tables(), whole, sizes)
    saved = make().update(S[:, :8], Tr[:8]).state_dict()
    same_tables(make().load_state_dict(saved).update(S[:, 8:], Tr[8:]).tables(), whole, "resumed")


def test_the_same_series_give_the_same_integers_at_every_position_and_on_a_second_accumulator():
    """one row of one variable placed as the truth, as the last member, in the first and in the last variable, and alone"""
    M, T, F, hw, K, Lmax, period = 3, 19, 3, 1028, 5, 7, 6
    x, y = R.fields("periodic", M, T, F, hw)
    x, y = x.copy(), y.copy()
    p = x[1, :, 1].copy()                                                           # (T, hw)
    y[:, 0], x[2, :, 2] = p, p
    thr = np.repeat(R.thresholds("periodic", y[:, 1:2], K), F, axis=0)              # the same thresholds for every variable
    above = R.directions(F, K, "above")
    a, b = update(x, y, thr, above, Lmax, period, 4), update(x, y, thr, above, Lmax, period, 4)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    alone = update(p[None, :, None], None, thr[:1], above[:1], Lmax, period, 4)
    for d, f in ((2, 1), (0, 0), (3, 2)):
        assert np.array_equal(a[0][:, d, f], alone[0][:, 0, 0]) and np.array_equal(a[1][d, f], alone[1][0, 0]), (d, f)
        assert np.array_equal(a[2][d, f], alone[2][0, 0]), (d, f)
    assert not np.array_equal(a[1][1, 1], alone[1][0, 0])


def test_unsupported_arguments_write_nothing_and_take_the_general_route():
    assert not spell_ops.supported(6, 2, 4, 6) and not spell_ops.supported(8, 9, 4, 6) and not spell_ops.supported(8, 2, 257, 6)
    assert not spell_ops.supported(8, 2, 4, 25) and not spell_ops.supported(8, 0, 4, 0) and not spell_ops.supported(8, 1, 0, 0)
    assert spell_ops.supported(4, 1, 1, 0) and spell_ops.supported(16384, 8, 256, 24)
    for hw, K, Lmax, period in ((6, 2, 4, 6), (8, 9, 4, 6), (8, 2, 257, 6), (8, 2, 4, 25)):
        x, y = R.fields("smooth", 2, 9, 1, hw)
        thr, above = R.thresholds("smooth", y, K), R.directions(1, K, "mixed")
        update(x, y, thr, above, Lmax, period, 2, expect=False)
        S, Tr, th = to_dev(x.reshape(2, 9, 1, 1, hw), y.reshape(9, 1, 1, hw), thr)
        t = SP.spell_tables(S, Tr, th, R.direction_names(above), Lmax, period, 2)
        assert t.hist.is_cuda
        assert_tables(t, R.spells_ref(x, y, thr, above, Lmax, period, 2), (hw, K, Lmax, period))


def test_a_nan_or_an_infinity_stays_in_its_own_series():
    M, T, F, hw, K, Lmax, period = 2, 12, 2, 1028, 2, 5, 6
    x, y = R.fields("smooth", M, T, F, hw)
    thr, above = R.thresholds("smooth", y, K), R.directions(F, K, "mixed")
    clean = update(x, y, thr, above, Lmax, period, 0)
    x, y = x.copy(), y.copy()
    x[1, 5, 0, 1027] = np.nan     # the last cell: the second chunk
    y[3, 1, 0] = np.inf
    x[0, 7, 1, 513] = -np.inf
    got = update(x, y, thr, above, Lmax, period, 0)
    touched = np.zeros((M + 1, F, hw), bool)
    touched[2, 0, 1027] = touched[0, 1, 0] = touched[1, 1, 513] = True
    keep = ~touched[None, :, :, None, :].repeat(4, axis=0).repeat(K, axis=3)
    assert np.array_equal(got[0][keep], clean[0][keep]) and int(clean[3].sum()) == 0
    assert got[3].tolist() == [[0, 0], [0, 0], [1, 0]]
    want = R.spells_ref(x, y, thr, above, Lmax, period, 0)
    hist, hours, count, longest = closed(got[0], got[1], Lmax)
    assert np.array_equal(hist, want["hist"]) and np.array_equal(hours, want["hours"]) and np.array_equal(count, want["count"])
    assert np.array_equal(longest, want["longest"]) and np.array_equal(got[2], want["onsets"])
    assert np.array_equal(got[1][1, 0], clean[1][1, 0]) and np.array_equal(got[1][2, 1], clean[1][2, 1])  # rows of the tables nothing touched


def test_a_call_on_another_stream_gives_the_same_tables():
    x, y = R.fields("pressure", 3, 21, 2, 2052)
    thr = R.thresholds("pressure", y, 5)
    S, Tr, th = to_dev(x.reshape(3, 21, 2, 36, 57), y.reshape(21, 2, 36, 57), thr)
    want = SP.spell_tables(S, Tr, th, "below", 12, 6, 3)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = SP.spell_tables(S, Tr, th, "below", 12, 6, 3)
    side.synchronize()
    same_tables(got, want)
    assert_tables(want, R.spells_ref(x, y, thr, R.directions(2, 5, "below"), 12, 6, 3))


def test_strided_half_precision_input_agrees_with_the_dense_route():
    base = (torch.randn(3, 15, 2, 16, 64, device=dev()) * 3.0 + 1.0).to(torch.float16)
    view, truth = base[..., ::2], base[0, ..., 1::2]
    dense, dtruth = view.float().contiguous(), truth.float().contiguous()
    thr = torch.tensor([[0.5, 4.0], [1.0, -2.0]], dtype=torch.float64)
    a = SP.spell_tables(view, truth, thr, ["above", "below"], 6, 4)
    b = SP.spell_tables(dense, dtruth, thr.float().to(dev()), ["above", "below"], 6, 4)
    same_tables(a, b)
    assert int(a.hours.sum()) > 0 and a.n_times == 15


# ------------------------------------------------------------------------------------------------------------------ the public functions

def test_public_functions_on_the_device_equal_the_general_route_on_cpu_copies():
    """(M, T, F) = (4, 26, 2) at 40 x 52, smooth and pressure-like, a NaN included: every public function through the kernel against
    the same function through the general torch route on CPU copies -- equal, since the tables are the same integers and the algebra is
    the same float64 code"""
    M, T, F, H, W_, K = 4, 26, 2, 40, 52, 3
    xs, ys = R.fields("smooth", M, T, 1, H * W_)
    xp, yp = R.fields("pressure", M, T, 1, H * W_)
    x, y = np.concatenate([xs, xp], axis=2), np.concatenate([ys, yp], axis=1)
    x[2, 11, 0, 77] = np.nan
    thr = np.concatenate([R.thresholds("smooth", ys, K), R.thresholds("pressure", yp, K)])
    S, Tr, th = to_dev(x.reshape(M, T, F, H, W_), y.reshape(T, F, H, W_), thr)

    def everything(S, Tr, th):
        acc = SP.SpellAccumulator(M, F, H, W_, th, ["above", "below", "above"], max_duration=10, period=6, t0=3, device=S.device)
        acc.update(S[:, :9], Tr[:9]).update(S[:, 9:], Tr[9:])
        t = acc.tables()
        u = SP.spell_tables(S, None, th, "above", 4, 0, 0)
        out = [t.hist, t.hours, t.count, t.longest, t.onsets, t.invalid, t.censored, u.hist, u.hours, u.count, u.longest, u.onsets, u.censored,
               SP.duration_pmf(t.hist), SP.survival(t.hist), SP.mean_duration(t.hours, t.count), SP.event_frequency(t.hours, t.n_times),
               SP.spell_duration_distance(t.hist), *SP.longest_spell_error(t.longest), SP.onset_share(t.onsets)]
        rep = SP.spells_report(S, Tr, th, ["above", "below", "above"], 10, 6, 3, names=["tas", "psl"])
        for _, v in rep:
            out += [v[k] for k in sorted(v)]
        return out, rep.as_dict(), t.n_times

    kernel, kernel_flat, n = everything(S, Tr, th)
    general, general_flat, n2 = everything(S.cpu(), Tr.cpu(), th.cpu())
    assert len(kernel) == len(general) and all(t.is_cuda for t in kernel) and n == n2 == T
    for i, (a, b) in enumerate(zip(kernel, general)):
        a = a.cpu()
        assert a.dtype == b.dtype and a.shape == b.shape, i
        if a.is_floating_point():
            assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0)), i
        else:
            assert torch.equal(a, b), i
    assert kernel_flat == general_flat and int(kernel[5].sum()) == 1


def test_the_periodic_and_the_alternating_known_answers():
    a, p, n, cells = 2, 6, 5, 1028
    row = torch.tensor([1.0 if t % p < a else 0.0 for t in range(n * p)], device=dev())
    alt = torch.tensor([1.0 - t % 2 for t in range(n * p - 1)], device=dev())
    S = row.view(1, -1, 1, 1, 1).expand(2, -1, 1, 4, 257).contiguous()
    t = SP.spell_tables(S, S[0], torch.tensor([[1.0]]), max_duration=8, period=p)
    hist = [0] * 8
    hist[a - 1] = n * cells
    assert t.hist.view(3, 8).tolist() == [hist] * 3 and t.onsets.view(3, p).tolist() == [[n * cells] + [0] * (p - 1)] * 3
    for got, want in ((t.hours, n * a), (t.longest, a), (t.count, n)):
        assert torch.equal(got, torch.full_like(got, want))
    assert t.censored.flatten().tolist() == [cells] * 3
    S = alt.view(1, -1, 1, 1, 1).expand(1, -1, 1, 4, 257).contiguous()
    t = SP.spell_tables(S, None, torch.tensor([[1.0]]), max_duration=3, period=2)
    T = n * p - 1
    assert t.hist.flatten().tolist() == [cells * (T + 1) // 2, 0, 0] and torch.equal(t.count, torch.full_like(t.count, (T + 1) // 2))
    assert t.onsets.flatten().tolist() == [cells * (T + 1) // 2, 0] and t.censored.item() == 2 * cells
    assert torch.equal(t.longest, torch.ones_like(t.longest)) and torch.equal(t.hours, torch.full_like(t.hours, (T + 1) // 2))
