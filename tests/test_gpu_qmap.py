"""The quantile-mapping kernels on the MI355X (csrc/qmap.hip through qmap_ops and climate2weather_amd.biascorrect): the nodes against
numpy on the float64 series as numbers; the mapping within the bound of tests/fp64_qmap_ref.py at every element, and its exact answers
-- identity, shift, monotone, in place; then the properties the interface promises: the same bits wherever a series lies in the launch
and on a second call, nothing written past the end of an output or of the scratch, nothing written for an unsupported shape, a
non-finite value kept in its own series and elements, the same result on another stream, and the public functions on the device
against the general float64 route.

profiles/qmap_measurements.md has the observed worst fraction of the bound per kind."""
import numpy as np
import pytest
import torch

import fp64_qmap_ref as R
from climate2weather_amd import biascorrect as BC
from climate2weather_amd import qmap_ops

pytestmark = pytest.mark.gpu

CANARY = -7.25
TAIL = 64  # canary values behind each output
F = 2
LENGTHS = (1, 2, 3, 255, 256, 257, 1025, 16384)
KS = (2, 9, 101, 128)


def dev():
    return torch.device("cuda:0")


def to_dev(*arrays):
    return [None if a is None else torch.tensor(np.ascontiguousarray(a)).to(dev()) for a in arrays]


def lists(ids, G):
    idx = R.index_lists(ids, G)
    tidx = np.array([t for i in idx for t in i], np.int32)
    goff = np.cumsum([0] + [len(i) for i in idx]).astype(np.int32)
    return tidx, goff, max(len(i) for i in idx)


def nodes(x, ids, G, levels, skipna=True, block=1024, expect=True):
    """(q (n_rep, G, F, hw, K) float64, n_valid int64) from qmap_ops.qmap_nodes on x (n_rep, T, F, hw), the cells in blocks of ``block``;
    the TAIL values behind q, n_valid and the scratch must keep the canary.  expect False: every call must answer False and leave every
    value of the three buffers alone."""
    n_rep, T, F_, hw = x.shape
    K = len(levels)
    tidx, goff, max_len = lists(ids, G)
    xd, td, gd, lv = to_dev(x, tidx, goff, np.asarray(levels, np.float64))
    n = n_rep * G * F_ * hw
    q = torch.full((n * K + TAIL,), CANARY, dtype=torch.float64, device=dev())
    nv = torch.full((n + TAIL,), -7, dtype=torch.int64, device=dev())
    block = min(block, hw)
    nws = qmap_ops.qmap_scratch_bytes(n_rep * F_, block, T) // 4
    ws = torch.full((nws + TAIL,), CANARY, dtype=torch.float32, device=dev())
    for c0 in range(0, hw, block):
        ok = qmap_ops.qmap_nodes(xd, td, gd, lv, q, nv, ws[:nws], n_rep, T, F_, hw, T, G, K, max_len, skipna, c0, min(hw, c0 + block))
        assert ok is expect
    assert torch.equal(q[n * K if expect else 0:], torch.full_like(q[n * K if expect else 0:], CANARY))
    assert torch.equal(nv[n if expect else 0:], torch.full_like(nv[n if expect else 0:], -7))
    assert torch.equal(ws[nws if expect else 0:], torch.full_like(ws[nws if expect else 0:], CANARY))
    return q[:n * K].view(n_rep, G, F_, hw, K), nv[:n].view(n_rep, G, F_, hw)


def apply(x, xq, yq, ids, in_place=False, expect=True):
    """out (n_rep, T, F, hw) fp32 from qmap_ops.qmap_apply; the TAIL values behind it must keep the canary"""
    n_rep, T, F_, hw = x.shape
    G, K = xq.shape[0], xq.shape[-1]
    tidx, goff, max_len = lists(ids, G)
    xd, td, gd, xqd, yqd = to_dev(x, tidx, goff, xq, yq)
    n = x.size
    out = torch.full((n + TAIL,), CANARY, dtype=torch.float32, device=dev())
    if in_place:
        out[:n] = xd.view(-1)
        xd = out[:n]
    ok = qmap_ops.qmap_apply(xd, out, xqd, yqd, td, gd, n_rep, T, F_, hw, T, G, K, max_len)
    assert ok is expect
    assert torch.equal(out[n if expect else 0:], torch.full_like(out[n if expect else 0:], CANARY))
    return out[:n].view(n_rep, T, F_, hw)


def group_ids(n, G):
    """G = 1: n times of group 0.  G = 3: group 0 has n times, group 1 none, group 2 n // 2 + 1, interleaved"""
    if G == 1:
        return [0] * n
    m = n // 2 + 1
    ids = [0, 2] * min(n, m) + [0] * (n - min(n, m)) + [2] * (m - min(n, m))
    return ids


# ------------------------------------------------------------------------------------------------------------------ nodes

@pytest.mark.parametrize("hw", [4, 64, 4100])
def test_the_nodes_equal_numpy_as_numbers(hw):
    """series lengths 1 .. 16384 (16384 at hw = 64 only), K in {2, 9, 101, 128} (all four at hw 4 and 64, taking turns at 4100, where
    the reference is the cost), G in {1, 3} uneven with one empty group, with and without leading members, NaNs skipped and not; the
    field kinds take turns.  One reference per (length, G): all its level sets at once."""
    k = 0
    for n in LENGTHS:
        if n == 16384 and hw != 64:
            continue
        for G in (1, 3):
            if hw == 4100 and n == 1025 and G == 3:
                continue  # the longest fields of the file: one group is enough there
            kind = R.KINDS[k % len(R.KINDS)]
            n_rep = 1 + k % 2 if n < 1025 and hw < 4100 else 1  # leading members at the two small sizes: the reference is the cost
            skipna = k % 3 != 2
            ks = KS if hw < 4100 else (KS[(k + k // 4) % 4],)
            k += 1
            ids = group_ids(n, G)
            x = R.fields(kind, n_rep, len(ids), F, hw)
            want, cnt = R.nodes64(x, ids, G, np.concatenate([R.levels_of(K) for K in ks]), skipna)
            at = 0
            for K in ks:
                q, nv = nodes(x, ids, G, R.levels_of(K), skipna)
                assert R.same_numbers(q.cpu().numpy(), want[..., at:at + K]), (kind, n, G, K, n_rep, skipna)
                assert np.array_equal(nv.cpu().numpy(), cnt)
                at += K
            if G == 3:
                assert torch.isnan(q[:, 1]).all() and int(nv[:, 1].abs().sum()) == 0


def test_the_public_quantiles_with_leading_members_equal_the_cpu_general_route():
    x = R.fields("temperature", 3, 130, F, 24 * 16)
    ids = torch.tensor(group_ids(86, 3))
    xt = torch.tensor(x).view(3, 130, F, 24, 16)
    want, cnt = BC.cell_quantiles(xt, 101, groups=ids, n_groups=3, return_counts=True)
    got, nv = BC.cell_quantiles(xt.to(dev()), 101, groups=ids, n_groups=3, return_counts=True)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (3, 3, F, 24, 16, 101)
    assert R.same_numbers(got.cpu().numpy(), want.numpy()) and torch.equal(nv.cpu(), cnt)
    half = xt.to(dev()).to(torch.float16)[..., ::2]
    assert torch.equal(BC.cell_quantiles(half, 9), BC.cell_quantiles(half.float().contiguous(), 9))


# ------------------------------------------------------------------------------------------------------------------ apply

def tables(kind, n, G, K, hw, seed=0):
    """the {xq, yq} (G, F, hw, K) a fit hands over, from the kernel's own nodes, and the group ids of the fit"""
    ids = group_ids(n, G)
    m, r = R.fields(kind, 1, len(ids), F, hw, seed=seed), R.fields(kind, 1, len(ids), F, hw, seed=seed + 1) * 1.1 + 0.5
    xq, yq = nodes(m, ids, G, R.levels_of(K))[0][0].cpu().numpy(), nodes(r.astype(np.float32), ids, G, R.levels_of(K))[0][0].cpu().numpy()
    bad = (np.isnan(xq).any(-1) | np.isnan(yq).any(-1))[..., None]
    return np.where(bad, np.nan, xq), np.where(bad, np.nan, yq)


@pytest.mark.parametrize("kind,hw,K", [("pressure", 64, 9), ("temperature", 4100, 101), ("wind", 4, 128), ("temperature", 100, 2)])
def test_the_mapping_is_within_the_bound_at_every_element(kind, hw, K):
    """cell blocks of 64 and 32 cells, whole and partial; three groups, one of them empty; inside the range against numpy.interp within
    the bound, in the tails the stated formula exactly, in the empty group NaN"""
    xq, yq = tables(kind, 257, 3, K, hw)
    assert np.all(np.diff(xq[[0, 2]], axis=-1) > 0)
    ids = [0, 2, 1, 0, 0, 2] * 5
    x = R.fields(kind, 2, len(ids), F, hw, seed=8)
    got = apply(x, xq, yq, ids).cpu().numpy()
    want, allow = R.interp64(x, xq, yq, ids)
    inside = ~np.isnan(want)
    frac = np.abs(got.astype(np.float64) - want)[inside] / allow[inside]
    print(f"{kind} hw {hw} K {K}: worst fraction of the bound {frac.max():.3g} over {int(inside.sum())} values")
    assert inside.sum() > x.size // 4 and np.all(frac <= 1.0)
    gid = np.asarray(ids)
    below, above, tail = R.tails64(x[:, gid != 1], xq, yq, gid[gid != 1])
    assert np.array_equal(got[:, gid != 1][below | above], tail[below | above])
    assert np.isnan(got[:, gid == 1]).all() and not np.isnan(got[:, gid != 1]).any()
    assert R.same_bits(apply(x, xq, yq, ids, in_place=True).cpu().numpy(), got)


def test_identity_shift_and_monotone_are_exact():
    hw, n = 68, 120
    for kind in R.EXACT_KINDS:  # a model mapped onto itself: every bit of x, beyond the range included
        m = R.fields(kind, 1, n, F, hw)
        xq = nodes(m, [0] * n, 1, R.levels_of(101))[0][0].cpu().numpy()
        centre = m.mean(axis=1, keepdims=True)
        x = (centre + 1.6 * (R.fields(kind, 2, 50, F, hw, seed=1) - centre)).astype(np.float32)
        assert (x > m.max(axis=1)).any() and (x < m.min(axis=1)).any()
        assert R.same_bits(apply(x, xq, xq, [0] * 50).cpu().numpy(), x), kind
    rng = np.random.default_rng(0)  # reference = model + c per cell on small integers: x + c everywhere
    m = rng.integers(-40, 41, (1, n, F, hw)).astype(np.float32)
    c = rng.integers(-9, 10, (1, 1, F, hw)).astype(np.float32)
    xq, yq = (nodes(v, [0] * n, 1, R.levels_of(21))[0][0].cpu().numpy() for v in (m, m + c))
    x = rng.integers(-60, 61, (2, 50, F, hw)).astype(np.float32)
    assert R.same_bits(apply(x, xq, yq, [0] * 50).cpu().numpy(), x + c)
    for kind in ("temperature", "ties"):  # sorted x gives non-decreasing output, repeated nodes and the nodes' neighbours included
        xq, yq = tables(kind, 100, 1, 17, hw)
        near = xq[0].astype(np.float32)
        near = np.moveaxis(np.concatenate([near, np.nextafter(near, np.float32(np.inf)), np.nextafter(near, np.float32(-np.inf))], -1), -1, 0)
        x = np.sort(np.concatenate([near, R.fields(kind, 1, 300, F, hw, seed=6)[0] * 1.3], axis=0), axis=0)[None]
        got = apply(x, xq, yq, [0] * x.shape[1]).cpu().numpy()
        assert np.all(np.diff(got, axis=1) >= 0), kind


# ------------------------------------------------------------------------------------------------------------------ the promises

def test_the_same_series_gives_the_same_bits_at_every_position():
    """one series as the first and the last cell of a plane, in both variables, both members and two groups; alone; on a second call"""
    n_rep, hw, n, K = 2, 4100, 70, 101
    ids = [0, 1] * n
    x = R.fields("temperature", n_rep, 2 * n, F, hw)
    series = x[0, 0::2, 0, 17].copy()
    x[0, 0::2, 0, 0] = x[1, 1::2, 1, hw - 1] = x[1, 0::2, 0, 2049] = series
    a, na = nodes(x, ids, 2, R.levels_of(K))
    b, _ = nodes(x, ids, 2, R.levels_of(K), block=64)  # another split into cell blocks, the second call
    assert torch.equal(a, b)
    alone = nodes(np.ascontiguousarray(np.broadcast_to(series[None, :, None, None], (1, n, 1, 4))), [0] * n, 1, R.levels_of(K))[0][0, 0, 0, 0]
    for rep, g, f, c in ((0, 0, 0, 17), (0, 0, 0, 0), (1, 1, 1, hw - 1), (1, 0, 0, 2049)):
        assert torch.equal(a[rep, g, f, c], alone), (rep, g, f, c)
    assert not torch.equal(a[0, 0, 0, 18], alone) and int(na.min()) == n
    # the mapping: the same values through the same tables at four positions
    xq, yq = a[0].cpu().numpy().copy(), (a[1].cpu().numpy() * 1.25 + 3.0)
    for g, f, c in ((0, 0, 0), (1, 1, hw - 1), (0, 0, 2049)):
        xq[g, f, c], yq[g, f, c] = xq[0, 0, 17], yq[0, 0, 17]
    v = R.fields("temperature", n_rep, 2 * n, F, hw, seed=3)
    v[0, 0::2, 0, 0] = v[1, 1::2, 1, hw - 1] = v[1, 0::2, 0, 2049] = v[0, 0::2, 0, 17]
    y, y2 = apply(v, xq, yq, ids), apply(v, xq, yq, ids)
    assert torch.equal(y, y2)
    for rep, g, f, c in ((0, 0, 0, 0), (1, 1, 1, hw - 1), (1, 0, 0, 2049)):
        assert torch.equal(y[rep, g::2, f, c], y[0, 0::2, 0, 17]), (rep, g, f, c)


def test_unsupported_shapes_write_nothing_and_take_the_general_route():
    assert not qmap_ops.qmap_supported(6, 9, 30) and not qmap_ops.qmap_supported(64, 129, 30) and not qmap_ops.qmap_supported(64, 9, 16385)
    assert not qmap_ops.qmap_supported(64, 1, 30) and qmap_ops.qmap_supported(4, 2, 0) and qmap_ops.qmap_supported(16384, 128, 16384)
    assert qmap_ops.qmap_scratch_bytes(8, 64, 100) == 8 * 64 * 100 * 4
    for H, W_, K, n in ((2, 3, 9, 30), (2, 4, 129, 30), (2, 2, 9, 16385)):  # hw = 6; K = 129; a series of 16 385 values
        hw = H * W_
        x = R.fields("temperature", 1, n, F, hw)
        nodes(x, [0] * n, 1, R.levels_of(K), expect=False)
        t = np.sort(R.fields("temperature", 1, K, F, hw, seed=1)[0], axis=0)
        xq = np.ascontiguousarray(np.moveaxis(t, 0, -1)[None]).astype(np.float64)
        apply(x, xq, xq + 1.0, [0] * n, expect=False)
        xt = torch.tensor(x[0]).view(n, F, H, W_)
        cpu = BC.QuantileMapping.fit(xt, xt * 1.5, levels=K)
        gpu = BC.QuantileMapping.fit(xt.to(dev()), xt.to(dev()) * 1.5, levels=K)
        assert gpu.xq.is_cuda and R.same_numbers(gpu.xq.cpu().numpy(), cpu.xq.numpy()) and R.same_numbers(gpu.yq.cpu().numpy(), cpu.yq.numpy())
        v = torch.tensor(R.fields("temperature", 2, 40, F, hw, seed=2)).view(2, 40, F, H, W_)
        assert R.same_numbers(gpu.apply(v.to(dev())).cpu().numpy(), cpu.apply(v).numpy())


def test_a_non_finite_value_stays_in_its_own_series_and_elements():
    hw, n, K = 68, 90, 33
    ids = [0, 1, 1] * (n // 3)
    m = R.fields("wind", 1, n, F, hw)
    clean, nclean = nodes(m, ids, 2, R.levels_of(K))
    dirty = m.copy()
    dirty[0, 3, 0, 5] = np.nan       # group 0
    dirty[0, 4, 1, 67] = np.inf      # group 1, the last cell
    dirty[0, 7, 0, 64] = -np.inf     # group 1, the second tile of cells
    dirty.view(np.uint32)[0, 10, 1, 0] = 0xFFC00001  # a NaN with the sign bit set, group 1
    q, nv = nodes(dirty, ids, 2, R.levels_of(K))
    touched = torch.zeros(1, 2, F, hw, dtype=torch.bool, device=dev())
    for g, f, c in ((0, 0, 5), (1, 1, 67), (1, 0, 64), (1, 1, 0)):
        touched[0, g, f, c] = True
    lost = torch.zeros_like(touched)  # the two NaNs are not counted; an infinity is a value
    lost[0, 0, 0, 5] = lost[0, 1, 1, 0] = True
    assert torch.equal(q[~touched], clean[~touched]) and torch.equal(nv, nclean - lost.long())
    assert R.same_numbers(q.cpu().numpy(), R.nodes64(dirty, ids, 2, R.levels_of(K))[0])
    strict, _ = nodes(dirty, ids, 2, R.levels_of(K), skipna=False)
    assert torch.isnan(strict[0, 0, 0, 5]).all() and torch.isnan(strict[0, 1, 1, 0]).all() and torch.equal(strict[~touched], clean[~touched])
    # the mapping: a NaN or an infinity of x stays in its element; a NaN row stays in its cell and group
    xq, yq = clean[0].cpu().numpy().copy(), clean[0].cpu().numpy() * 2.0 + 1.0
    xq[1, 0, 9], yq[1, 0, 9] = np.nan, np.nan
    x = R.fields("wind", 2, n, F, hw, seed=1)
    base = apply(x, xq, yq, ids).cpu().numpy()
    v = x.copy()
    v[1, 5, 1, 66], v[0, 0, 0, 0], v[0, 1, 1, 3] = np.nan, np.inf, -np.inf
    got = apply(v, xq, yq, ids).cpu().numpy()
    changed = np.zeros(x.shape, bool)
    changed[1, 5, 1, 66] = changed[0, 0, 0, 0] = changed[0, 1, 1, 3] = True
    assert R.same_bits(got[~changed], base[~changed])
    assert np.isnan(got[1, 5, 1, 66]) and got[0, 0, 0, 0] == np.inf and got[0, 1, 1, 3] == -np.inf
    row = np.zeros(x.shape, bool)
    row[:, np.asarray(ids) == 1, 0, 9] = True
    assert np.array_equal(np.isnan(base), row)


def test_a_call_on_another_stream_gives_the_same_result():
    m, r = R.fields("pressure", 1, 300, F, 4100)[0], R.fields("pressure", 1, 290, F, 4100, seed=1)[0]
    ids, ids_r = BC.calendar_groups("2000-12-25-00", 300, step_hours=6), BC.calendar_groups("2000-12-25-00", 290, step_hours=6)
    md, rd, xd = (torch.tensor(v).view(v.shape[:-1] + (41, 100)).to(dev()) for v in (m, r, R.fields("pressure", 2, 300, F, 4100, seed=2)))
    want = BC.QuantileMapping.fit(md, rd, model_groups=ids, reference_groups=ids_r, n_groups=12)
    y = want.apply(xd, ids)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = BC.QuantileMapping.fit(md, rd, model_groups=ids, reference_groups=ids_r, n_groups=12)
        y2 = got.apply(xd, ids)
    side.synchronize()
    assert R.same_numbers(got.xq.cpu().numpy(), want.xq.cpu().numpy()) and R.same_numbers(got.yq.cpu().numpy(), want.yq.cpu().numpy())
    assert R.same_numbers(y2.cpu().numpy(), y.cpu().numpy()) and not torch.isnan(y).any()


def test_the_public_mapping_on_the_device_equals_the_cpu_general_route():
    """fit, apply (also in place), the state dict across devices and the report: the kernels' numbers are the general route's"""
    T, Tr, H, W_ = 400, 333, 16, 24
    m = np.concatenate([R.fields("temperature", 1, T, 1, H * W_)[0], R.fields("wind", 1, T, 1, H * W_)[0]], axis=1)
    r = np.concatenate([R.fields("temperature", 1, Tr, 1, H * W_, seed=1)[0] * 0.8 + 50.0, R.fields("wind", 1, Tr, 1, H * W_, seed=1)[0] * 1.4], axis=1)
    ids, ids_r = BC.calendar_groups("1999-11-01-00", T, step_hours=6, by="season"), BC.calendar_groups("1999-11-01-00", Tr, step_hours=6, by="season")
    mt, rt = torch.tensor(m).view(T, F, H, W_), torch.tensor(r.astype(np.float32)).view(Tr, F, H, W_)
    cpu = BC.QuantileMapping.fit(mt, rt, model_groups=ids, reference_groups=ids_r, n_groups=4)
    gpu = BC.QuantileMapping.fit(mt.to(dev()), rt.to(dev()), model_groups=ids, reference_groups=ids_r, n_groups=4)
    for k, v in gpu.state_dict().items():
        assert v.is_cuda and R.same_numbers(v.cpu().numpy(), cpu.state_dict()[k].numpy()), k
    x = torch.tensor(R.fields("temperature", 3, T, F, H * W_, seed=5)).view(3, T, F, H, W_)
    want = cpu.apply(x, ids)
    got = gpu.apply(x.to(dev()), ids)
    assert got.is_cuda and got.dtype == torch.float32 and R.same_numbers(got.cpu().numpy(), want.numpy())
    buf = x.to(dev())
    assert gpu.apply(buf, ids, out=buf) is buf and torch.equal(buf, got)
    moved = BC.QuantileMapping.from_state_dict(cpu.state_dict()).to(dev())
    assert torch.equal(moved.apply(x.to(dev()), ids), got)
    rc, rg = BC.bias_report(mt, rt, cpu, groups=ids), BC.bias_report(mt.to(dev()), rt.to(dev()), gpu, groups=ids)
    for name, v in rg:
        for key, t in v.items():
            assert t.is_cuda and R.same_numbers(t.cpu().numpy(), rc[name][key].numpy()), (name, key)
