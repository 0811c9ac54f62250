"""TEST DOUBLE for the wind-power launchers (climate2weather_amd.wind_ops: wind_supported, wind_table_bytes, wind_table,
wind_scratch_bytes, wind_power), on CPU tensors.

It restates csrc/wind_core.h in NumPy: the table builder byte for byte (the fp32 knots, the slopes formed in float64 from the rounded
knots, the bucket index and the mode), the chunk bounds, the (round, thread, column) -> cell map, the per-thread accumulation order
(the fold through LDS and the fold over the chunks are emu_ordered_sum's) -- and the kernel's arithmetic in fp32, operation by
operation and in the kernel's order, no multiply fused with an add.  The interval of a speed is found by a plain search over the fp32
knots: the bucket index and the bisection of the kernel are two ways to the same interval, and tests/host_wind_main.cpp holds both to
this restatement bit for bit.  Unsupported shapes answer False and write nothing.  ``install`` also makes the windpower module treat CPU
tensors as device tensors, so the host code takes the launcher's branch.
"""
from __future__ import annotations

import sys

import numpy as np
import torch

from emu_ordered_sum import fold_parts, fold_workgroup, nan_if_nan, seq_sum

CALLS = []  # (planes, F, u, v, K, hw, with_derived) of every call that reached the launcher

THREADS, MAX_K, BUCKETS, SCAN, ROUNDS = 256, 256, 256, 2, 4
CHUNK = ROUNDS * THREADS * 4
MODE_BUCKETS, MODE_BISECT = 0, 1
F32_MAX = float(np.finfo(np.float32).max)
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ wind_core.h, restated

def chunks(hw):
    return (hw + CHUNK - 1) // CHUNK


def chunk_bounds(hw, c):
    return c * CHUNK, min(hw, (c + 1) * CHUNK)


def wind_supported(hw, K):
    return hw >= 4 and hw % 4 == 0 and 2 <= K <= MAX_K


def wind_table_bytes(K):
    return 32 + 16 * (K - 1) + 2 * BUCKETS if 2 <= K <= MAX_K else 0


def wind_scratch_bytes(planes, hw):
    return planes * chunks(hw) * 2 * 8 if planes >= 1 and hw >= 1 and chunks(hw) > 1 else 0


def bucket_of(s, x0, inv):
    """fp32 arrays or scalars: min(int((s - x0) inv), BUCKETS - 1), every operation in fp32"""
    d = (np.asarray(s, f32) - f32(x0)).astype(f32)
    return np.minimum((d * f32(inv)).astype(f32).astype(np.int32), BUCKETS - 1)


def table_parts(xs, ps):
    """(x^ (K,), p^ (K,), slope (K - 1,) fp32, inv fp32, mode, start (BUCKETS,) uint16), or None where build_table refuses"""
    xs, ps = np.asarray(xs, np.float64), np.asarray(ps, np.float64)
    K = xs.shape[0]
    if not 2 <= K <= MAX_K:
        return None
    if not (np.all(np.abs(xs) <= F32_MAX) and np.all(np.abs(ps) <= F32_MAX)):  # NaN too
        return None
    xf, pf = xs.astype(f32), ps.astype(f32)
    if not (np.all(xs[1:] > xs[:-1]) and np.all(xf[1:] > xf[:-1])):
        return None
    slope = (pf[1:].astype(np.float64) - pf[:-1].astype(np.float64)) / (xf[1:].astype(np.float64) - xf[:-1].astype(np.float64))
    if not np.all(np.abs(slope) <= F32_MAX):
        return None
    wide = BUCKETS / (float(xf[-1]) - float(xf[0]))
    inv = f32(wide) if wide <= F32_MAX else f32(0)
    mode = MODE_BUCKETS if wide <= F32_MAX else MODE_BISECT
    start = np.zeros(BUCKETS, np.uint16)
    if mode == MODE_BUCKETS:
        b = bucket_of(xf[:-1], xf[0], inv)  # the last knot is no interval's start
        if np.bincount(b, minlength=BUCKETS).max() > SCAN:
            mode = MODE_BISECT
        for a in range(BUCKETS):
            below = np.flatnonzero(b < a)
            start[a] = below[-1] if below.size else 0
    return xf, pf, slope.astype(f32), inv, mode, start


def wind_table(xs, ps):
    """the packed table as uint8, byte for byte what c2w_wind_table writes; None where it refuses"""
    parts = table_parts(xs, ps)
    if parts is None:
        return None
    xf, pf, slope, inv, mode, start = parts
    K = xf.shape[0]
    head = np.zeros(8, np.uint32)
    head[:4] = np.array([xf[0], xf[-1], pf[-1], inv], f32).view(np.uint32)
    head[4], head[5] = K, mode
    entries = np.stack([xf[:-1], pf[:-1], slope, xf[1:]], axis=1).astype(f32)
    out = np.concatenate([head.view(np.uint8), entries.reshape(-1).view(np.uint8), start.view(np.uint8)])
    assert out.shape[0] == wind_table_bytes(K)
    return out


def unpack_table(table, K):
    """uint8 -> (x^ (K,), p (K - 1,) at the intervals' starts, slope (K - 1,), p at the last knot)"""
    raw = np.ascontiguousarray(table[:wind_table_bytes(K)])
    head = raw[:32].view(f32)
    e = raw[32:32 + 16 * (K - 1)].view(f32).reshape(K - 1, 4)
    assert int(raw[:32].view(np.int32)[4]) == K
    return np.concatenate([e[:, 0], e[-1:, 3]]), e[:, 1], e[:, 2], head[2]


# ------------------------------------------------------------------------------------------------------------------ the arithmetic

def cell_values32(u, v, hub, xf, pf, slope, p_last):
    """u, v fp32 arrays -> (speed, power) fp32: the kernel's per-cell arithmetic, every operation rounded to fp32 in its order"""
    assert u.dtype == f32 and v.dtype == f32
    K = xf.shape[0]
    with np.errstate(all="ignore"):
        uu, vv = u * u, v * v
        q = uu + vv
        s = np.sqrt(q) * f32(hub)
        assert s.dtype == f32
        live = (s >= xf[0]) & (s < xf[-1])
        sin = np.where(live, s, xf[0])
        j = np.clip(np.searchsorted(xf, sin, side="right") - 1, 0, K - 2)
        d = sin - xf[j]
        r = d * slope[j]
        val = pf[j] + r
        assert val.dtype == f32
        out = np.where(s == xf[-1], f32(p_last), f32(0))
        p = np.where(np.isnan(s), s, np.where(live, val, out)).astype(f32)
    return s, p


def thread_sums(vals):
    """vals (2, n) fp32 of one chunk in cell order -> (2, 256) float64: what each thread accumulates, in (round, column) order"""
    n = vals.shape[1]
    padded = np.zeros((2, CHUNK), np.float64)  # a thread without cells adds nothing: its accumulator stays +0
    padded[:, :n] = vals
    t = padded.reshape(2, ROUNDS, THREADS, 4).transpose(0, 2, 1, 3).reshape(2, THREADS, ROUNDS * 4)
    return seq_sum(t, 2)


def wind_power(fields, F, u_index, v_index, table, K, hub, sums, derived, scratch, planes, hw):
    CALLS.append((int(planes), int(F), int(u_index), int(v_index), int(K), int(hw), derived is not None))
    if not wind_supported(hw, K):
        return False
    assert fields.dtype == torch.float32 and fields.is_contiguous() and fields.data_ptr() % 16 == 0 and fields.numel() >= planes * F * hw
    assert 0 <= u_index < F and 0 <= v_index < F and planes >= 1
    assert table.dtype == torch.uint8 and table.data_ptr() % 16 == 0 and table.numel() >= wind_table_bytes(K)
    assert sums.dtype == torch.float64 and sums.is_contiguous() and sums.numel() >= planes * 2
    nc = chunks(hw)
    need = wind_scratch_bytes(planes, hw)
    assert need == 0 or (scratch is not None and scratch.dtype == torch.float64 and scratch.numel() * 8 >= need)
    xf, pf, slope, p_last = unpack_table(table.numpy(), K)
    x = fields.reshape(-1).numpy()[:planes * F * hw].reshape(planes, F, hw)
    out = sums.reshape(-1).numpy()
    part = np.full((planes, nc, 2), np.nan)  # every entry that is read must have been written by a workgroup
    dv = None
    if derived is not None:
        assert derived.dtype == torch.float32 and derived.is_contiguous() and derived.numel() >= planes * 2 * hw and derived.data_ptr() % 16 == 0
        dv = derived.reshape(-1).numpy()[:planes * 2 * hw].reshape(planes, 2, hw)
    for pl in range(planes):
        for c in range(nc):
            lo, hi = chunk_bounds(hw, c)
            s, p = cell_values32(x[pl, u_index, lo:hi], x[pl, v_index, lo:hi], hub, xf, pf, slope, p_last)
            if dv is not None:
                dv[pl, 0, lo:hi], dv[pl, 1, lo:hi] = s, p
            part[pl, c] = fold_workgroup(thread_sums(np.stack([s, p])), nan_if_nan)
    if nc > 1:
        scratch.reshape(-1).numpy()[:planes * nc * 2] = part.reshape(-1)
    out[:planes * 2] = (fold_parts(part, 1, nan_if_nan) if nc > 1 else part[:, 0]).reshape(-1)
    return True


def install(monkeypatch, wind_ops_module, windpower_module):
    me = sys.modules[__name__]
    del CALLS[:]
    for name in ("wind_supported", "wind_table_bytes", "wind_table", "wind_scratch_bytes", "wind_power"):
        monkeypatch.setattr(wind_ops_module, name, getattr(me, name))
    monkeypatch.setattr(windpower_module, "_on_device", lambda x: True)
