"""The launch layer of the HIP library (csrc/launch.h): dispatch arithmetic that means "one workgroup per compute unit" follows the
device's own CU count, and the per-device dynamic-LDS opt-in lets one process launch every kernel family on a second device."""
import math

import pytest
import torch

from climate2weather_amd import _lib, ops

pytestmark = pytest.mark.gpu

BF16, F32 = ops.DTYPE_BF16, ops.DTYPE_F32
S1, K1 = ops.CONV_S1, ops.CONV_1X1
two_gpus = pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs in one process")


def geom(B, H, W, Cin, Cout, mode=S1):
    return dict(B=B, Hin=H, Win=W, Cin=Cin, Hout=H, Wout=W, Cout=Cout, ldy=Cout, wrows=Cout, mode=mode)


@pytest.mark.parametrize("B", [76, 100, 129])
def test_splitk_plan_follows_the_cu_count(B):
    """c2w_conv_splitk_plan deals a tile's K chunks to as many workgroups as keep the launch at one workgroup per CU, at most one per
    chunk and 8: an 8x16 image is one tile, Cin = 512 is eight bf16 chunks.  On 256 CUs: 3, 2 and no split.  Query only."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = geom(B, 8, 16, 512, 128)
    assert ops.conv_dispatch(g, BF16) == _lib.KERNEL_PATCH_8X16
    n = min(8, 8, cus // B)
    want = (n, n * B * 128 * 128 * 4) if n >= 2 else (1, 0)
    with torch.cuda.device(0):
        assert ops.conv_splitk_plan(g, BF16) == want, f"{cus} CUs, {B} tiles"
    if cus == 256:
        assert want[0] == {76: 3, 100: 2, 129: 1}[B]


def _rnd(shape, seed, dtype=torch.bfloat16, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


@pytest.fixture
def knob(monkeypatch):
    """set(name, value) flips a run-time knob of the library; every knob set is unset again, and the library told, afterwards"""
    names = []

    def set_(name, value):
        monkeypatch.setenv(name, value)
        names.append(name)
        ops.knobs_reload()
    yield set_
    for n in names:
        monkeypatch.delenv(n, raising=False)
    ops.knobs_reload()


def _conv(dev, g, naive=0):
    x = _rnd((g["B"] * g["Hin"] * g["Win"], g["Cin"]), 1).to(dev)
    w = _rnd((g["Cout"], 1 if g["mode"] == K1 else 9, g["Cin"]), 2, scale=1.0 / math.sqrt(9 * g["Cin"])).to(dev)
    bias = _rnd((g["Cout"],), 3, torch.float32).to(dev)
    y = torch.full((g["B"] * g["Hout"] * g["Wout"], g["Cout"]), 7.0, dtype=torch.bfloat16, device=dev)
    ops.conv(x, w, bias, y, g, BF16, naive=naive)
    return [y]


def _wgrad(dev, g, family):
    assert ops.conv_wgrad_dispatch(g, BF16) == family
    x = _rnd((g["B"] * g["Hin"] * g["Win"], g["Cin"]), 1).to(dev)
    dy = _rnd((g["B"] * g["Hout"] * g["Wout"], g["Cout"]), 2).to(dev)
    taps = 1 if g["mode"] == K1 else 9
    dw = torch.zeros(g["Cout"] * taps * g["Cin"], dtype=torch.float32, device=dev)
    need = ops.conv_wgrad_workspace_bytes(g, BF16)  # a split reduction goes through scratch in a fixed order, never through atomics
    ws = torch.empty(need // 4, dtype=torch.float32, device=dev) if need else None
    ops.conv_wgrad(x, dy, dw, g, BF16, workspace=ws)
    return [dw]


def _attention(dev):
    B, T, C = 1, 64, 32
    qkv, do = _rnd((B * T, 3 * C), 1).to(dev), _rnd((B * T, C), 2).to(dev)
    o, lse, delta, dqkv = torch.empty_like(do), torch.empty(B * T, device=dev), torch.empty(B * T, device=dev), torch.empty_like(qkv)
    ops.attention_forward(qkv, o, lse, B, T, C, BF16)
    ops.attention_backward(qkv, o, do, lse, delta, dqkv, B, T, C, BF16)
    return [o, lse, dqkv]


def _rapsd(dev):
    x, spec = _rnd((1, 128, 128), 1, torch.float32).to(dev), torch.empty((1, 64), device=dev)
    assert ops.rapsd(x, spec, 1, 128, 128)
    return [spec]


def _swd_distance(dev):
    px, py = _rnd((1, 1, 1, 16), 1, torch.float32).to(dev), _rnd((1, 1, 16), 2, torch.float32).to(dev)
    out = torch.empty((1, 1, 1), dtype=torch.float64, device=dev)
    assert ops.swd_distance(px, py, out, 1, 1, 1, 16)
    return [out]


def _conv_center(dev):
    B, H, W, Cin, wrows = 1, 8, 16, 64, 16
    assert ops.conv_center_supported(H, W, Cin, 1, BF16)
    x, w = _rnd((B * H * W, Cin), 1).to(dev), _rnd((wrows, 9, Cin), 2, scale=1.0 / math.sqrt(9 * Cin)).to(dev)
    bias, out = _rnd((wrows,), 3, torch.float32).to(dev), torch.empty((B, 1, H, W), device=dev)
    ops.conv_center(x, w, bias, out, B, H, W, Cin, wrows, 0, 1, H * W, BF16)
    return [out]


def _launch_every_opt_in_site(devices, knob):
    """One smallest-shape launch per translation unit with a dynamic-LDS opt-in on each of ``devices`` in turn, from identical inputs:
    every launch succeeds and gives the bits of the first device."""
    small, tall = geom(1, 8, 16, 64, 128), geom(1, 16, 16, 64, 128)
    onebyone = geom(128, 1, 1, 64, 128, K1)
    assert ops.conv_dispatch(small, BF16) == _lib.KERNEL_PATCH_8X16 and ops.conv_dispatch(onebyone, BF16) == _lib.KERNEL_GATHER

    def t3(dev):
        assert ops.conv_dispatch(tall, BF16) == _lib.KERNEL_PATCH_16X16
        return _conv(dev, tall)
    # (name, knob to set first, launch)
    cases = [("conv_patch: 8x16-tile conv", None, lambda d: _conv(d, small)),
             ("conv_igemm: gather conv", None, lambda d: _conv(d, small, naive=2)),
             ("wgrad_patch: halo-patch weight gradient", None, lambda d: _wgrad(d, small, _lib.KERNEL_PATCH_8X16)),
             ("wgrad: gather weight gradient", None, lambda d: _wgrad(d, onebyone, _lib.KERNEL_GATHER)),
             ("attention_mfma: matrix-core attention", None, _attention),
             ("spectrum: rapsd 128x128", None, _rapsd),
             ("swd: distance", None, _swd_distance),
             ("conv_center", None, _conv_center),
             ("conv_patch3: 16x16-tile conv", ("C2W_CONV_T3", "16"), t3),
             ("attention: VALU attention", ("C2W_ATTN_VALU", "1"), _attention)]
    for name, kn, run in cases:
        if kn is not None:
            knob(*kn)
        outs = []
        for d in devices:
            with torch.cuda.device(d):
                outs.append([t.cpu() for t in run(torch.device("cuda", d))])  # .cpu() synchronises: a refused launch raises here at the latest
        for a, b in zip(*outs):
            assert torch.isfinite(a.double()).all(), name
            assert torch.equal(a, b), f"{name}: cuda:{devices[1]} differs from cuda:{devices[0]}"


@two_gpus
def test_every_opt_in_site_launches_on_a_second_device(knob):
    """The per-device opt-in: in one process, first cuda:0 and then cuda:1."""
    _launch_every_opt_in_site((0, 1), knob)
