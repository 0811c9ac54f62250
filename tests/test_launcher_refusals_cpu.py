"""What the launchers of the metric units and of evaluation.hip refuse, and with which code, pinned without a GPU.

Every entry point that takes pointers has one base call, which would be valid and is NEVER made, and rows that each break it in one way:
a required pointer null, a pointer of each alignment class moved off its alignment, a grid over what a launch takes (where integer
arguments can reach that), an unsupported shape.  Every row returns a negative C2W_ERR_* code, that is before any launch or memset: the
device addresses are made-up multiples of 4096 and nothing dereferences them.  Pointers the library reads ON THE HOST (the quantile
levels, the FSS radii, the wind curve) are real arrays.  The expected codes were recorded from the launchers as they were when the
checks were still written out in every entry point; c2w_aligned and c2w_grid_fits (csrc/launch.h) must not change one of them, nor
the order unsupported -> bad argument -> bad shape.  Skipped where a GPU is visible: no row may ever be in a position to launch.

c2w_conv_forward and the weight-gradient entry points take their geometry in a C2wConvArgs block (ConvBlock below: a change that names
one of its fields lands in the block).  Their rows pin the geometry no definition covers (include/c2w_hip.h next to C2wConvArgs): more
channels than a row of y holds, and an output grid that is not the mode's function of the input grid -- C2W_ERR_BAD_SHAPE, before any
launch."""
import ctypes

import pytest

from climate2weather_amd import _lib, build

BAD_ARG, BAD_SHAPE, UNSUPPORTED = -1, -2, -3
BIG = 1 << 62  # scratch bytes nobody runs short of
Q2 = (ctypes.c_double * 2)(0.25, 0.75)
RADII = (ctypes.c_int * 2)(1, 2)
XS, PS, TABLE = (ctypes.c_double * 2)(1.0, 2.0), (ctypes.c_double * 2)(0.0, 1.0), ctypes.create_string_buffer(4096)


class Dev:
    """A made-up device address: argument number i of a call is 4096 (16 + i)."""


DEV = Dev()


class ConvBlock:
    """A C2wConvArgs passed by reference: the fields given (DEV: a made-up device address), every other one zero."""

    def __init__(self, **fields):
        self.fields = fields

    def build(self, change):
        f = dict(self.fields, **{k: v for k, v in change.items() if k in self.fields})
        block = _lib.ConvArgs()
        for j, (k, v) in enumerate(f.items()):
            setattr(block, k, 4096 * (64 + j) if v is DEV else v)
        return block


X1, S1, S2, UP, TS2 = _lib.CONV_1X1, _lib.CONV_S1, _lib.CONV_S2, _lib.CONV_UP, _lib.CONV_TS2
CONV = dict(x=DEV, w=DEV, y=DEV, B=2, Hin=8, Win=8, Cin=64, Hout=8, Wout=8, Cout=64, ldy=64, wrows=64, mode=S1)  # bf16: 3x3 stride 1 on 8x8

# name -> the base call, in the order of the C signature (DEV: a device pointer)
BASE = {
    "c2w_conv_forward": dict(args=ConvBlock(**CONV), dtype=_lib.DTYPE_BF16, naive=0, stream=None),
    "c2w_conv_wgrad": dict(args=ConvBlock(**CONV), dw=DEV, dbias=DEV, workspace=None, workspace_bytes=0, dtype=_lib.DTYPE_BF16, stream=None),
    "c2w_conv_wgrad_dispatch": dict(args=ConvBlock(**CONV), dtype=_lib.DTYPE_BF16),
    "c2w_rapsd": dict(x=DEV, spec=DEV, n_fields=4, H=8, W=8, stream=None),
    "c2w_ssim": dict(x=DEV, y=DEV, data_range=DEV, out=DEV, n_pairs=4, n_truth=2, H=16, W=16, win=7, stream=None),
    "c2w_swd_project": dict(x=DEV, theta=DEV, shift=DEV, scale=DEV, proj=DEV, n_rep=2, T=2, F=2, d=64, P=4, stream=None),
    "c2w_swd_project_pair": dict(x=DEV, y=DEV, theta=DEV, shift=DEV, scale=DEV, proj_x=DEV, proj_y=DEV, n_rep=2, T=2, F=2, d=64, P=4, stream=None),
    "c2w_swd_distance": dict(proj_x=DEV, proj_y=DEV, out=DEV, n_rep=2, F=2, P=4, T=8, stream=None),
    "c2w_kde_partial": dict(x=DEV, y=DEV, offsets=DEV, pivot=DEV, h=DEV, scratch=DEV, scratch_bytes=BIG, n_rep=2, T=2, F=2, hw=16, N=8, stream=None),
    "c2w_kde_fold": dict(scratch=DEV, h=DEV, dens=DEV, D=4, n=32, N=8, stream=None),
    "c2w_kde_eval": dict(x=DEV, y=DEV, offsets=DEV, pivot=DEV, h=DEV, scratch=DEV, scratch_bytes=BIG, dens=DEV, n_rep=2, T=2, F=2, hw=16, N=8,
                         stream=None),
    "c2w_pit_counts": dict(x=DEV, y=DEV, counts=DEV, M=4, T=2, F=2, hw=16, stream=None),
    "c2w_quantiles": dict(x=DEV, y=DEV, q=Q2, Q=2, skipna=0, scratch=DEV, scratch_bytes=BIG, out=DEV, stats=DEV, n_valid=DEV, n_rep=2, T=2, F=2,
                          hw=16, stream=None),
    "c2w_crps_terms": dict(x=DEV, y=DEV, sums=DEV, cells=DEV, scratch=DEV, scratch_bytes=BIG, M=4, T=2, F=2, hw=16, stream=None),
    "c2w_wind_table": dict(xs=XS, ps=PS, K=2, table_host=TABLE),
    "c2w_wind_power": dict(fields=DEV, F=2, u_index=0, v_index=1, table=DEV, K=2, hub_factor=1.0, sums=DEV, derived=DEV, scratch=DEV,
                           scratch_bytes=BIG, planes=4, hw=16, stream=None),
    "c2w_escore_pairs": dict(x=DEV, y=DEV, d2=DEV, scratch=DEV, scratch_bytes=BIG, M=4, planes=4, hw=16, stream=None),
    "c2w_vario_terms": dict(x=DEV, y=DEV, V=DEV, scratch=DEV, scratch_bytes=BIG, M=4, planes=4, H=8, W=8, R=1, order2=2, stream=None),
    "c2w_tincr_terms": dict(x=DEV, y=DEV, S=DEV, scratch=DEV, scratch_bytes=BIG, n_rep=2, T=4, F=2, hw=16, L=2, stream=None),
    "c2w_qmap_nodes": dict(x=DEV, tidx=DEV, goff=DEV, levels=DEV, q=DEV, n_valid=DEV, scratch=DEV, scratch_bytes=BIG, n_rep=2, T=8, F=2, hw=16, Tu=8,
                           G=2, K=4, max_len=4, skipna=0, c0=0, c1=16, stream=None),
    "c2w_qmap_apply": dict(x=DEV, out=DEV, xq=DEV, yq=DEV, tidx=DEV, goff=DEV, n_rep=2, T=8, F=2, hw=16, Tu=8, G=2, K=4, max_len=4, stream=None),
    "c2w_event_counts": dict(x=DEV, y=DEV, thr=DEV, dir=DEV, counts=DEV, invalid=DEV, M=4, T=2, F=2, hw=16, K=2, stream=None),
    "c2w_fss_sums": dict(x=DEV, y=DEV, thr=DEV, dir=DEV, sums=DEV, radii=RADII, M=4, T=2, F=2, H=8, W=8, K=2, S=2, stream=None),
    "c2w_spell_update": dict(x=DEV, y=DEV, thr=DEV, dir=DEV, state=DEV, hist=DEV, onsets=DEV, invalid=DEV, M=2, T=4, F=2, hw=16, K=2, max_duration=8,
                             period=4, t0=0, stream=None),
    "c2w_sq_err_levels": dict(y=DEV, eps=DEV, t=DEV, table=DEV, count=DEV, per_image=DEV, B=2, C=4, HW=16, ldc=4, K=4, scratch=DEV,
                              scratch_bytes=BIG, dtype=_lib.DTYPE_F32, stream=None),
    "c2w_sq_err_levels_noise": dict(y=DEV, seed=7, t=DEV, table=DEV, count=DEV, per_image=DEV, B=2, C=4, HW=16, ldc=4, K=4, scratch=DEV,
                                    scratch_bytes=BIG, dtype=_lib.DTYPE_F32, stream=None),
}


def null(*names):
    return [("%s null" % n, {n: None}) for n in names]


def off(by, *names):  # a pointer of the 16-, 8- (by 4 bytes) or 4-byte class (by 2) moved off its alignment
    return [("%s off by %d" % (n, by), {n: by}) for n in names]


M20 = 1 << 20  # T = F = 2^20: 2^40 planes, over any grid while a plane is one chunk (hw = 16 needs no scratch)

# an output grid that is not the mode's function of the input grid (8x8 in): 1x1 and stride 1 keep it, stride 2 halves it (rounding either
# way), the up-conv doubles it, the stride-2 input gradient gives 2 n - 1 or 2 n
GRID = [("stride 1, a row more", dict(Hout=9)), ("stride 1, a column less", dict(Wout=7)), ("1x1, a column less", dict(mode=X1, Wout=7)),
        ("stride 2, Hout under Hin / 2", dict(mode=S2, Hout=3, Wout=4)), ("stride 2, Wout over (Win + 1) / 2", dict(mode=S2, Hout=4, Wout=5)),
        ("up-conv, Hout over 2 Hin", dict(mode=UP, Hout=17, Wout=16)), ("up-conv, Wout under 2 Win", dict(mode=UP, Hout=16, Wout=15))]
GRID_TS2 = [("stride-2 input gradient, Hout over 2 Hin", dict(mode=TS2, Hout=17, Wout=16)),
            ("stride-2 input gradient, Wout under 2 Win - 1", dict(mode=TS2, Hout=16, Wout=14))]

# (entry point, [(what is broken, {argument: None | a byte offset for a device pointer | a value})], the codes in that order)
TABLE_ROWS = [
    ("c2w_conv_forward", null("x", "w", "y") + [("Cout over ldy", dict(ldy=56)), ("Cout over ldy, 1x1", dict(mode=X1, ldy=8))] + GRID + GRID_TS2,
     [BAD_ARG] * 3 + [BAD_SHAPE] * (2 + len(GRID) + len(GRID_TS2))),
    ("c2w_conv_wgrad", [("Cout over ldy", dict(ldy=56))] + GRID + [("the stride-2 input gradient has no weight gradient", dict(mode=TS2, Hout=16, Wout=16))],
     [BAD_SHAPE] * (1 + len(GRID)) + [BAD_ARG]),
    ("c2w_conv_wgrad_dispatch", [("Cout over ldy", dict(ldy=56))] + GRID, [BAD_SHAPE] * (1 + len(GRID))),
    ("c2w_rapsd", null("x", "spec") + off(4, "x") + [("grid", dict(n_fields=1 << 35)), ("unsupported", dict(H=12, W=12))],
     [BAD_ARG, BAD_ARG, BAD_ARG, BAD_SHAPE, UNSUPPORTED]),
    ("c2w_ssim", null("x", "y", "data_range", "out") + off(4, "x", "y", "out") + [("grid", dict(n_pairs=1 << 40)), ("unsupported", dict(win=9))],
     [BAD_ARG] * 7 + [BAD_SHAPE, UNSUPPORTED]),
    ("c2w_swd_project", null("x", "theta", "shift", "scale", "proj") + off(4, "x", "theta") + off(2, "proj")
     + [("grid", dict(n_rep=1 << 40)), ("unsupported", dict(d=65))], [BAD_ARG] * 8 + [BAD_SHAPE, UNSUPPORTED]),
    ("c2w_swd_project_pair", null("x", "theta", "shift", "scale", "proj_x", "proj_y") + off(4, "x", "y", "theta") + off(2, "proj_x", "proj_y")
     + [("grid", dict(n_rep=1 << 40)), ("unsupported", dict(P=0))], [BAD_ARG] * 11 + [BAD_SHAPE, UNSUPPORTED]),
    ("c2w_swd_distance", null("proj_x", "proj_y", "out") + off(4, "out") + [("grid", dict(n_rep=1 << 40)), ("unsupported", dict(T=0))],
     [BAD_ARG] * 4 + [BAD_SHAPE, UNSUPPORTED]),
    ("c2w_kde_partial", null("x", "offsets", "pivot", "h", "scratch") + off(4, "x", "y", "h", "scratch") + off(2, "offsets", "pivot")
     + [("grid", dict(n_rep=1 << 40)), ("unsupported", dict(hw=6))], [BAD_ARG] * 11 + [BAD_SHAPE, UNSUPPORTED]),
    ("c2w_kde_fold", null("scratch", "h", "dens") + off(4, "scratch", "h", "dens") + [("grid", dict(D=1 << 40)), ("unsupported", dict(N=0))],
     [BAD_ARG] * 6 + [BAD_SHAPE, UNSUPPORTED]),
    ("c2w_kde_eval", null("dens", "x", "h") + off(4, "dens", "x") + [("grid", dict(n_rep=1 << 40)), ("unsupported", dict(hw=6))],
     [BAD_ARG] * 5 + [BAD_SHAPE, UNSUPPORTED]),
    ("c2w_pit_counts", null("x", "y", "counts") + off(4, "x", "y", "counts") + [("unsupported", dict(M=0))], [BAD_ARG] * 6 + [UNSUPPORTED]),
    ("c2w_quantiles", null("x", "q", "scratch", "out", "stats", "n_valid") + off(4, "x", "y", "scratch", "out", "n_valid") + off(2, "stats")
     + [("level outside [0, 1]", dict(q=(ctypes.c_double * 2)(0.5, 1.5))), ("grid", dict(n_rep=1 << 40)), ("unsupported", dict(Q=0))],
     [BAD_ARG] * 13 + [BAD_SHAPE, UNSUPPORTED]),
    ("c2w_crps_terms", null("x", "y", "sums") + off(4, "x", "y", "cells", "sums", "scratch")
     + [("grid", dict(T=M20, F=M20)), ("unsupported", dict(M=0))], [BAD_ARG] * 8 + [BAD_SHAPE, UNSUPPORTED]),
    ("c2w_wind_table", null("xs", "ps", "table_host") + [("a curve of one knot", dict(K=1))], [BAD_ARG] * 4),  # host code: one code
    ("c2w_wind_power", null("fields", "table", "sums") + off(4, "fields", "table", "derived", "sums", "scratch")
     + [("grid", dict(planes=1 << 40)), ("unsupported", dict(K=1))], [BAD_ARG] * 8 + [BAD_SHAPE, UNSUPPORTED]),
    ("c2w_escore_pairs", null("x", "y", "d2") + off(4, "x", "y", "d2", "scratch") + [("grid", dict(planes=1 << 40)), ("unsupported", dict(hw=6))],
     [BAD_ARG] * 7 + [BAD_SHAPE, UNSUPPORTED]),
    ("c2w_vario_terms", null("x", "y", "V") + off(2, "x", "y") + off(4, "V", "scratch") + [("grid", dict(planes=1 << 40)), ("unsupported", dict(order2=3))],
     [BAD_ARG] * 7 + [BAD_SHAPE, UNSUPPORTED]),
    ("c2w_tincr_terms", null("x", "S") + off(4, "x", "y", "S", "scratch") + [("grid", dict(T=M20, F=M20)), ("unsupported", dict(L=0))],
     [BAD_ARG] * 6 + [BAD_SHAPE, UNSUPPORTED]),
    ("c2w_qmap_nodes", null("x", "tidx", "goff", "levels", "q", "n_valid", "scratch") + off(2, "x", "scratch") + off(4, "q", "n_valid", "levels")
     + [("grid", dict(n_rep=65535, F=1, hw=M20, c1=M20, G=64)), ("rows over 65535", dict(n_rep=65536, F=1)), ("unsupported", dict(K=1))],
     [BAD_ARG] * 12 + [BAD_SHAPE, BAD_SHAPE, UNSUPPORTED]),
    ("c2w_qmap_apply", null("x", "out", "xq", "yq", "tidx", "goff") + off(4, "x", "out", "xq", "yq")
     + [("grid dimension over 65535", dict(G=65536, F=1)), ("unsupported", dict(K=1))], [BAD_ARG] * 10 + [BAD_SHAPE, UNSUPPORTED]),
    ("c2w_event_counts", null("x", "y", "thr", "dir", "counts", "invalid") + off(4, "x", "y", "counts", "invalid") + off(2, "thr", "dir")
     + [("grid", dict(T=M20, F=M20)), ("unsupported", dict(K=0))], [BAD_ARG] * 12 + [BAD_SHAPE, UNSUPPORTED]),
    ("c2w_fss_sums", null("x", "y", "thr", "dir", "sums") + off(4, "x", "y", "sums") + off(2, "thr", "dir")
     + [("grid", dict(T=M20, F=M20)), ("radii null", dict(radii=None)), ("unsupported", dict(W=6))], [BAD_ARG] * 10 + [BAD_SHAPE, UNSUPPORTED, UNSUPPORTED]),
    ("c2w_spell_update", null("x", "thr", "dir", "state", "hist", "onsets", "invalid") + off(4, "x", "y", "state", "hist", "onsets", "invalid")
     + off(2, "thr", "dir") + [("grid", dict(M=M20, F=M20)), ("T over the limit", dict(T=1 << 30)), ("unsupported", dict(period=-1))],
     [BAD_ARG] * 15 + [BAD_SHAPE, BAD_SHAPE, UNSUPPORTED]),
    ("c2w_sq_err_levels", null("y", "eps", "t", "table", "count", "scratch") + off(4, "y")
     + [("dtype", dict(dtype=9)), ("scratch short", dict(scratch_bytes=8)), ("shape", dict(ldc=3))], [BAD_ARG] * 9 + [BAD_SHAPE]),
    ("c2w_sq_err_levels_noise", null("y", "t", "table", "count", "scratch") + off(4, "y") + [("shape", dict(C=0)), ("unsupported", dict(HW=18))],
     [BAD_ARG] * 6 + [BAD_SHAPE, UNSUPPORTED]),
]


def arguments(name, change):
    """The base call of `name` with `change` applied; never the base call itself."""
    assert change, name
    out = []
    for i, (arg, value) in enumerate(BASE[name].items()):
        address = 4096 * (16 + i)
        if isinstance(value, ConvBlock):
            value = ctypes.byref(value.build(change))
        elif arg in change:
            c = change[arg]
            value = address + c if value is DEV and isinstance(c, int) else c
        elif value is DEV:
            value = address
        out.append(value)
    blocks = [f for v in BASE[name].values() if isinstance(v, ConvBlock) for f in v.fields]
    assert set(change) <= set(BASE[name]) | set(blocks), (name, change)
    return out


def rows():
    for name, cases, codes in TABLE_ROWS:
        assert len(cases) == len(codes), name
        for (what, change), code in zip(cases, codes):
            yield name, what, change, code


def test_the_table_covers_every_pointer_taking_launcher_and_holds_no_valid_row():
    assert {name for name, *_ in TABLE_ROWS} == set(BASE) and len(TABLE_ROWS) == len(BASE)
    for name, what, change, code in rows():
        assert code < 0 and change, (name, what)
        assert len(arguments(name, change)) == len(_lib._PROTOS[name]), name


def test_the_launchers_refuse_what_they_refused():
    import torch
    if torch.cuda.is_available():
        pytest.skip("made-up device addresses: only where nothing can launch")
    build.build(verbose=False)
    lib = _lib.load()
    wrong = []
    for name, what, change, code in rows():
        rc = getattr(lib, name)(*arguments(name, change))
        if rc != code:
            wrong.append((name, what, rc, code))
    assert not wrong, wrong
