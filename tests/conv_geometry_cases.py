"""Shared case table of the conv / weight-gradient geometry tests (CPU tier: tests/test_conv_geometry_cpu.py on the restatement; GPU
tier: tests/test_gpu_conv_geometry.py on the kernels).  An explicit table, seeded per case -- nothing is drawn.  The reference and the
error model are fp64_ref.py's; nothing here calls climate2weather_amd.ops or tests/emu_ops.py.

The rows sit where the launchers change route (conv_igemm.hip::c2w_conv_forward, wgrad.hip::c2w_conv_wgrad): Hout % 8, Wout % 16,
Wout == 8, odd B, (Hout | Wout) & 1, npix / 4 % BM of the parity-class stride-2 input gradient, Cout <= 80, and npix one either side of a
128- or 256-pixel tile.  Every forward row runs with every (Cout, ldy, wrows) of `triples`, every weight-gradient row with every
(Cout, ldy) of `wgrad_couts`."""
import math

import torch

import fp64_ref as R

F32, BF16, F16 = 0, 1, 2  # the library's dtype codes
DTYPES = (F32, BF16, F16)
TD = R.STORAGE
CK = {F32: 32, BF16: 64, F16: 64}   # channels per 128-byte K chunk
VEC = {F32: 4, BF16: 8, F16: 8}     # elements per 16-byte store: Cout and ldy are multiples of it in the forward launcher
X1, S1, S2, UP, TS2 = R.CONV_1X1, R.CONV_S1, R.CONV_S2, R.CONV_UP, R.CONV_TS2
GATHER, P8X16, P16X16, PAIR, PTS2, PS2 = 0, 1, 2, 3, 4, 5  # c2w_conv_dispatch's answers (include/c2w_hip.h)
ARENA_OFFSET = 272  # bytes from the allocation to every operand: a multiple of 16 (what the header asks for), not of 128 or 256

EPILOGUES = ("none", "bias+silu", "bias+res", "dsilu*mul+res", "relu pair")


def out_hw(mode, Hin, Win):
    """the even-sized rule; rows whose output is odd-sized name it themselves"""
    if mode == S2:
        return (Hin + 1) // 2, (Win + 1) // 2
    if mode in (UP, TS2):
        return 2 * Hin, 2 * Win
    return Hin, Win


def grid_defined(mode, Hin, Win, Hout, Wout):
    """the launchers' rule (include/c2w_hip.h next to C2wConvArgs), restated"""
    def ok(i, o):
        return {X1: o == i, S1: o == i, S2: o in ((i + 1) // 2, i // 2), UP: o == 2 * i, TS2: o in (2 * i - 1, 2 * i)}[mode]
    return ok(Hin, Hout) and ok(Win, Wout)


class Row:
    def __init__(self, name, mode, B, Hin, Win, out=None, chunks=1, knobs=(), only16=False, want=None, want32=None):
        self.name, self.mode, self.B, self.Hin, self.Win, self.chunks, self.knobs, self.only16 = name, mode, B, Hin, Win, chunks, tuple(knobs), only16
        self.Hout, self.Wout = out or out_hw(mode, Hin, Win)
        self.want = want            # c2w_conv_dispatch's answer the row is there for (None: whatever the rule gives; gather-sized rows say GATHER)
        self.want32 = want if want32 is None else want32
        assert grid_defined(mode, Hin, Win, self.Hout, self.Wout), name

    def dtypes(self):
        return (BF16, F16) if self.only16 else DTYPES

    def wanted(self, dt):
        return self.want32 if dt == F32 else self.want

    def geom(self, dt, Cout, ldy, wrows):
        return dict(B=self.B, Hin=self.Hin, Win=self.Win, Cin=self.chunks * CK[dt], Hout=self.Hout, Wout=self.Wout, Cout=Cout, ldy=ldy, wrows=wrows,
                    mode=self.mode)


def _edges(mode):
    return [Row(f"1x1 1x{n}", mode, 1, 1, n, want=GATHER) for n in (127, 128, 129, 255, 256, 257)]


T3_16, T3_0, NO_H8 = (("C2W_CONV_T3", "16"),), (("C2W_CONV_T3", "0"),), (("C2W_NO_HALF8", "1"),)

FORWARD = [
    # ---- the gather kernel at odd sizes
    Row("s1 3x5x7", S1, 3, 5, 7, want=GATHER),
    Row("s2 2x7x9", S2, 2, 7, 9, want=GATHER),                       # -> 4x5
    Row("s2 2x6x10", S2, 2, 6, 10, want=GATHER),                     # -> 3x5
    Row("up 1x3x5", UP, 1, 3, 5, want=GATHER),                       # -> 6x10
    Row("ts2 2x3x5 even", TS2, 2, 3, 5, want=GATHER),                # -> 6x10, 30 pixels per class: identity order
    Row("ts2 128x3x5 even", TS2, 128, 3, 5, want=GATHER),            # -> 6x10, 1920 = 15 x 128 pixels per class: parity-class tiles
    Row("ts2 2x3x5 odd", TS2, 2, 3, 5, out=(5, 9), want=GATHER),     # odd output: identity order
    Row("1x1 5x1x1", X1, 5, 1, 1, want=GATHER),
    # ---- pixel-tile edges of the gather kernel (128- and 256-pixel tiles; 64-pixel K tiles of the weight gradient)
    *_edges(X1),
    # ---- the 8x16 halo patch and one step off it
    Row("s1 1x8x16", S1, 1, 8, 16, want=P8X16),
    Row("s1 3x16x32 odd chunks", S1, 3, 16, 32, chunks=3, want=P8X16),  # the table's split-K case: 12 tiles, 3 chunks
    Row("s1 2x8x24", S1, 2, 8, 24, want=GATHER),
    Row("s1 2x12x16", S1, 2, 12, 16, want=GATHER),
    Row("s1 2x4x16", S1, 2, 4, 16, want=GATHER),
    # ---- two images per tile
    Row("s1 1x8x8", S1, 1, 8, 8, want=PAIR),
    Row("s1 2x8x8", S1, 2, 8, 8, want=PAIR),
    Row("s1 3x8x8", S1, 3, 8, 8, want=PAIR),
    Row("s1 3x16x8", S1, 3, 16, 8, want=PAIR),
    # ---- the up-conv patch and off it
    Row("up 2x4x8", UP, 2, 4, 8, want=P8X16),
    Row("up 2x4x4", UP, 2, 4, 4, want=GATHER),
    # ---- the stride-2 input gradient: the patch kernel under both C2W_TS2_PAIRS, the gather kernel's parity classes
    Row("ts2 2x8x16 pairs", TS2, 2, 8, 16, knobs=(("C2W_TS2_PAIRS", "1"),), want=PTS2),
    Row("ts2 2x8x16 no pairs", TS2, 2, 8, 16, knobs=(("C2W_TS2_PAIRS", "0"),), want=PTS2),
    Row("ts2 4x8x8", TS2, 4, 8, 8, want=GATHER),
    # ---- the stride-2 forward on parity planes (16-bit), and the same shapes on the gather kernel
    *[Row(f"s2 {B}x{H}x{W} patch={k}", S2, B, H, W, knobs=(("C2W_CONV_S2_PATCH", k),), want=PS2 if k == "2" else GATHER, want32=GATHER)
      for k in ("2", "0") for B, H, W in ((2, 16, 32), (1, 16, 16), (3, 16, 16))],
    # ---- the 16x16-tile kernel (16-bit) and the 8x16 kernel on the same shapes
    *[Row(f"{n} t3={k[0][1]}", m, B, H, W, knobs=k, only16=True, want=P16X16 if k is T3_16 else P8X16)
      for k in (T3_16, T3_0) for n, m, B, H, W in (("s1 1x16x16", S1, 1, 16, 16), ("s1 2x16x32", S1, 2, 16, 32), ("up 1x8x8", UP, 1, 8, 8))],
    # ---- the 8x16 cases without the eight-wave form
    Row("s1 1x8x16 no half8", S1, 1, 8, 16, knobs=NO_H8, want=P8X16),
    Row("s1 3x16x32 odd chunks no half8", S1, 3, 16, 32, chunks=3, knobs=NO_H8, want=P8X16),
    Row("up 2x4x8 no half8", UP, 2, 4, 8, knobs=NO_H8, want=P8X16),
]
FORWARD_BY_NAME = {r.name: r for r in FORWARD}
assert len(FORWARD_BY_NAME) == len(FORWARD)


def triples(dt):
    """(Cout, ldy, wrows) of every forward row"""
    v = VEC[dt]
    return [(v, v, v), (v, 3 * v, v), (72, 80, 71), (128, 128, 128), (136, 256, 130), (200, 200, 1)]


def _shape(r):
    return (r.mode, r.B, r.Hin, r.Win, r.Hout, r.Wout, r.chunks)


def forward_cases(dedupe=False):
    """(row name, triple index, dtype, naive).  A knob row runs under its knobs on the product route (naive = 0) only: naive 1 and 2
    read no knob, so they run once per (shape, triple, dtype) with no knob set -- on the knob-free row of the shape where the table has
    one, else on the first knob row of it.  dedupe: one per (shape, triple, dtype), for the restatement, which has one route."""
    seen, out = set(), []
    free = {(_shape(r), dt) for r in FORWARD if not r.knobs for dt in r.dtypes()}
    for r in FORWARD:
        for dt in r.dtypes():
            first = (_shape(r), dt) not in seen
            seen.add((_shape(r), dt))
            for ti in range(6):
                if dedupe:
                    if first:
                        out.append((r.name, ti, dt, 0))
                    continue
                out.append((r.name, ti, dt, 0))
                if not r.knobs or (first and (_shape(r), dt) not in free):
                    out += [(r.name, ti, dt, 1), (r.name, ti, dt, 2)]
    return out


WGRAD = [
    Row("s1 3x5x7", S1, 3, 5, 7, want=GATHER),
    Row("s2 2x7x9", S2, 2, 7, 9, want=GATHER),
    Row("s2 2x6x10", S2, 2, 6, 10, want=GATHER),
    Row("up 1x3x5", UP, 1, 3, 5, want=GATHER),
    Row("1x1 5x1x1", X1, 5, 1, 1, want=GATHER),
    *_edges(X1),
    Row("s1 1x8x16", S1, 1, 8, 16, want=P8X16),
    Row("s1 1x8x8", S1, 1, 8, 8, want=PAIR),
    Row("s1 2x8x8", S1, 2, 8, 8, want=PAIR),
    Row("s1 3x8x8", S1, 3, 8, 8, want=PAIR),
    Row("s1 3x16x8", S1, 3, 16, 8, want=GATHER),  # the forward pairs it; the weight gradient's pair form is 8x8 only
    Row("up 2x4x8", UP, 2, 4, 8, want=P8X16),
]
WGRAD_BY_NAME = {r.name: r for r in WGRAD}
WGRAD_COUTS = [(128, 128), (80, 80), (88, 88), (71, 72), (1, 8), (136, 256)]  # (Cout, ldy): the narrow form (16-bit, <= 80) and one off it
GROUPED = [("s1 1x8x16", (128, 128)), ("1x1 1x129", (128, 128))]  # one patch and one 1x1 geometry, at n = 2 and n = GROUP_MAX
GROUP_MAX = 16  # WP_MAX_ITEMS / WG_MAX_ITEMS (wgrad_patch.hip, wgrad.hip)


def wgrad_cases():
    return [(r.name, ci, dt) for r in WGRAD for dt in DTYPES for ci in range(len(WGRAD_COUTS))]


def ts2_parity_order(g, cus):
    """does the gather kernel form parity-class tiles for this stride-2 input gradient (conv_igemm.hip: `par`), restated: even output
    and a quarter of the pixels a multiple of the pixel tile -- 128 pixels while 256-pixel tiles would leave CUs idle, else 256"""
    npix = g["B"] * g["Hout"] * g["Wout"]
    nN = -(-g["Cout"] // 128)
    BM = 128 if -(-npix // 256) * nN < cus else 256
    return (g["Hout"] | g["Wout"]) & 1 == 0 and (npix // 4) % BM == 0


def _seed(*key):
    s = 0
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % (1 << 31)
    return s


def _randn(shape, T, gen, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(T)


def forward_operands(row, ti, dt):
    """seeded CPU operands of a forward case: g and x, w, bias, res, mul -- res / mul with NaN in their padding columns [Cout, ldy)"""
    Cout, ldy, wrows = triples(dt)[ti]
    g = row.geom(dt, Cout, ldy, wrows)
    gen = torch.Generator().manual_seed(_seed("fwd", row.mode, row.B, row.Hin, row.Win, row.Hout, row.Wout, row.chunks, ti, dt))
    taps = 1 if row.mode == X1 else 9
    T = TD[dt]
    npix = row.B * row.Hout * row.Wout
    o = dict(x=_randn((row.B * row.Hin * row.Win, g["Cin"]), T, gen), w=_randn((wrows, taps, g["Cin"]), T, gen, 1.0 / math.sqrt(taps * g["Cin"])),
             bias=_randn((wrows,), torch.float32, gen), res=_randn((npix, ldy), T, gen), mul=_randn((npix, ldy), T, gen))
    o["res"][:, Cout:] = float("nan")
    o["mul"][:, Cout:] = float("nan")
    return g, o


def epilogue_kwargs(name, o):
    """(bias, kwargs of ops.conv / emu_ops.conv / fp64_ref.conv) of one of EPILOGUES; the pair's y2 is the caller's"""
    return {"none": (None, {}), "bias+silu": (o["bias"], dict(act=R.ACT_SILU)), "bias+res": (o["bias"], dict(res=o["res"])),
            "dsilu*mul+res": (None, dict(mul=o["mul"], mulmode=R.MUL_DSILU, res=o["res"])), "relu pair": (o["bias"], dict(act=R.ACT_RELU_PAIR))}[name]


def missing_tap(o, g):
    """the planted defect: the centre tap (the only one of a 1x1) of input channel 0 missing at the border pixels of image 0"""
    return R.conv_term(o["x"], o["w"], g, 0, slice(0, 1), None if g["mode"] == X1 else 4, R.border_mask(g["Hout"], g["Wout"]))


def wgrad_operands(row, ci, dt, item=0):
    """seeded CPU operands of a weight-gradient case: g and x, dy (NaN in its padding columns), the non-zero fp32 starting content of dw and dbias"""
    Cout, ldy = WGRAD_COUTS[ci] if isinstance(ci, int) else ci
    g = row.geom(dt, Cout, ldy, Cout)
    gen = torch.Generator().manual_seed(_seed("wgrad", row.mode, row.B, row.Hin, row.Win, ci, dt, item))
    taps = 1 if row.mode == X1 else 9
    T = TD[dt]
    npix = row.B * row.Hout * row.Wout
    o = dict(x=_randn((row.B * row.Hin * row.Win, g["Cin"]), T, gen), dy=_randn((npix, ldy), T, gen),
             dw0=_randn((Cout * taps * g["Cin"],), torch.float32, gen), db0=_randn((Cout,), torch.float32, gen))
    o["dy"][:, Cout:] = float("nan")
    return g, o
