"""The case table of tests/test_gpu_conv_geometry.py (tests/conv_geometry_cases.py) proven on the CPU before a GPU sees it: the fp32
restatement (tests/emu_ops.py) run through every shape, (Cout, ldy, wrows) and dtype of the table against fp64_ref.py.

  * the restatement is inside the float64 bound at every case, and leaves the padding columns [Cout, ldy) untouched;
  * the bound is not vacuous: the largest err / bound over the table is above 1e-3 (the rule of tests/test_fp64_bounds_cpu.py);
  * the planted missing tap is rejected at every geometry -- the 1-pixel-high and the 5x7 ones included, where every pixel is a border
    pixel, and the stride-2 input gradient, which receives the centre tap on even pixels only;
  * the table reaches every kernel family the library's dispatch queries can answer (they need no device), every row dispatches to the
    family it is there for, and both orders of the gather stride-2 input gradient occur;
  * every geometry the pinned launch order of a training step holds obeys the launchers' output-grid rule."""
import json
import os
import re

import pytest
import torch

import conv_geometry_cases as C
import emu_ops as E
import fp64_ref as R

WORST = {}  # (kind, dtype) -> largest err / bound seen


def _note(kind, dt, r):
    WORST[(kind, dt)] = max(WORST.get((kind, dt), 0.0), r)


@pytest.mark.parametrize("name,ti,dt,naive", C.forward_cases(dedupe=True), ids=lambda v: str(v).replace(" ", "_"))
def test_restatement_forward_within_the_bound(name, ti, dt, naive):
    row = C.FORWARD_BY_NAME[name]
    g, o = C.forward_operands(row, ti, dt)
    npix, Cout, ldy = g["B"] * g["Hout"] * g["Wout"], g["Cout"], g["ldy"]
    pre = R.conv_sum(o["x"], o["w"], g)
    assert (pre.v[:, min(g["wrows"], Cout):] == 0).all() and (pre.e[:, min(g["wrows"], Cout):] == 0).all()  # rows >= wrows: exact zeros
    for epi in C.EPILOGUES:
        bias, kw = C.epilogue_kwargs(epi, o)
        y = torch.full((npix, ldy), 7.0, dtype=C.TD[dt])
        y2 = torch.full((npix, ldy), 3.0, dtype=C.TD[dt]) if epi == "relu pair" else None
        E.conv(o["x"], o["w"], bias, y, g, dt, y2=y2, **kw)
        what = f"{name} {C.triples(dt)[ti]} dt={dt} {epi}"
        ref = R.conv(o["x"], o["w"], g, dt, bias=bias, pre=pre, **kw)
        _note("conv", dt, R.assert_within(y[:, :Cout], ref["y"], what=what, layout=R.layout(g)))
        assert (y[:, Cout:] == 7.0).all(), what + ": padding columns written"
        if y2 is not None:
            R.assert_mask_consistent(y[:, :Cout], y2[:, :Cout], what=what + " mask")
            assert (y2[:, Cout:] == 3.0).all(), what + ": padding columns of the mask written"
        if epi == "none":
            R.assert_rejects(y[:, :Cout].double() - C.missing_tap(o, g), ref["y"], what=what + ", planted missing border tap")


@pytest.mark.parametrize("name,ci,dt", C.wgrad_cases(), ids=lambda v: str(v).replace(" ", "_"))
def test_restatement_wgrad_within_the_bound(name, ci, dt):
    row = C.WGRAD_BY_NAME[name]
    g, o = C.wgrad_operands(row, ci, dt)
    dw, db = o["dw0"].clone(), o["db0"].clone()
    E.conv_wgrad(o["x"], o["dy"], dw, g, dt, dbias=db)
    rw, rb = R.wgrad(o["x"], o["dy"], g)
    what = f"wgrad {name} {C.WGRAD_COUTS[ci]} dt={dt}"
    _note("wgrad", dt, R.assert_within(dw, R.accumulated(o["dw0"], rw.view(-1)), what=what + " dw"))
    _note("dbias", dt, R.assert_within(db, R.accumulated(o["db0"], rb), what=what + " dbias"))
    # the power check of the accumulating form: the last image's contribution missing
    if g["B"] > 1:
        lw, lb = R.wgrad(o["x"], o["dy"], g, images=(g["B"] - 1, g["B"]))
        R.assert_rejects(dw.double() - lw.v.view(-1), R.accumulated(o["dw0"], rw.view(-1)), what=what + ", planted missing image")


def test_the_bound_is_not_vacuous_over_the_table():
    if not WORST:  # selected on its own: a slice of the table
        for case in C.forward_cases(dedupe=True)[::37]:
            test_restatement_forward_within_the_bound(*case)
        for case in C.wgrad_cases()[::11]:
            test_restatement_wgrad_within_the_bound(*case)
    for kind in ("conv", "wgrad", "dbias"):
        worst = max(v for (k, _), v in WORST.items() if k == kind)
        print(f"{kind}: largest err/bound of the restatement over the table {worst:.3e}")
        assert worst > 1e-3, f"vacuous bound ({kind}): {worst:.2e}"


def test_the_table_reaches_every_route(monkeypatch):
    """c2w_conv_dispatch / c2w_conv_wgrad_dispatch answer without a device (256 compute units assumed): every row goes where it is meant
    to, every kernel family is reached, and both orders of the gather stride-2 input gradient occur"""
    from climate2weather_amd import _lib, build, ops
    build.build(verbose=False)
    families = {_lib.KERNEL_GATHER, _lib.KERNEL_PATCH_8X16, _lib.KERNEL_PATCH_16X16, _lib.KERNEL_PATCH_PAIR, _lib.KERNEL_PATCH_TS2, _lib.KERNEL_PATCH_S2}
    assert families == {C.GATHER, C.P8X16, C.P16X16, C.PAIR, C.PTS2, C.PS2}
    knobs = sorted({k for r in C.FORWARD for k, _ in r.knobs})
    seen, seen_w, orders, split = set(), set(), set(), 0
    try:
        for r in C.FORWARD:
            for k in knobs:
                monkeypatch.delenv(k, raising=False)
            for k, v in r.knobs:
                monkeypatch.setenv(k, v)
            ops.knobs_reload()
            for dt in r.dtypes():
                for ti, t in enumerate(C.triples(dt)):
                    g = r.geom(dt, *t)
                    fam = ops.conv_dispatch(g, dt)
                    assert r.wanted(dt) is None or fam == r.wanted(dt), (r.name, dt, t, fam)
                    seen.add(fam)
                    split += ops.conv_splitk_plan(g, dt)[0] > 1
                    if r.mode == C.TS2:  # (naive = 2 takes the gather kernel at every one of these rows)
                        orders.add(C.ts2_parity_order(g, 256))
        for k in knobs:
            monkeypatch.delenv(k, raising=False)
        ops.knobs_reload()
        for r in C.WGRAD:
            for dt in C.DTYPES:
                for co in C.WGRAD_COUTS:
                    fam = ops.conv_wgrad_dispatch(r.geom(dt, co[0], co[1], co[0]), dt)
                    assert fam == r.want, (r.name, dt, co, fam)
                    seen_w.add(fam)
        for name, co in C.GROUPED:
            for dt in C.DTYPES:
                g = C.WGRAD_BY_NAME[name].geom(dt, co[0], co[1], co[0])
                assert ops.conv_wgrad_grouped_supported(g, 2, dt) and ops.conv_wgrad_grouped_supported(g, C.GROUP_MAX, dt)
                assert not ops.conv_wgrad_grouped_supported(g, C.GROUP_MAX + 1, dt)
    finally:
        for k in knobs:
            monkeypatch.delenv(k, raising=False)
        ops.knobs_reload()
    assert seen == families, seen
    assert seen_w == {C.GATHER, C.P8X16, C.PAIR}, seen_w  # everything c2w_conv_wgrad_dispatch returns
    assert orders == {True, False}
    assert split > 0, "no row of the table splits K"


def test_every_pinned_launch_geometry_obeys_the_output_grid_rule():
    """the launchers refuse an output grid that is not the mode's function of the input grid: nothing a training step launches is"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "launch_order_tiny.json")
    with open(path) as f:
        lines = [line for plan in json.load(f).values() for line in plan]
    n = 0
    for line in lines:
        m = re.search(r"\{B=(\d+),Hin=(\d+),Win=(\d+),Cin=(\d+),Hout=(\d+),Wout=(\d+),Cout=(\d+),ldy=(\d+),wrows=(\d+),mode=(\d+)\}", line)
        if not m:
            continue
        B, Hin, Win, Cin, Hout, Wout, Cout, ldy, wrows, mode = map(int, m.groups())
        assert C.grid_defined(mode, Hin, Win, Hout, Wout) and Cout <= ldy, line
        n += 1
    assert n > 100
