"""The conv and weight-gradient launchers held to float64 over the geometry they accept, with every operand guarded.

The table is tests/conv_geometry_cases.py (explicit and seeded; proven against the restatement by tests/test_conv_geometry_cpu.py).  The
only reference here is fp64_ref.py and the only bound its error model: no kernel is compared with another kernel, tests/emu_ops.py is
not imported, and no tolerance is introduced.

Arenas.  Every operand -- x, w, bias, res, mul, y, y2, dy, dw, dbias, the workspaces, every item of a grouped launch -- is a view that
starts ARENA_OFFSET = 272 bytes into a larger allocation and is followed by at least its own size again: 16-byte aligned, which is all
include/c2w_hip.h asks for, and neither 128- nor 256-byte aligned.  Around an input the allocation holds NaN, so a buffer descriptor
that is an image, a weight row or a bias element too long (the kernels take every zero they need from the descriptor's range check:
halos, the missing partner image of an odd batch, weight rows >= wrows, the bias tail) turns live outputs into NaN; so do the padding
columns [Cout, ldy) of res, mul and dy.  Around an output and around a workspace it holds a fill that must be bit-identical after the
launch, as must the padding columns [Cout, ldy) of y and y2; the live elements start as NaN (forward) or as a seeded non-zero fp32
content (dw, dbias: the call accumulates) and must come out without a NaN and inside the bound."""
import math

import pytest
import torch

import conv_geometry_cases as C
import fp64_ref as R
from climate2weather_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEVICE = torch.device("cuda:0")
FAMILY = {_lib.KERNEL_GATHER: "gather", _lib.KERNEL_PATCH_8X16: "8x16 patch", _lib.KERNEL_PATCH_16X16: "16x16 tile", _lib.KERNEL_PATCH_PAIR: "pair",
          _lib.KERNEL_PATCH_TS2: "ts2 patch", _lib.KERNEL_PATCH_S2: "s2 patch"}
KNOBS = sorted({k for r in C.FORWARD for k, _ in r.knobs} | {"C2W_FORCE_GATHER"})
SEEN, SEEN_WGRAD, ORDERS, WORST = set(), set(), set(), {}
SPLIT_RAN, FORWARD_RAN = [], set()
INT = {2: torch.int16, 4: torch.int32}


@pytest.fixture(autouse=True)
def _knobs_follow_the_environment():
    """monkeypatch restores the environment after a test; the library's knob table (read once) must follow."""
    yield
    ops.knobs_reload()


def _sync():
    torch.cuda.synchronize()


def _cus():
    return torch.cuda.get_device_properties(DEVICE).multi_processor_count


def _set_knobs(monkeypatch, knobs):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs:
        monkeypatch.setenv(k, v)
    ops.knobs_reload()


def _note(route, dt, worst):
    WORST[(route, dt)] = max(WORST.get((route, dt), 0.0), worst)


def _arena(n, T, fill):
    """(allocation, the n-element view ARENA_OFFSET bytes into it): head and tail hold `fill`, the tail at least the view's size again"""
    esz = torch.empty((), dtype=T).element_size()
    head = C.ARENA_OFFSET // esz
    buf = torch.full((head + 2 * n + 4096 // esz,), fill, dtype=T, device=DEVICE)
    view = buf[head:head + n]
    assert view.data_ptr() % 16 == 0 and view.data_ptr() % 128 != 0
    return buf, view


def guarded(t):
    """an input: a copy of the CPU tensor t in the middle of NaN"""
    _, view = _arena(t.numel(), t.dtype, float("nan"))
    view.copy_(t.reshape(-1))
    return view.view(t.shape)


class Out:
    """an output in the middle of a fill.  live_cols: the columns [0, live_cols) of the rows start as NaN and may be written, the rest of
    the rows keeps the fill; init: the (fp32) content the call accumulates onto -- every element live."""

    def __init__(self, shape, T, fill, live_cols=None, init=None):
        n = math.prod(shape)
        self.buf, flat = _arena(n, T, fill)
        self.t = flat.view(shape)
        self.head, self.n, self.shape, self.live_cols = C.ARENA_OFFSET // self.t.element_size(), n, shape, live_cols
        if init is not None:
            self.t.copy_(init.view(shape))
        elif live_cols is not None:
            self.t[:, :live_cols] = float("nan")
        self.before = self.buf.clone()

    def _live(self, buf):
        v = buf[self.head:self.head + self.n].view(self.shape)
        return v if self.live_cols is None else v[:, :self.live_cols]

    def assert_guards_intact(self, what):
        after = self.buf.clone()
        self._live(after).copy_(self._live(self.before))
        it = INT[after.element_size()]
        same = after.view(it) == self.before.view(it)
        if not bool(same.all()):
            i = int((~same).nonzero()[0].item()) - self.head
            where = f"element {i} of the tensor (padding column {i % self.shape[-1]})" if 0 <= i < self.n else f"{i if i < 0 else i - self.n} elements {'before' if i < 0 else 'behind'} the tensor"
            raise AssertionError(f"{what}: {int((~same).sum().item())} guard elements disturbed, first at {where}")


_CACHE = {}


def _forward_case(name, ti, dt):
    """operands in their arenas, the reference's accumulator and the planted term: computed once per (row, triple, dtype), shared by
    the three `naive` values, never modified"""
    key = (name, ti, dt)
    if _CACHE.get("key") != key:
        row = C.FORWARD_BY_NAME[name]
        g, o = C.forward_operands(row, ti, dt)
        o = {k: guarded(v) for k, v in o.items()}
        _CACHE.clear()
        _CACHE.update(key=key, g=g, o=o, pre=R.conv_sum(o["x"], o["w"], g), term=C.missing_tap(o, g))
    return _CACHE["g"], _CACHE["o"], _CACHE["pre"], _CACHE["term"]


def _launch_and_hold(what, route, g, o, pre, term, dt, epi, naive, splitk=None):
    T = C.TD[dt]
    npix, Cout, ldy = g["B"] * g["Hout"] * g["Wout"], g["Cout"], g["ldy"]
    bias, kw = C.epilogue_kwargs(epi, o)
    pair = epi == "relu pair"
    y = Out((npix, ldy), T, 7.0, live_cols=Cout)
    y2 = Out((npix, ldy), T, 3.0, live_cols=Cout) if pair else None
    outs = [(y, "y")] + ([(y2, "y2")] if pair else [])
    if splitk is not None:
        ns, nbytes = splitk
        ws = Out((nbytes // 4,), torch.float32, 5.0, init=torch.zeros(nbytes // 4))
        outs.append((ws, "split-K scratch"))
        kw = dict(kw, splitk=(ws.t, ns))
    ops.conv(o["x"], o["w"], bias, y.t, g, dt, naive=naive, y2=y2.t if pair else None, **kw)
    _sync()
    kw.pop("splitk", None)
    ref = R.conv(o["x"], o["w"], g, dt, bias=bias, pre=pre, **kw)
    for out, n in outs:
        out.assert_guards_intact(f"{what}: {n}")
    live = y.t[:, :Cout]
    assert not bool(torch.isnan(live).any()), f"{what}: {int(torch.isnan(live).sum().item())} live elements of y are NaN"
    _note(route, dt, R.assert_within(live, ref["y"], what=what, layout=R.layout(g)))
    if pair:
        assert not bool(torch.isnan(y2.t[:, :Cout]).any()), f"{what}: live elements of y2 are NaN"
        R.assert_mask_consistent(live, y2.t[:, :Cout], what=what + " mask")
    if epi == "none":  # the power check: one tap of input channel 0 missing at the border pixels of image 0
        R.assert_rejects(live.double() - term, ref["y"], what=what + ", planted missing border tap")


def _assert_refusals(what, g, o, dt):
    """a fused form that answers `not supported` for the geometry is refused by the launcher, and nothing is written"""
    T = C.TD[dt]
    npix = g["B"] * g["Hout"] * g["Wout"]
    forms = []
    if not ops.conv_pool2_supported(g, dt):
        forms.append(("pool2", dict(pool2=True)))
    if not ops.conv_lnfwd_supported(g, dt):
        forms.append(("fused LayerNorm forward", "lnf"))
    if not ops.conv_lnbwd_supported(g, dt):
        forms.append(("fused LayerNorm backward", "ln"))
    for form, kw in forms:
        y, side = Out((npix, g["ldy"]), T, 7.0), Out((npix, g["ldy"]), T, 3.0)
        if kw == "lnf":
            kw = dict(lnf=dict(y=side.t, m=None, ldm=0, eps=1e-5, unbiased=True))
        elif kw == "ln":
            kw = dict(ln=dict(x=o["res"], m=None, dm=None, ldm=0, eps=1e-5, unbiased=True))
        with pytest.raises(_lib.C2wError):
            ops.conv(o["x"], o["w"], None, y.t, g, dt, **kw)
        _sync()
        y.live_cols = side.live_cols = 0
        y.assert_guards_intact(f"{what}: y of the refused {form}")
        side.assert_guards_intact(f"{what}: second output of the refused {form}")


@pytest.mark.parametrize("name,ti,dt,naive", C.forward_cases(), ids=lambda v: str(v).replace(" ", "_"))
def test_conv_forward_geometry(name, ti, dt, naive, monkeypatch):
    row = C.FORWARD_BY_NAME[name]
    _set_knobs(monkeypatch, row.knobs if naive == 0 else ())  # naive 1 and 2 read no knob: they run with none set
    g, o, pre, term = _forward_case(name, ti, dt)
    fam = ops.conv_dispatch(g, dt)
    if naive == 0:
        assert row.wanted(dt) is None or fam == row.wanted(dt), f"{name}: dispatches to {FAMILY[fam]}"
        SEEN.add(fam)
    if row.mode == C.TS2 and (naive == 2 or (naive == 0 and fam == _lib.KERNEL_GATHER)):
        # the pixel order is inferred, not observed: ts2_parity_order restates conv_igemm.hip's `par` and its choice of the pixel tile
        # (launch_mode's `small`); if either changes there, the restatement has to follow
        ORDERS.add(C.ts2_parity_order(g, _cus()))
    route = {0: FAMILY[fam], 1: "direct", 2: "gather (forced)"}[naive]
    tag = f"{name} (Cout, ldy, wrows)={C.triples(dt)[ti]} dt={dt} naive={naive}"
    for epi in C.EPILOGUES:
        _launch_and_hold(f"{tag} {epi}", route, g, o, pre, term, dt, epi, naive)
        if naive == 0 and epi != "relu pair":  # the plan takes no second output
            ns, nbytes = ops.conv_splitk_plan(g, dt, C.epilogue_kwargs(epi, o)[1].get("act", R.ACT_NONE))
            if ns > 1:
                SPLIT_RAN.append(name)
                _launch_and_hold(f"{tag} {epi} split-K x{ns}", route + " split-K", g, o, pre, term, dt, epi, naive, splitk=(ns, nbytes))
    if naive == 0:
        _assert_refusals(tag, g, o, dt)
    FORWARD_RAN.add((name, ti, dt, naive))


def _wgrad_variant(what, route, g, o, rw, rb, dt, deterministic, workspace):
    taps = 1 if g["mode"] == C.X1 else 9
    dw = Out((g["Cout"] * taps * g["Cin"],), torch.float32, 7.0, init=o["dw0"])
    db = Out((g["Cout"],), torch.float32, 3.0, init=o["db0"])
    outs = [(dw, "dw"), (db, "dbias")]
    ws = None
    if workspace:
        need = ops.conv_wgrad_workspace_bytes(g, dt, deterministic=deterministic)
        ws = Out((max(need // 4, 4),), torch.float32, 5.0, init=torch.zeros(max(need // 4, 4)))
        outs.append((ws, "workspace"))
    ops.conv_wgrad(o["x"], o["dy"], dw.t, g, dt, dbias=db.t, workspace=ws.t if ws is not None else None, deterministic=deterministic)
    _sync()
    for out, n in outs:
        out.assert_guards_intact(f"{what}: {n}")
    assert not bool(torch.isnan(dw.t).any()) and not bool(torch.isnan(db.t).any()), f"{what}: NaN in dw or dbias"
    _note(route, dt, R.assert_within(dw.t, R.accumulated(o["dw0"], rw.view(-1)), what=what + " dw"))
    _note(route + " dbias", dt, R.assert_within(db.t, R.accumulated(o["db0"], rb), what=what + " dbias"))


@pytest.mark.parametrize("name,ci,dt", C.wgrad_cases(), ids=lambda v: str(v).replace(" ", "_"))
def test_conv_wgrad_geometry(name, ci, dt, monkeypatch):
    row = C.WGRAD_BY_NAME[name]
    _set_knobs(monkeypatch, ())
    g, o = C.wgrad_operands(row, ci, dt)
    o = {k: (guarded(v) if k in ("x", "dy") else v.to(DEVICE)) for k, v in o.items()}
    rw, rb = R.wgrad(o["x"], o["dy"], g)
    fam = ops.conv_wgrad_dispatch(g, dt)
    assert fam == row.want, f"{name}: the weight gradient dispatches to {FAMILY[fam]}"
    SEEN_WGRAD.add(fam)
    tag = f"wgrad {name} (Cout, ldy)={C.WGRAD_COUTS[ci]} dt={dt}"
    for variant, det, wsp in (("atomics", False, False), ("workspace", False, True), ("deterministic", True, True)):
        _wgrad_variant(f"{tag} {variant}", f"wgrad {FAMILY[fam]} {variant}", g, o, rw, rb, dt, det, wsp)
    if fam != _lib.KERNEL_GATHER:  # two kernels exist: the same on the gather kernel
        _set_knobs(monkeypatch, (("C2W_FORCE_GATHER", "1"),))
        assert ops.conv_wgrad_dispatch(g, dt) == _lib.KERNEL_GATHER
        SEEN_WGRAD.add(_lib.KERNEL_GATHER)
        for variant, det, wsp in (("atomics", False, False), ("workspace", False, True), ("deterministic", True, True)):
            _wgrad_variant(f"{tag} forced gather {variant}", f"wgrad gather (forced) {variant}", g, o, rw, rb, dt, det, wsp)


@pytest.mark.parametrize("dt", C.DTYPES)
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("n", [2, C.GROUP_MAX])
@pytest.mark.parametrize("name,couts", C.GROUPED, ids=lambda v: str(v).replace(" ", "_"))
def test_conv_wgrad_grouped_geometry(name, couts, n, deterministic, dt, monkeypatch):
    """the grouped entry points at n = 2 and at the routes' maximum: every item in arenas of its own, every second one without a dbias"""
    row = C.WGRAD_BY_NAME[name]
    _set_knobs(monkeypatch, ())
    g = row.geom(dt, couts[0], couts[1], couts[0])
    assert ops.conv_wgrad_grouped_supported(g, n, dt) and not ops.conv_wgrad_grouped_supported(g, C.GROUP_MAX + 1, dt)
    taps = 1 if g["mode"] == C.X1 else 9
    items, outs = [], []
    for i in range(n):
        _, o = C.wgrad_operands(row, couts, dt, item=i)
        x, dy = guarded(o["x"]), guarded(o["dy"])
        dw = Out((g["Cout"] * taps * g["Cin"],), torch.float32, 7.0, init=o["dw0"])
        db = Out((g["Cout"],), torch.float32, 3.0, init=o["db0"])
        items.append((x, dy, dw, db, o))
        outs += [(dw, f"dw of item {i}"), (db, f"dbias of item {i}")]
    need = ops.conv_wgrad_grouped_workspace_bytes(g, n, dt, deterministic=deterministic)
    ws = Out((max(need // 4, 4),), torch.float32, 5.0, init=torch.zeros(max(need // 4, 4)))
    outs.append((ws, "workspace"))
    ops.conv_wgrad_grouped([(x, dy, dw.t, db.t if i % 2 == 0 else None) for i, (x, dy, dw, db, _) in enumerate(items)], g, dt, workspace=ws.t,
                           deterministic=deterministic)
    _sync()
    what = f"grouped wgrad {name} n={n} dt={dt} deterministic={deterministic}"
    for out, nm in outs:
        out.assert_guards_intact(f"{what}: {nm}")
    route = f"wgrad grouped {'1x1' if g['mode'] == C.X1 else 'patch'}{' deterministic' if deterministic else ''}"
    for i, (x, dy, dw, db, o) in enumerate(items):
        rw, rb = R.wgrad(x, dy, g)
        _note(route, dt, R.assert_within(dw.t, R.accumulated(o["dw0"].to(DEVICE), rw.view(-1)), what=f"{what} dw of item {i}"))
        if i % 2 == 0:
            _note(route + " dbias", dt, R.assert_within(db.t, R.accumulated(o["db0"].to(DEVICE), rb), what=f"{what} dbias of item {i}"))
        else:
            assert torch.equal(db.t, o["db0"].to(DEVICE)), f"{what}: the dbias nobody passed was written (item {i})"


def test_the_table_reached_every_route(monkeypatch):
    """every value c2w_conv_dispatch and c2w_conv_wgrad_dispatch can return is reached by the table on this device, split-K runs, and the
    gather stride-2 input gradient takes both its parity-class and its identity order (inferred from the restated rule, see
    test_conv_forward_geometry).  Walks the table's dispatch answers itself, so a selection of the tests above still checks the table;
    where all forward cases ran, what the launches themselves recorded must be the whole set too, and split-K must have run."""
    families = set(FAMILY)
    seen, seen_w, orders, split = set(), set(), set(), 0
    for r in C.FORWARD:
        _set_knobs(monkeypatch, r.knobs)
        for dt in r.dtypes():
            for t in C.triples(dt):
                g = r.geom(dt, *t)
                fam = ops.conv_dispatch(g, dt)
                seen.add(fam)
                split += ops.conv_splitk_plan(g, dt)[0] > 1
                if r.mode == C.TS2:  # naive = 2 runs every one of them on the gather kernel
                    orders.add(C.ts2_parity_order(g, _cus()))
    _set_knobs(monkeypatch, ())
    for r in C.WGRAD:
        for dt in C.DTYPES:
            for co in C.WGRAD_COUTS:
                seen_w.add(ops.conv_wgrad_dispatch(r.geom(dt, co[0], co[1], co[0]), dt))
    assert seen == families, {FAMILY[f] for f in families - seen}
    assert seen_w == {_lib.KERNEL_GATHER, _lib.KERNEL_PATCH_8X16, _lib.KERNEL_PATCH_PAIR}
    assert orders == {True, False} and split > 0
    assert SEEN <= seen and ORDERS <= orders
    if FORWARD_RAN == set(C.forward_cases()):  # the forward tests ran: the launches reached all of it
        assert SEEN == families, {FAMILY[f] for f in families - SEEN}
        assert ORDERS == {True, False}
        assert SPLIT_RAN, "no launch of the table ran with a split-K plan"
    for (route, dt), worst in sorted(WORST.items()):
        R.report(f"conv geometry, {route}, dt={dt}", worst)
