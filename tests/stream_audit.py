"""Stream audit: a happens-before checker for everything a run enqueues on HIP streams.

An ordering bug is a property of the host's enqueue order and of the event edges between the streams, not of timing: a launch B that
touches bytes an earlier launch A on ANOTHER stream wrote (or writes bytes A read) is safe only if some chain of event records and
waits puts B behind A.  Whether the two happen to run in order on a given machine (two streams of a process often share one hardware
queue, climate2weather_amd/streams.py) says nothing.  So one run is recorded, once, and checked from the record alone.

``record(monkeypatch, ops_module)`` is a context manager that yields a ``Trace`` -- one list of entries in host enqueue order:
  * every launcher of ``climate2weather_amd.ops`` (wrapped like launch_replay.install wraps them; SIGS, leaves, WRITES, SCRATCH and
    live_regions of that module are reused): name, launch index, the raw handle of torch's current stream, read and written footprints.
    Host queries and knobs_reload record nothing; publish_scalar reads its source; scratch arguments count as written;
  * every ATen op, through a TorchDispatchMode: arguments whose schema alias_info says is_write are written, outputs with storage of
    their own are written (and that storage is "fresh on the current stream", rule R2), every other tensor argument is read.  Ops whose
    outputs all alias an input without a write (views) are skipped, and so is a bare allocation (torch.empty enqueues nothing; its
    storage is still fresh on its stream); record_stream is a lifetime note; _local_scalar_dense and
    device-to-host copies are a read followed by "the host joins that stream";
  * Event.record / Event.wait / Event.synchronize, Stream.synchronize and torch.cuda.synchronize.  In the installed torch
    Stream.wait_event is ``event.wait(self)``, Stream.record_event is ``event.record(self)`` and Stream.wait_stream is
    ``self.wait_event(stream.record_event())``: all three arrive through the two Event methods and are recorded ONCE, there
    (tests/test_gpu_stream_order.py::test_the_stream_methods_are_python_over_the_event_methods pins that);
  * async collectives: ``dist.all_reduce(t, async_op=True)`` reads and writes t on a pseudo-stream of its own, forked from the issuing
    stream; ``work.wait()`` makes the CURRENT stream wait for that pseudo-stream (ProcessGroupNCCL's contract).

The recorder keeps every storage it sees alive until the recording ends, so no block is freed and handed out again inside a trace and
an address names one buffer.  That HIDES reuse-after-free from rule R1 (a temporary freed while a side stream still reads it would be
a second buffer at the same address); rule R2 is there for it.

Analysis (``r1``, ``r2``, ``power``): vector clocks.  Every stream, the host and every collective pseudo-stream is a timeline.  An entry on stream S
gets S's clock after the increment, joined with the host's; Event.record snapshots the stream's clock into the event; a wait joins the
snapshot the event holds AT THE TIME OF THE WAIT CALL (never recorded: nothing; recorded again later: the earlier wait is unchanged);
the synchronising calls join into the host.  No implicit ordering with the default stream is assumed.
  R1 (data)      two entries A (earlier), B on different timelines whose footprints share a byte, at least one of the two touches a
                 write (atomic accumulations are writes): clock(B)[timeline(A)] >= seq(A).
  R2 (lifetime)  a storage first seen as a fresh output on stream A and touched on a stream S != A, which nobody but the recorder owns
                 when the recording ends (torch._C._storage_Use_Count against the recorder's own calibrated share), must have had
                 record_stream(S): the contract Engine._on_grad_stream states.  R2_EXEMPT is the only way round it, by name and with
                 a reason, and an entry holds only where the trace shows why it is safe: the recorder notes the moment the last owner
                 of such a storage lets go (``release``), and the stream that allocated it must by then be ordered behind S's last
                 use -- the allocator hands a freed block out again on the stream that allocated it, nowhere else.

Footprints are sets of byte ranges [lo, hi) of device addresses, kept as boxes (lo, rows, width, pitch): ``rows`` ranges of ``width``
bytes, ``pitch`` apart -- the rows x C of an NHWC buffer with padding columns are not one range.  Where the engine hands a launcher the
open-ended tail of a flat buffer (flat_grad[w_off:], the packed weights, a whole trajectory) the footprint comes from the launcher's
integer arguments as include/c2w_hip.h defines them (``EXACT``); tests/test_stream_audit_cpu.py holds each of those against what the
restatement of the launcher really writes.  Everything in a Trace is plain data (ints, strings, tuples): it can be pickled and analysed
elsewhere.
"""
from __future__ import annotations

import contextlib
import gc
from collections import Counter

import torch
from torch.utils._python_dispatch import TorchDispatchMode

import launch_replay as LR

HOST = "host"
UNRECORDED = {"knobs_reload", "check", "new_workspace"}  # no launch: the environment, the error-code helper, a torch allocation (ATen sees it)
# R2: (name of the first entry that touched the storage on another stream, argument path) -> reason.  Any other crossing without
# record_stream is a finding, and so is a listed one whose block was let go before its stream was ordered behind the last use (r2).
R2_EXEMPT: dict = {
    ("conv_center", "out"): "score_fn's eps: allocated on the caller's stream, written by the window-batch streams, handed back behind the "
                            "wait_stream loop; the caller lets go of it on its own stream, behind that join",
    ("timestep_embedding", "t"): "score_fn's device copy of t: a local, read by every window-batch stream, dropped when score_fn returns -- "
                                 "behind the wait_stream loop on the stream that allocated it",
    ("window_gather", "x"): "score_fn's device copy of a host trajectory: as its copy of t",
    ("conv_wgrad", "dw"): "the module path's private gradient buffer: written on the gradient stream, delivered to autograd behind the "
                          "segment events and join_grad_stream, let go by autograd on the caller's stream after its accumulation",
}


# ------------------------------------------------------------------------------------------------------------------ boxes

def box(lo, nbytes):
    return (int(lo), 1, int(nbytes), int(nbytes))


def rows_box(lo, rows, width, pitch):
    """``rows`` ranges of ``width`` bytes, ``pitch`` bytes apart; one range where they touch"""
    if rows <= 1 or width >= pitch:
        return box(lo, (rows - 1) * pitch + width if rows >= 1 else 0)
    return (int(lo), int(rows), int(width), int(pitch))


def hull(b):
    lo, rows, width, pitch = b
    return lo, lo + (rows - 1) * pitch + width


def ranges(b):
    lo, rows, width, pitch = b
    return [(lo + r * pitch, lo + r * pitch + width) for r in range(rows)] if width else []


def _hit(lo, hi, b):
    """the first bytes of [lo, hi) inside box b, or None"""
    blo, rows, width, pitch = b
    if lo >= hi or not width:
        return None
    k = max(0, (lo - blo - width) // pitch + 1)  # the first row that ends behind lo
    if k >= rows:
        return None
    s, e = max(lo, blo + k * pitch), min(hi, blo + k * pitch + width)
    return (s, e) if s < e else None


def overlap(a, b):
    """the first byte range two boxes share, or None.  Exact: adjacent ranges and the gaps between rows do not count."""
    (alo, ahi), (blo, bhi) = hull(a), hull(b)
    if alo >= bhi or blo >= ahi:
        return None
    if a[1] > b[1]:
        a, b = b, a
    for lo, hi in ranges(a):
        h = _hit(lo, hi, b)
        if h:
            return h
    return None


def tensor_box(t):
    """the bytes a tensor view can touch: exact for a dense view and for dense rows under one outer stride, else the hull"""
    esz = t.element_size()
    if t.numel() == 0:
        return box(t.data_ptr(), 0)
    dims = [(s, st) for s, st in zip(t.shape, t.stride()) if s > 1]
    inner = 1
    while dims and dims[-1][1] == inner:
        inner *= dims.pop()[0]
    if not dims:
        return box(t.data_ptr(), inner * esz)
    if len(dims) == 1 and dims[0][1] > inner:
        return rows_box(t.data_ptr(), dims[0][0], inner * esz, dims[0][1] * esz)
    lo, hi = LR._span(t)
    return box(lo, hi - lo)


class TD(tuple):
    """what the footprints need of a tensor argument: (address, box, element size, storage address)"""
    __slots__ = ()
    ptr = property(lambda s: s[0])
    box = property(lambda s: s[1])
    esz = property(lambda s: s[2])
    skey = property(lambda s: s[3])


def describe(t):
    return TD((t.data_ptr(), tensor_box(t), t.element_size(), t.untyped_storage().data_ptr()))


# ------------------------------------------------------------------------------- footprints from the launchers' integer arguments

def _n(td, count):
    return [box(td.ptr, count * td.esz)]


def _rows(td, rows, C, ld):
    return [rows_box(td.ptr, rows, C * td.esz, ld * td.esz)]


def _get(a, path):
    try:
        v = LR.at(a, path)
    except (KeyError, IndexError, TypeError):
        return None
    return v if isinstance(v, TD) else None


def _live(name, a):
    """launch_replay.live_regions as boxes: the conv and weight-gradient outputs"""
    out = {}
    for p, (n, ld, C) in LR.live_regions(name, a).items():
        td = _get(a, p)
        if td is not None:
            out[p] = _rows(td, n, C, ld)
    return out


def _x_conv(a):
    g = a["g"]
    out = _live("conv", a)
    if a.get("no_y"):
        out.pop(("y",), None)
    dm = _get(a, ("ln", "dm"))
    if dm is not None:  # [B][ldm] modulation-gradient rows, or one shared row
        ldm = int(a["ln"].get("ldm", 0))
        out[("ln", "dm")] = _rows(dm, g["B"], g["Cout"], ldm) if ldm else _n(dm, g["Cout"])
    w = _get(a, ("w",))
    if w is not None:  # the engine hands over the tail of the shadow / packed buffer from this matrix on
        taps = LR._taps(g)
        out[("w",)] = _n(w, 9 * g["Cin"] * ((g["wrows"] + 127) // 128 * 128) if a.get("wpacked") else g["wrows"] * taps * g["Cin"])
    if _get(a, ("bias",)) is not None:
        out[("bias",)] = _n(a["bias"], g["wrows"])
    return out


def _x_wgrad(a):
    return _live("conv_wgrad", a)


def _x_wgrad_grouped(a):
    return _live("conv_wgrad_grouped", a)


def _frames(td, F, HW, frames):
    """whole frames of an [L][F][HW] trajectory, neighbours merged"""
    out, fb = [], F * HW * td.esz
    for f in sorted(set(frames)):
        if out and out[-1][0] + out[-1][2] == td.ptr + f * fb:
            out[-1] = box(out[-1][0], out[-1][2] + fb)
        else:
            out.append(box(td.ptr + f * fb, fb))
    return out


def kept_frames(nw, k, i0, nwin_total):
    """fold (include/c2w_hip.h::c2w_window_scatter): the centre frame of every window, the leading k of window 0, the trailing k of the last"""
    out = []
    for gi in range(i0, i0 + nw):
        out += [gi + tau for tau in range(2 * k + 1) if tau == k or (gi == 0 and tau < k) or (gi == nwin_total - 1 and tau > k)]
    return out


def _x_window_gather(a):
    w = 2 * a["k"] + 1
    return {("y",): _n(a["y"], a["nw"] * a["HW"] * a["ldc"]), ("x",): _frames(a["x"], a["F"], a["HW"], range(a["i0"], a["i0"] + a["nw"] - 1 + w))}


def _x_window_scatter(a):
    return {("eps",): _frames(a["eps"], a["F"], a["HW"], kept_frames(a["nw"], a["k"], a["i0"], a["nwin_total"])),
            ("y",): _n(a["y"], a["nw"] * a["HW"] * a["ldc"])}


def _x_conv_center(a):
    out = {("out",): [rows_box(a["out"].ptr, a["B"], a["nr"] * a["H"] * a["W"] * a["out"].esz, a["ostride"] * a["out"].esz)],
           ("w",): _n(a["w"], a["wrows"] * 9 * a["Cin"]), ("x",): _n(a["x"], a["B"] * a["H"] * a["W"] * a["Cin"])}
    if a.get("bias") is not None:
        out[("bias",)] = _n(a["bias"], a["wrows"])
    return out


def _x_fold_list(a):
    """frames l0 <= l < l0 + nl: a frame no window of the list contains is left alone, but the list lives on the device"""
    return {("out",): _frames(a["out"], a["F"], a["HW"], range(a["l0"], a["l0"] + a["nl"])),
            ("dx",): _n(a["dx"], a["n"] * (2 * a["k"] + 1) * a["F"] * a["HW"])}


def _x_cotangent_list(a):
    return {("dy",): _n(a["dy"], a["n"] * a["HW"] * a["ldc"])}


def _x_gather_list(a):
    return {("y",): _n(a["y"], a["n"] * a["HW"] * a["ldc"])}


def _x_adamw(a):
    return {(k,): _n(a[k], a["n"]) for k in ("p", "g", "m", "v", "ema", "shadow") if a.get(k) is not None}


def _x_nchw(a):
    out = {("y",): _n(a["y"], a["B"] * a["HW"] * a["ldc"])}
    if isinstance(a.get("x"), TD) and a.get("img_off") is None:
        out[("x",)] = _n(a["x"], a["B"] * a["C"] * a["HW"])
    if isinstance(a.get("eps"), TD):
        out[("eps",)] = _n(a["eps"], a["B"] * a["C"] * a["HW"])
    if isinstance(a.get("erows"), TD):
        out[("erows",)] = _n(a["erows"], a["B"] * a["HW"] * a["lde"])
    return out


def _x_flat(*names):
    """the flat kernels: ``n`` elements of each named argument"""
    return lambda a: {(k,): _n(a[k], a["n"]) for k in names if isinstance(a.get(k), TD)}


def _x_pack(a):
    """desc rows (src_off, dst_off, rows, cin), read back by the recorder: every matrix's own slot, nothing between them"""
    src, dst = a["src"], a["dst"]
    return {("dst",): [box(dst.ptr + do * dst.esz, 9 * k * ((r + 127) // 128 * 128) * dst.esz) for so, do, r, k in a["desc_rows"]],
            ("src",): [box(src.ptr + so * src.esz, r * 9 * k * src.esz) for so, do, r, k in a["desc_rows"]]}


EXACT = {
    "conv": _x_conv, "conv_wgrad": _x_wgrad, "conv_wgrad_grouped": _x_wgrad_grouped, "window_gather": _x_window_gather,
    "window_scatter": _x_window_scatter, "conv_center": _x_conv_center, "window_grad_fold_list": _x_fold_list,
    "window_cotangent_list": _x_cotangent_list, "window_gather_list": _x_gather_list, "adamw_ema": _x_adamw, "nchw_to_nhwc": _x_nchw,
    "nchw_to_nhwc_noise": _x_nchw, "nchw_to_nhwc_noise_rows": _x_nchw, "windows_to_nhwc_noise": _x_nchw,
    "pack_conv_weights_batched": _x_pack, "silu": _x_flat("x", "y"), "silu_backward": _x_flat("x", "dy", "dx"),
    "sampler_predict": _x_flat("x", "eps"), "sampler_correct": _x_flat("x", "eps", "z"), "ema_update": _x_flat("ema", "p"),
    "cast_f32": _x_flat("src", "dst"), "grad_scaler_check": _x_flat("g"), "philox_normal": _x_flat("out"), "sumsq": _x_flat("v"),
}


def footprints(name, a):
    """(reads, writes) of one launch: lists of (storage address, box, argument path).  ``a``: the bound arguments with every tensor
    replaced by its TD."""
    decl = LR.WRITES.get(name, [])
    written = set(decl(a) if callable(decl) else decl)
    exact = EXACT[name](a) if name in EXACT else {}
    reads, writes = [], []
    for p, td in _leaves(a):
        boxes = exact.get(p, [td.box])
        (writes if p in written or p[0] in LR.SCRATCH else reads).extend((td.skey, b, LR.pstr(p)) for b in boxes if b[2])
    return reads, writes


def _leaves(v, path=()):
    if isinstance(v, TD):
        yield path, v
    elif isinstance(v, dict):
        for k, x in v.items():
            yield from _leaves(x, path + (k,))
    elif isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            yield from _leaves(x, path + (i,))


def plain(v):
    """an argument tree with every tensor replaced by its TD"""
    if isinstance(v, torch.Tensor):
        return describe(v)
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)) and not isinstance(v, TD):
        return type(v)(plain(x) for x in v)
    return v


# ------------------------------------------------------------------------------------------------------------------ the trace

class Trace:
    """Entries in host enqueue order.  The same constructors serve the recorder and the hand-written traces of the CPU tests."""

    def __init__(self):
        self.entries = []
        # storage address -> dict(fresh=the timeline it was allocated on inside the recording or None, crossed={other timeline: (name, path,
        # position of its first access there)}, noted=timelines of record_stream, last={timeline: position of its last access},
        # released=position of the release entry or None, owned=does anybody but the recorder own it at the end)
        self.storages = {}
        self.names = {}      # storage address -> [(lo, hi, name)]: engine attributes, for the report
        self.launches = 0
        self._coll = 0
        self._ev = 0
        self.before_push = None  # the recorder's hooks: look for released storages before an entry goes in / a storage crossed streams
        self.on_cross = None

    def _push(self, e):
        if self.before_push is not None:
            self.before_push()
        e["pos"] = len(self.entries)
        self.entries.append(e)
        return e["pos"]

    @staticmethod
    def _storage(fresh=None):
        return dict(fresh=fresh, crossed={}, noted=set(), owned=None, last={}, released=None)

    # -- accesses
    def access(self, name, tl, reads=(), writes=(), src="ops", fresh=()):
        """reads / writes: (storage key, box, path).  ``fresh``: storage keys this entry allocated (rule R2)."""
        e = dict(kind="access", name=name, tl=tl, reads=list(reads), writes=list(writes), src=src)
        self._push(e)
        if src == "ops":
            e["index"] = self.launches
            self.launches += 1
        for sk in fresh:
            self.storages.setdefault(sk, self._storage(tl))
        for sk, _, p in e["reads"] + e["writes"]:
            st = self.storages.setdefault(sk, self._storage())
            st["last"][tl] = e["pos"]
            if st["fresh"] is not None and tl != st["fresh"] and tl not in st["crossed"]:
                st["crossed"][tl] = (name, p, e["pos"])
                if self.on_cross is not None:
                    self.on_cross(sk)
        return e

    def launch(self, name, tl, reads=(), writes=()):
        return self.access(name, tl, reads, writes)

    def fresh(self, skey, tl):
        """a storage allocated on ``tl`` by a call that enqueues nothing (torch.empty)"""
        self.storages.setdefault(skey, self._storage(tl))

    def release(self, skey):
        """nobody but the recorder owns the storage any more: from here on the allocator may hand the block out again, on the stream
        that allocated it"""
        st = self.storages[skey]
        st["released"] = self._push(dict(kind="release", skey=skey, tl=st["fresh"]))

    # -- edges
    def new_event(self):
        self._ev += 1
        return ("ev", self._ev)

    def record_event(self, ev, tl):
        self._push(dict(kind="record", ev=ev, tl=tl))

    def wait_event(self, tl, ev):
        return self._push(dict(kind="wait", ev=ev, tl=tl))

    def wait_stream(self, tl, other):
        """torch's Stream.wait_stream: tl.wait_event(other.record_event()); returns the position of the wait"""
        ev = self.new_event()
        self.record_event(ev, other)
        return self.wait_event(tl, ev)

    def sync_stream(self, tl):
        return self._push(dict(kind="host", what="stream", tl=tl))

    def sync_event(self, ev):
        return self._push(dict(kind="host", what="event", ev=ev))

    def sync_all(self):
        return self._push(dict(kind="host", what="all"))

    def fork(self, tl):
        """a collective's pseudo-stream, ordered behind everything enqueued so far on ``tl``"""
        self._coll += 1
        c = ("coll", self._coll)
        self._push(dict(kind="fork", tl=c, of=tl))
        return c

    def collective(self, name, tl, footprint):
        c = self.fork(tl)
        self.access(name, c, reads=footprint, writes=footprint, src="coll")
        return c

    def work_wait(self, tl, c):
        return self._push(dict(kind="waittl", tl=tl, on=c))

    def note_record_stream(self, skey, tl):
        self._push(dict(kind="note", skey=skey, tl=tl))
        self.storages.setdefault(skey, self._storage())["noted"].add(tl)

    # -- views of the trace
    def accesses(self):
        return [e for e in self.entries if e["kind"] == "access"]

    def wait_edges(self):
        return [e["pos"] for e in self.entries if e["kind"] in ("wait", "waittl")]

    def streams_with_launches(self):
        return {e["tl"] for e in self.entries if e["kind"] == "access" and e["src"] == "ops"}

    def name_of(self, skey, lo):
        for a, b, n in self.names.get(skey, ()):
            if a <= lo < b:
                return f"{n}+{lo - a:#x}"
        return None


# --------------------------------------------------------------------------------------------------------------- the analysis

def _join(c, o):
    for k, v in o.items():
        if c.get(k, 0) < v:
            c[k] = v


def clocks(trace, drop=None, need=None):
    """{position of an access: (sequence number on its timeline, clock)}.  ``drop``: the position of one edge (an event wait, a
    work.wait(), a host synchronisation), or a set of them, to leave out; ``need``: the positions whose clocks are wanted (default: all)."""
    C, evs, out = {HOST: {}}, {}, {}
    drop = set() if drop is None else ({drop} if isinstance(drop, int) else set(drop))
    for e in trace.entries:
        k = e["kind"]
        if e["pos"] in drop:
            continue
        if k == "release":
            c = C.setdefault(e["tl"], {})
            _join(c, C[HOST])
            out[e["pos"]] = (None, dict(c))
        elif k == "access":
            c = C.setdefault(e["tl"], {})
            _join(c, C[HOST])
            c[e["tl"]] = c.get(e["tl"], 0) + 1
            if need is None or e["pos"] in need:
                out[e["pos"]] = (c[e["tl"]], dict(c))
        elif k == "record":
            c = C.setdefault(e["tl"], {})
            _join(c, C[HOST])
            evs[e["ev"]] = dict(c)
        elif k == "wait":
            if e["ev"] in evs:
                _join(C.setdefault(e["tl"], {}), evs[e["ev"]])
        elif k == "waittl":
            _join(C.setdefault(e["tl"], {}), C.get(e["on"], {}))
        elif k == "fork":
            c = C.setdefault(e["of"], {})
            _join(c, C[HOST])
            C[e["tl"]] = dict(c)
        elif k == "host":
            if e["what"] == "stream":
                _join(C[HOST], C.get(e["tl"], {}))
            elif e["what"] == "event":
                _join(C[HOST], evs.get(e["ev"], {}))
            else:
                for tl in list(C):
                    if tl != HOST:
                        _join(C[HOST], C[tl])
    return out


def conflicting_pairs(trace):
    """Every (A, B) the data rule has to look at: for each footprint of an entry B and each OTHER timeline, the latest earlier entry A
    on that timeline that shares a byte with it, one of the two touches a write.  (Clocks grow along a timeline: if the latest is
    ordered before B, so is every earlier one.)  Footprints are indexed per storage, and a storage only one timeline ever touches is
    never searched.  -> [(pos A, pos B, (lo, hi), path A, path B, storage key)]"""
    index, tls = {}, {}
    pairs = []
    for e in trace.entries:
        if e["kind"] != "access":
            continue
        tl = e["tl"]
        mine = [(sk, b, p, False) for sk, b, p in e["reads"]] + [(sk, b, p, True) for sk, b, p in e["writes"]]
        for sk, b, p, w in mine:
            others = tls.get(sk, set()) - {tl}
            if not others:
                continue
            found = set()
            for pos, otl, ob, op, ow in reversed(index[sk]):
                if otl == tl or otl in found or not (w or ow):
                    continue
                h = overlap(ob, b)
                if h:
                    pairs.append((pos, e["pos"], h, op, p, sk))
                    found.add(otl)
                    if found == others:
                        break
        for sk, b, p, w in mine:
            index.setdefault(sk, []).append((e["pos"], tl, b, p, w))
            tls.setdefault(sk, set()).add(tl)
    return pairs


class Finding:
    def __init__(self, trace, pair, rule="R1"):
        self.rule, self.pair = rule, pair
        a, b, self.bytes, self.path_a, self.path_b, self.skey = pair
        self.a, self.b = trace.entries[a], trace.entries[b]
        self._trace = trace

    @property
    def text(self):
        return self._text(self._trace)

    def key(self):
        return (self.a["name"], self.a.get("index"), self.b["name"], self.b.get("index"))

    def _text(self, tr):
        a, b = self.a, self.b
        w_b = max((e["pos"] for e in tr.entries[: b["pos"]] if e["kind"] in ("wait", "waittl") and e["tl"] == b["tl"]), default=None)
        r_a = next((e["pos"] for e in tr.entries[a["pos"]:] if e["kind"] == "record" and e["tl"] == a["tl"]), None)
        owner = tr.name_of(self.skey, self.bytes[0])
        return (f"{b['name']} #{b.get('index', b['pos'])} on stream {b['tl']} ({self.path_b}) is not ordered behind {a['name']} "
                f"#{a.get('index', a['pos'])} on stream {a['tl']} ({self.path_a}): bytes [{self.bytes[0]:#x}, {self.bytes[1]:#x})"
                + (f" of {owner}" if owner else "") + f"; last wait on {b['tl']} before it: entry {w_b}; first event recorded on {a['tl']} behind it: entry {r_a}")

    def __repr__(self):
        return self.text


def r1(trace, pairs=None, drop=None):
    """the data rule: the pairs that no chain of edges orders"""
    pairs = conflicting_pairs(trace) if pairs is None else pairs
    clk = clocks(trace, drop, {p for pr in pairs for p in pr[:2]})
    bad = []
    for pr in pairs:
        seq_a, _ = clk[pr[0]]
        _, c_b = clk[pr[1]]
        if c_b.get(trace.entries[pr[0]]["tl"], 0) < seq_a:
            bad.append(Finding(trace, pr))
    return bad


def r2(trace, exempt=None):
    """the lifetime rule -> [(storage key, timeline, (entry name, path, pos), why)].  A temporary (fresh in the recording, owned by nobody
    but the recorder at its end) that another stream touched needs record_stream for that stream.  The only way round is an entry of
    the exemption table, and that entry holds only where the trace shows the block could not be handed out early: when the last owner
    let go (a ``release`` entry) the stream that allocated it -- the one whose pool the block returns to -- was already ordered behind
    the other stream's last use of it."""
    exempt = R2_EXEMPT if exempt is None else exempt
    need = {st["released"] for st in trace.storages.values() if st["released"] is not None}
    need |= {p for st in trace.storages.values() if st["crossed"] for p in st["last"].values()}
    clk = clocks(trace, need=need)
    bad = []
    for sk, st in trace.storages.items():
        if st["fresh"] is None or st["owned"] is not False:
            continue  # not allocated inside the recording, or somebody still owns it
        for tl, who in st["crossed"].items():
            if tl in st["noted"]:
                continue
            if (who[0], who[1]) not in exempt:
                bad.append((sk, tl, who, "no record_stream, and not in the exemption table"))
            elif st["released"] is None or clk[st["released"]][1].get(tl, 0) < clk[st["last"][tl]][0]:
                bad.append((sk, tl, who, "exempt by name, but released before its stream was ordered behind the last use"))
    return bad


def r2_crossings(trace):
    return sum(len(st["crossed"]) for st in trace.storages.values() if st["fresh"] is not None)


def twins(trace):
    """{position of an event wait: the waits of the same stream for the same point of the other streams (itself included)}.  Two joins
    back to back -- nothing enqueued in between on the stream waited for -- are each redundant alone by construction; what can be
    load-bearing is the group."""
    C, evs, sig = {HOST: {}}, {}, {}
    for e in trace.entries:
        if e["kind"] == "access":
            c = C.setdefault(e["tl"], {})
            c[e["tl"]] = c.get(e["tl"], 0) + 1
        elif e["kind"] == "record":
            evs[e["ev"]] = {k: v for k, v in C.get(e["tl"], {}).items() if k == e["tl"]}
        elif e["kind"] == "wait" and e["ev"] in evs:
            sig.setdefault((e["tl"], tuple(sorted(evs[e["ev"]].items(), key=repr))), []).append(e["pos"])
    return {pos: grp for grp in sig.values() for pos in grp}


def power(trace, pairs=None):
    """Delete every wait edge alone and analyse again (host work only) -> {position of the edge: [findings its deletion brings]}"""
    pairs = conflicting_pairs(trace) if pairs is None else pairs
    return {pos: r1(trace, pairs, drop=pos) for pos in trace.wait_edges()}


def assert_clean(trace, pairs=None):
    bad = r1(trace, pairs)
    assert not bad, "%d unordered pairs (R1):\n%s" % (len(bad), "\n".join("  " + f.text for f in bad[:12]))
    life = r2(trace)
    assert not life, "%d temporaries cross streams without record_stream (R2):\n%s" % (
        len(life), "\n".join(f"  storage {sk:#x} allocated on {trace.storages[sk]['fresh']}, used on {tl} by {who[0]} ({who[1]}, entry {who[2]}): {why}"
                              for sk, tl, who, why in life[:12]))


def stats(trace, pairs, pw=None):
    s = dict(records=len(trace.accesses()), launches=trace.launches, streams=len({e["tl"] for e in trace.accesses()}),
             launch_streams=len(trace.streams_with_launches()), edges=len(trace.wait_edges()), pairs=len(pairs), r2_crossings=r2_crossings(trace))
    if pw is not None:
        s["load_bearing"] = sum(1 for v in pw.values() if v)
        s["redundant"] = sum(1 for v in pw.values() if not v)
    return s


# --------------------------------------------------------------------------------------------------------------- the recorder

_ALLOC_ONLY = {"aten::empty", "aten::empty_like", "aten::empty_strided", "aten::new_empty", "aten::new_empty_strided"}  # nothing is enqueued
_HOST_READS = {"aten::_local_scalar_dense", "aten::item", "aten::equal", "aten::is_nonzero"}


def _own_share():
    """how many owners _storage_Use_Count reports for a storage that only a kept UntypedStorage object holds"""
    t = torch.empty(4)
    s = t.untyped_storage()
    del t
    return torch._C._storage_Use_Count(s._cdata)


class _Mode(TorchDispatchMode):
    def __init__(self, rec):
        super().__init__()
        self.rec = rec

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        out = func(*args, **kwargs)
        if not self.rec.paused:
            self.rec.aten(func, args, kwargs, out)
        return out


class Recorder:
    def __init__(self, gpu=None, current_stream=None):
        self.trace = Trace()
        self.gpu = torch.cuda.is_available() if gpu is None else gpu
        self.current_stream = current_stream or self._raw_stream
        self.paused = False
        self.keep = {}     # storage address -> UntypedStorage: nothing is freed and handed out again inside a trace
        self.events = {}   # id(event) -> the event (kept: an id names one event) and its trace id
        self.desc = {}     # address of a descriptor tensor -> its rows
        self.calls = Counter()
        self.share = _own_share()
        self.watch = {}    # fresh storages that crossed streams and still have an owner: address -> UntypedStorage
        self.trace.on_cross = self._watch
        self.trace.before_push = self._poll

    def _watch(self, sk):
        if sk in self.keep and self.trace.storages[sk]["released"] is None:
            self.watch[sk] = self.keep[sk]

    def _poll(self):
        """before anything else goes into the trace: which watched storages has their last owner let go of?"""
        if not self.watch:
            return
        gone = [sk for sk, s in self.watch.items() if torch._C._storage_Use_Count(s._cdata) <= self.share]
        for sk in gone:
            del self.watch[sk]
        for sk in gone:
            self.trace.release(sk)

    @staticmethod
    def _raw_stream():
        return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()) if torch.cuda.is_available() else 0

    def tracked(self, t):
        return isinstance(t, torch.Tensor) and (t.is_cuda or not self.gpu) and t.layout == torch.strided

    def hold(self, t):
        s = t.untyped_storage()
        self.keep.setdefault(s.data_ptr(), s)
        return s.data_ptr()

    def name_storages(self, obj, prefix):
        """remember which attribute of ``obj`` (tensors, and dicts / lists of them, one level) a storage belongs to: for the report"""
        def put(n, t):
            if self.tracked(t) and t.numel():
                lo, hi = LR._span(t)
                self.trace.names.setdefault(t.untyped_storage().data_ptr(), []).append((lo, hi, n))
        for k, v in vars(obj).items():
            if isinstance(v, torch.Tensor):
                put(f"{prefix}.{k}", v)
            elif isinstance(v, dict):
                for kk, vv in v.items():
                    put(f"{prefix}.{k}[{kk!r}]", vv)
            elif isinstance(v, (list, tuple)):
                for i, vv in enumerate(v):
                    put(f"{prefix}.{k}[{i}]", vv)

    # -- launchers
    def launch(self, name, fn, a, kw):
        if name in UNRECORDED or LR.is_host_query(name):
            return fn(*a, **kw)
        ba = LR.SIGS[name].bind(*a, **kw)
        ba.apply_defaults()
        real = dict(ba.arguments)
        for _, t in LR.leaves(real):
            if self.tracked(t):
                self.hold(t)
        desc = plain(real)
        if name == "pack_conv_weights_batched":
            desc["desc_rows"] = self._desc_rows(real["desc"], real["n"])
        reads, writes = footprints(name, desc)
        e = self.trace.launch(name, self.current_stream(), reads, writes)
        self.paused = True
        try:
            ret = fn(*a, **kw)
        finally:
            self.paused = False
        if ret is False:  # "unsupported": nothing was enqueued
            e["kind"] = "refused"
            self.trace.launches -= 1
            assert self.trace.entries[-1] is e
            self.trace.entries.pop()
        else:
            self.calls[name] += 1
        return ret

    def _desc_rows(self, desc, n):
        key = (desc.data_ptr(), n)
        if key not in self.desc:  # read back once per descriptor (the engine keeps them): a host wait the run itself does not have,
            self.paused = True    # and timing is irrelevant to the verdict
            try:
                if desc.is_cuda:
                    _REAL["sync"]()
                self.desc[key] = [tuple(r) for r in desc.reshape(-1, 4)[:n].tolist()]
            finally:
                self.paused = False
        return self.desc[key]

    # -- ATen
    def aten(self, func, args, kwargs, out):
        sch = func._schema
        name = sch.name
        if name.startswith("c10d::"):
            return  # the collectives are recorded where they are issued (record: all_reduce), on a pseudo-stream of their own
        if name == "aten::record_stream":
            if self.tracked(args[0]):
                self.trace.note_record_stream(self.hold(args[0]), _stream_id(args[1]))
            return
        reads, writes, seen = [], [], set()
        non_blocking = False
        vals = list(zip(sch.arguments, args)) + [(s, kwargs[s.name]) for s in sch.arguments if s.name in kwargs]
        cpu_written = False
        for s, v in vals:
            if s.name == "non_blocking":
                non_blocking = bool(v)
            is_w = s.alias_info is not None and s.alias_info.is_write
            for t in (v if isinstance(v, (list, tuple)) else (v,)):
                if not isinstance(t, torch.Tensor) or not t.numel():
                    continue
                if not self.tracked(t):
                    cpu_written = cpu_written or (is_w and not t.is_cuda)
                    continue
                sk = self.hold(t)
                seen.add(sk)
                (writes if is_w else reads).append((sk, tensor_box(t), s.name))
        fresh, cpu_out = [], False
        outs = out if isinstance(out, (list, tuple)) else (out,)
        for i, t in enumerate(outs):
            if not isinstance(t, torch.Tensor) or not t.numel():
                continue
            if not self.tracked(t):
                cpu_out = cpu_out or not t.is_cuda
                continue
            sk = self.hold(t)
            if sk not in seen and sk not in self.trace.storages:
                fresh.append(sk)
                if name not in _ALLOC_ONLY:
                    writes.append((sk, tensor_box(t), f"out{i}"))
                seen.add(sk)
        to_host = bool(reads) and (name in _HOST_READS or (self.gpu and (cpu_out or cpu_written)))
        tl = self.current_stream()
        if not writes and not to_host:
            for sk in fresh:  # an allocation: no entry, but the block belongs to this stream (R2)
                self.trace.fresh(sk, tl)
            return  # else a view, or nothing of ours
        self.trace.access(name, tl, reads, writes, src="aten", fresh=fresh)
        if to_host and not non_blocking:
            self.trace.sync_stream(tl)

    # -- events
    def ev(self, event):
        got = self.events.get(id(event))
        if got is None:
            got = self.events[id(event)] = (event, self.trace.new_event())
        return got[1]


def _stream_id(s):
    h = getattr(s, "cuda_stream", None)
    if h is None:
        h = torch.cuda.Stream(stream_id=s.stream_id, device_index=s.device_index, device_type=s.device_type).cuda_stream
    return h


_REAL = {"sync": torch.cuda.synchronize}


class _Work:
    """an async collective's work object: wait() orders the CURRENT stream behind the collective's pseudo-stream"""

    def __init__(self, rec, work, tl):
        self._rec, self._work, self._tl = rec, work, tl

    def wait(self, *a, **kw):
        self._rec.trace.work_wait(self._rec.current_stream(), self._tl)
        return self._work.wait(*a, **kw)

    def __getattr__(self, k):
        return getattr(self._work, k)


@contextlib.contextmanager
def record(monkeypatch, ops_module, *, gpu=None, current_stream=None, dist_module=None):
    """Record everything enqueued inside the block -> Trace (complete, with the owners of every storage, when the block ends).
    ``recorder`` is reachable as ``trace.recorder`` while the block runs (name_storages)."""
    rec = Recorder(gpu, current_stream)
    tr = rec.trace
    tr.recorder = rec
    with monkeypatch.context() as mp:
        for name in sorted(LR.SIGS):
            fn = getattr(ops_module, name, None)
            if fn is None or not callable(fn):
                continue

            def wrap(name=name, fn=fn):
                def launch(*a, **kw):
                    return rec.launch(name, fn, a, kw)
                launch.__name__, launch.__wrapped__ = name, fn
                return launch
            mp.setattr(ops_module, name, wrap())
        if rec.gpu:
            E, S = torch.cuda.Event, torch.cuda.Stream
            e_record, e_wait, e_sync, s_sync, c_sync = E.record, E.wait, E.synchronize, S.synchronize, torch.cuda.synchronize
            _REAL["sync"] = c_sync

            def record_(self, stream=None):
                stream = torch.cuda.current_stream() if stream is None else stream
                tr.record_event(rec.ev(self), stream.cuda_stream)
                return e_record(self, stream)

            def wait_(self, stream=None):
                stream = torch.cuda.current_stream() if stream is None else stream
                tr.wait_event(stream.cuda_stream, rec.ev(self))
                return e_wait(self, stream)

            def esync_(self):
                tr.sync_event(rec.ev(self))
                return e_sync(self)

            def ssync_(self):
                tr.sync_stream(self.cuda_stream)
                return s_sync(self)

            def csync_(device=None):
                if not rec.paused:
                    tr.sync_all()
                return c_sync(device)
            mp.setattr(E, "record", record_)
            mp.setattr(E, "wait", wait_)
            mp.setattr(E, "synchronize", esync_)
            mp.setattr(S, "synchronize", ssync_)
            mp.setattr(torch.cuda, "synchronize", csync_)
        if dist_module is not None:
            real_ar = dist_module.all_reduce

            def all_reduce(tensor, *a, **kw):
                work = real_ar(tensor, *a, **kw)
                if not rec.tracked(tensor):
                    return work
                fp = [(rec.hold(tensor), tensor_box(tensor), "tensor")]
                tl = rec.current_stream()
                c = tr.collective("all_reduce", tl, fp)
                if kw.get("async_op") and work is not None:
                    return _Work(rec, work, c)
                tr.work_wait(tl, c)  # the blocking form: the issuing stream is behind it on return
                return work
            mp.setattr(dist_module, "all_reduce", all_reduce)
        try:
            with _Mode(rec):
                yield tr
        finally:
            tr.recorder = None
    gc.collect()
    rec._poll()
    tr.before_push = tr.on_cross = None
    for sk, st in tr.storages.items():
        s = rec.keep.get(sk)
        if s is not None:
            st["owned"] = torch._C._storage_Use_Count(s._cdata) > rec.share
    tr.calls = dict(rec.calls)
    rec.keep.clear()
    rec.events.clear()
