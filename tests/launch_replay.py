"""Launch replay: every ``ops.NAME(...)`` call a real step makes is checked, with the operands the engine itself passed, against the
references the kernel tests use -- the PyTorch restatement of the same op (tests/emu_ops.py and its siblings) at the tolerance of the
kernel's own test, and the element-wise float64 bound (tests/fp64_ref.py, fp64_update_ref.py, fp64_noise_ref.py, fp64_guidance_ref.py,
attention_cases.py) wherever one exists.

``install(monkeypatch, ops_module, mode=...)`` wraps every launcher of ``climate2weather_amd.ops``.  Per call the wrapper
  1. synchronises and snapshots every tensor argument (also inside the ln / lnf / resn / loss dicts, the splitk / det / workspace scratch
     and the items of conv_wgrad_grouped).  The snapshot is taken per STORAGE: arguments that are views of one buffer stay views of one
     copy, at their offsets, so the same view shares one clone and nothing is ever un-aliased.  A WRITTEN argument whose byte range
     partially overlaps another argument's raises AliasError;
  2. runs the real launcher on the real arguments (the step goes on undisturbed);
  3. synchronises, runs the restatement on a second copy of the snapshot, and compares every declared output over its whole buffer:
     live elements at the kernel test's tolerance (or bit for bit where that test demands equal bits), everything else -- padding
     columns, padded weight rows, the tail of the buffer -- bit for bit; then the float64 bound on the pristine snapshot;
  4. requires every byte of every argument's storage outside the declared outputs to be what it was.

What the doubles do not take is translated here, never in emu_ops.py: packed weights are resolved to the plain matrix through the
``pack_conv_weights_batched`` calls the harness saw; the fused loss is the plain conv of the snapshot followed by the definition in
include/c2w_hip.h; scratch (splitk / det / workspace / delta_ws) is handed to the reference fresh and exempt from step 4; the
``*_noise`` launchers get the float64 Philox stream of tests/fp64_noise_ref.py as their noise tensor.

This proves kernel against reference AT THE ENGINE'S ARGUMENTS.  It does not prove that the engine passes the right arguments (that is
tests/test_engine_emulated.py and the oracle parities), nor anything about races between launches: the harness serialises
(the ordering between streams is tests/stream_audit.py's subject).
"""
from __future__ import annotations

import inspect
import os
from collections import Counter

import torch

import attention_cases as AB
import emu_det_ops
import emu_eval_ops
import emu_exact_ops
import emu_ops
import fp64_guidance_ref as G
import fp64_noise_ref as N
import fp64_ref as R
import fp64_update_ref as U
from climate2weather_amd import ops as _ops

F32, BF16, F16 = 0, 1, 2
TD = emu_ops.TD
TOL = {F32: 1e-4, BF16: 2e-2, F16: 4e-3}      # tests/test_gpu_kernels.py:23 (== test_gpu_bench_dispatch.py:31 for the 16-bit types)
TOL_W = {F32: 1e-4, BF16: 1e-2, F16: 2e-3}    # weight gradients: test_gpu_kernels.py:403 (fp32), test_gpu_bench_dispatch.py:32 (16-bit)
TOL_DM = 1e-2                                 # modulation gradients: test_gpu_kernels.py:349, test_gpu_bench_dispatch.py:149
TOL_STAT = 2e-3                               # kept 1/sigma and mean: test_gpu_bench_dispatch.py:784/787
TOL_SUM = 1e-4                                # loss sums: test_gpu_kernels.py:624
TOL_COLSUM = {F32: 1e-4, BF16: 2e-3, F16: 2e-3}  # test_gpu_kernels.py:578
TOL_UPDATE = 2e-6                             # AdamW / EMA under the loss scaler: test_gpu_kernels.py:713 (1e-6 without: :661)
TOL_SHADOW = {torch.bfloat16: 1e-2, torch.float16: 4e-3, torch.float32: 1e-6}  # test_gpu_kernels.py:663
SIGS = {n: inspect.signature(f) for n, f in vars(_ops).items() if inspect.isfunction(f) and not n.startswith("_")}

# The ONLY launchers that may go unchecked, with the reason.  Any other name without a reference is a failure.
HOST_QUERY_SUFFIXES = ("_supported", "_bytes", "_plan", "_dispatch", "_numel")  # pure host arithmetic: no kernel runs
UNCHECKED = {
    "knobs_reload": "re-reads the environment on the host",
    "new_workspace": "a torch allocation",
    "publish_scalar": "copies four bytes into pinned host memory; its consumer is HostRing.read_bits on the host",
    "pack_conv_weights_batched": "checked through its consumer: every packed operand is resolved to the plain matrix and the conv compared",
    "check": "the error-code helper imported from _lib",
}
SCRATCH = {"splitk", "det", "workspace", "scratch", "delta_ws"}  # contents undefined before and after (include/c2w_hip.h)
EQUAL = {"window_gather", "window_scatter", "window_gather_list", "window_cotangent_list", "upsample2", "cast_f32", "weight_transpose",
         "weight_transpose_batched"}  # their own tests demand equal bits


class AliasError(AssertionError):
    pass


class NoReference(AssertionError):
    pass


def is_host_query(name):
    return name.endswith(HOST_QUERY_SUFFIXES)


# ------------------------------------------------------------------------------------------------------------ argument trees

def leaves(v, path=()):
    if isinstance(v, torch.Tensor):
        yield path, v
    elif isinstance(v, dict):
        for k, x in v.items():
            yield from leaves(x, path + (k,))
    elif isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            yield from leaves(x, path + (i,))


def remap(v, fn, path=()):
    if isinstance(v, torch.Tensor):
        return fn(path, v)
    if isinstance(v, dict):
        return {k: remap(x, fn, path + (k,)) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(remap(x, fn, path + (i,)) for i, x in enumerate(v))
    return v


def at(tree, path):
    for k in path:
        tree = tree[k]
    return tree


def pstr(path):
    return ".".join(str(p) for p in path)


def _sbytes(t):
    """the whole storage of t as a uint8 tensor"""
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())


def _on(t, sbytes):
    """t's view (offset, shape, strides) on another storage of the same size"""
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(sbytes.untyped_storage(), t.storage_offset(), t.shape, t.stride())


def _span(t):
    """[lo, hi) byte addresses the view can touch"""
    if t.numel() == 0:
        return t.data_ptr(), t.data_ptr()
    ext = sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1
    return t.data_ptr(), t.data_ptr() + ext * t.element_size()


def _vkey(t):
    return (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype)


def rows(t, n, ld):
    return t.reshape(-1)[: n * ld].view(n, ld)


def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- what every launcher writes

def _conv_writes(a):
    w = [("y2",), ("ln", "dm"), ("lnf", "y"), ("lnf", "rstd"), ("lnf", "mean"), ("loss", "sum")]
    return w if a.get("no_y") else [("y",)] + w


WRITES = {
    "conv": _conv_writes,
    "conv_wgrad": [("dw",), ("dbias",)],
    "conv_wgrad_grouped": lambda a: [("items", i, j) for i in range(len(a["items"])) for j in (2, 3)],
    "ln_forward": [("y",)], "ln_backward": [("dx",), ("dm",)], "colsum": [("out",)], "silu": [("y",)], "silu_backward": [("dx",)],
    "sumpool2": [("dx",)], "upsample2": [("y",)], "nchw_to_nhwc": [("y",)], "nhwc_to_nchw": [("out",)],
    "mse_loss_grad": [("dy",), ("loss_sum",)], "philox_normal": [("out",)], "nchw_to_nhwc_noise": [("y",)],
    "nchw_to_nhwc_noise_rows": [("y",), ("erows",)], "windows_to_nhwc_noise": [("y",)], "mse_loss_grad_noise": [("dy",), ("loss_sum",)],
    "sq_err": [("out",), ("loss_sum",)], "sq_err_levels": [("table",), ("count",), ("per_image",)], "timestep_embedding": [("out",)],
    "mu_sigma": [("musig",)], "conv_center": [("out",)], "gemv_f32": [("y",)], "cast_f32": [("dst",)], "weight_transpose": [("out",)],
    "weight_transpose_batched": [("out",)], "adamw_ema": [("p",), ("m",), ("v",), ("ema",), ("shadow",)], "grad_scaler_init": [("state",)],
    "grad_scaler_check": [("state",)], "grad_scaler_update": [("state",)], "ema_update": [("ema",)], "attention_forward": [("o",), ("lse",)],
    "attention_backward": [("dqkv",)], "window_gather": [("y",)], "window_scatter": [("eps",)], "sampler_predict": [("x",), ("nan_flag",)],
    "sumsq": [("out",)], "sampler_correct": [("x",), ("nan_flag",)], "guidance": [("eps",)], "guidance_delta": [("delta",)],
    "window_gather_list": [("y",)], "window_cotangent_list": [("dy",)], "window_grad_fold_list": [("out",)], "pool_stride": [("y",)],
    "affine_channels": [("y",)], "pack_conv_weights_batched": [("dst",)],
}


def _conv_out_rows(a):
    g = a["g"]
    n = g["B"] * g["Hout"] * g["Wout"]
    return n // 4 if a.get("pool2") else n


def _taps(g):
    return 1 if g["mode"] == emu_ops.CONV_1X1 else 9


def live_regions(name, a):
    """{path: (rows, ld, C)}: the elements of a declared output the op defines.  Everything else in that buffer must keep its bits."""
    if name == "conv":
        g = a["g"]
        n, ld, C = _conv_out_rows(a), g["ldy"], g["Cout"]
        npix = g["B"] * g["Hout"] * g["Wout"]
        out = {("y",): (n, ld, C), ("y2",): (n, ld, C), ("lnf", "y"): (n, ld, C), ("lnf", "rstd"): (1, npix, npix), ("lnf", "mean"): (1, npix, npix),
               ("loss", "sum"): (1, 1, 1)}
        if a.get("loss") is not None:  # channels >= loss_C of the real rows: zero (c2w_hip.h), which the reference writes too
            out[("y",)] = (n, ld, ld)
        return out
    if name == "conv_wgrad":
        g = a["g"]
        k = g["Cout"] * _taps(g) * g["Cin"]
        return {("dw",): (1, k, k), ("dbias",): (1, g["Cout"], g["Cout"])}
    if name == "conv_wgrad_grouped":
        g = a["g"]
        k = g["Cout"] * _taps(g) * g["Cin"]
        out = {}
        for i in range(len(a["items"])):
            out[("items", i, 2)] = (1, k, k)
            out[("items", i, 3)] = (1, g["Cout"], g["Cout"])
        return out
    return {}


# ----------------------------------------------------------------------------------------------------------------- the report

class Report:
    def __init__(self, mode):
        self.mode = mode
        self.seen, self.checked, self.unchecked, self.refused = Counter(), Counter(), Counter(), Counter()
        self.worst = {}      # launcher name -> {bound name: worst ratio}
        self.families = {}   # kernel family of ops.conv_dispatch -> launches
        self.routes = Counter()  # attention routes
        self.flags = Counter()   # "conv:loss", "conv:wpacked", ... : the argument combinations seen
        self.failures = []   # (launch index, name, message)
        self.packed_resolved = 0
        self.calls = []      # (index, name, flags) of every launch
        self.bounded = Counter()  # launches per name that had a float64 bound
        self.bounded_flags = Counter()  # the same per "name:flag" (the argument combinations that were seen AND bounded)

    def ratio(self, name, what, r):
        d = self.worst.setdefault(name, {})
        d[what] = max(d.get(what, 0.0), float(r))

    def fail(self, index, name, msg):
        self.failures.append((index, name, msg))

    def assert_clean(self):
        assert not self.failures, "%d launches outside their references:\n%s" % (
            len(self.failures), "\n".join("  launch %d (%s): %s" % f for f in self.failures[:12]))
        extra = {n: c for n, c in self.unchecked.items() if n not in UNCHECKED and not is_host_query(n)}
        assert not extra, f"launchers without a reference: {extra}"
        for n, c in self.seen.items():
            assert self.checked[n] + self.refused[n] == c, f"{n}: {c} launches seen, {self.checked[n]} checked"

    def lines(self):
        out = []
        for n in sorted(self.seen):
            w = ", ".join(f"{k} {v:.3g}" for k, v in sorted(self.worst.get(n, {}).items()))
            out.append(f"{n}: {self.seen[n]} launches, {self.checked[n]} checked ({self.bounded[n]} with a float64 bound); worst ratio: {w}")
        out.append("conv families: " + ", ".join(f"{k}: {v}" for k, v in sorted(self.families.items())))
        out.append("attention routes: " + ", ".join(f"{k}: {v}" for k, v in sorted(self.routes.items())))
        return out


# ------------------------------------------------------------------------------------------------------------------- one call

class Call:
    def __init__(self, index, name, real, snap, ref):
        self.index, self.name, self.real, self.snap, self.ref = index, name, real, snap, ref
        self.flags = set()
        self.got = {}  # path -> tensor that stands for the real output in the comparison (the planted defects of the GPU power check)

    def out(self, path):
        return self.got.get(path, at(self.real, path))


class Harness:
    def __init__(self, monkeypatch, ops_module, mode, planted):
        self.ops, self.mode, self.planted = ops_module, mode, planted
        self.report = Report(mode)
        self.packed = {}  # address of a packed matrix -> (source tensor, source offset, rows, cin)
        self.n = 0
        self.refs = {}
        stack = [emu_ops] + {"default": [], "det": [emu_det_ops], "exact": [emu_exact_ops], "eval": [emu_eval_ops]}[mode]
        for mod in stack:
            for name, fn in vars(mod).items():
                if inspect.isfunction(fn) and not name.startswith("_") and name != "install":
                    self.refs[name] = fn
        for name in sorted(SIGS):
            fn = getattr(ops_module, name, None)
            if fn is None or not callable(fn):
                continue
            monkeypatch.setattr(ops_module, name, self._wrap(name, fn))

    def _wrap(self, name, fn):
        def launch(*a, **kw):
            return self.call(name, fn, a, kw)
        launch.__name__ = name
        launch.__wrapped__ = fn
        return launch

    # -- the wrapper ------------------------------------------------------------------------------------------------------
    def call(self, name, fn, a, kw):
        rep = self.report
        if name in UNCHECKED or is_host_query(name):
            rep.unchecked[name] += 1
            if name == "pack_conv_weights_batched":
                self._watch_pack(SIGS[name].bind(*a, **kw).arguments)
            return fn(*a, **kw)
        index = self.n
        self.n += 1
        rep.seen[name] += 1
        if name not in WRITES or (name not in self.refs and name not in TRANSLATE):
            rep.unchecked[name] += 1
            rep.fail(index, name, "a launcher without a reference")
            return fn(*a, **kw)
        ba = SIGS[name].bind(*a, **kw)
        ba.apply_defaults()
        real = dict(ba.arguments)
        _sync()
        written = WRITES[name](real) if callable(WRITES[name]) else WRITES[name]
        written = [p for p in written if _has(real, p)]
        scratch = [p for p, _ in leaves(real) if p[0] in SCRATCH]
        self._alias_rule(index, name, real, written + scratch)
        groups = {}  # storage address -> (bytes view, snapshot bytes)
        scr_only = {}
        for p, t in leaves(real):
            scr_only[t.untyped_storage().data_ptr()] = scr_only.get(t.untyped_storage().data_ptr(), True) and p[0] in SCRATCH
        for p, t in leaves(real):
            sp = t.untyped_storage().data_ptr()
            if sp not in groups and not scr_only[sp]:
                b = _sbytes(t)
                groups[sp] = (b, b.clone())
        ret = fn(*a, **kw)
        _sync()
        flags = self._flags(name, real)
        rep.calls.append((index, name, flags))
        for f in flags:
            rep.flags[f"{name}:{f}"] += 1
        refstore = {sp: snap.clone() for sp, (_, snap) in groups.items()}

        def view(store):
            def f(p, t):
                sp = t.untyped_storage().data_ptr()
                if scr_only[sp]:
                    return torch.empty_like(t) if store is refstore else t
                return _on(t, store[sp] if store is refstore else groups[sp][1])
            return f
        call = Call(index, name, real, remap(real, view(None)), remap(real, view(refstore)))
        call.flags = flags
        try:
            if ret is False:  # "unsupported": nothing may have been written at all
                rep.refused[name] += 1
                written = []
            else:
                call.snap, call.ref = self._translate(call, call.snap, True), self._translate(call, call.ref)
                if self.planted is not None:
                    self.planted(call)
                rep.checked[name] += 1  # a reference exists and is run; what it finds goes to rep.failures
                self._restatement(call, written)
                self._bounds(call)
            self._untouched(call, groups, written + scratch)
        except AliasError:
            raise
        except (AssertionError, NoReference) as e:
            rep.fail(index, name, f"{name} {sorted(flags)}: {e}")
        return ret

    def _flags(self, name, a):
        f = set()
        if name == "conv":
            g = a["g"]
            for k in ("ln", "lnf", "resn", "loss", "splitk", "det", "res", "mul", "y2", "bias"):
                if a.get(k) is not None:
                    f.add(k)
            for k in ("pool2", "wpacked", "no_y", "kvalid"):
                if a.get(k):
                    f.add(k)
            if a.get("ln") is not None and a["ln"].get("rstd") is not None:
                f.add("ln.rstd")
            if a.get("lnf") is not None:
                f.update("lnf." + k for k in ("rstd", "mean") if a["lnf"].get(k) is not None)
            if a.get("act") in (emu_ops.ACT_RELU, emu_ops.ACT_RELU_PAIR):
                f.add("relu" if a["act"] == emu_ops.ACT_RELU else "relu_pair")
            if g["ldy"] != g["Cout"]:
                f.add("ldy!=Cout")
            f.add("mode%d" % g["mode"])
            if not getattr(self.ops, "EMULATED", False):
                fam = self.ops.conv_dispatch.__wrapped__(g, a["dtype"], bool(a.get("pool2")), a.get("ln") is not None or a.get("lnf") is not None)
                self.report.families[fam] = self.report.families.get(fam, 0) + 1
                f.add("family%d" % fam)
        elif name in ("attention_forward", "attention_backward"):
            route = AB.attn_route(a["B"], a["T"], a["C"], a["dtype"], os.environ.get("C2W_ATTN_VALU") == "1")
            self.report.routes[route] += 1
            f.add(route)
        else:
            for k in ("det", "workspace", "scaler", "shadow", "img_off"):
                if a.get(k) is not None:
                    f.add(k)
            if a.get("deterministic"):
                f.add("deterministic")
            if "i0" in a and a["i0"]:
                f.add("i0!=0")
            if isinstance(a.get("eps"), int):
                f.add("seed")
            if isinstance(a.get("gamma"), torch.Tensor):
                f.add("gamma[F]")
        return f

    def _alias_rule(self, index, name, real, written):
        """a written argument's bytes -- the elements the op defines, where the engine hands over an open-ended view of a flat buffer
        (live_regions), else the whole view -- may not partially overlap another argument's"""
        live = live_regions(name, real)

        def span(p, t):
            lo, hi = _span(t)
            if p in live and t.is_contiguous():
                hi = min(hi, lo + live[p][0] * live[p][1] * t.element_size())
            return lo, hi
        lv = list(leaves(real))
        for p in written:
            t = at(real, p)
            lo, hi = span(p, t)
            for q, o in lv:
                if q == p or _vkey(o) == _vkey(t):
                    continue
                olo, ohi = span(q, o)
                if lo < ohi and olo < hi:
                    raise AliasError(f"launch {index} ({name}): written argument {pstr(p)} partially overlaps argument {pstr(q)} "
                                     f"([{lo:#x}, {hi:#x}) and [{olo:#x}, {ohi:#x}))")

    def _watch_pack(self, a):
        src, dst, desc, n, dtype = a["src"], a["dst"], a["desc"], a["n"], a["dtype"]
        for so, do, r, k in desc.reshape(-1, 4)[:n].tolist():
            self.packed[dst.data_ptr() + do * dst.element_size()] = (src, so, r, k)

    def _translate(self, call, a, count=False):
        a = dict(a)
        if call.name == "conv" and a.get("wpacked"):
            key = call.real["w"].data_ptr()
            if key not in self.packed:
                raise NoReference("a packed weight operand no pack_conv_weights_batched call of this run produced")
            src, so, r, k = self.packed[key]
            g = a["g"]
            assert r == g["wrows"] and k == g["Cin"], f"packed as ({r}, {k}), consumed as ({g['wrows']}, {g['Cin']})"
            a["w"] = src.reshape(-1)[so: so + r * 9 * k].clone()  # the plain [rows][taps][Cin] matrix the copy was made from
            a["wpacked"] = False
            self.report.packed_resolved += int(count)
        return a

    # -- restatement ------------------------------------------------------------------------------------------------------
    def _restatement(self, call, written):
        name, a = call.name, call.ref
        (TRANSLATE.get(name) or _plain)(self, call, a)
        live = live_regions(name, call.real)
        for p in written:
            got, ref, old = call.out(p), at(call.ref, p), at(call.snap, p)
            rule, tol = compare_rule(name, p, call.real, got)
            what = f"{pstr(p)} vs restatement"
            if got.dtype.is_floating_point and got.shape == ref.shape == old.shape:
                # NaNs that were in the buffer before the call and that neither side touched (the unwritten part of a torch.empty behind
                # an open-ended view): equal bits three times over, but NaN != NaN would fail every comparison below
                stale = torch.isnan(old) & _eq_bits(got, old) & _eq_bits(ref, old)
                if bool(stale.any()):
                    got, ref, old = (torch.where(stale, torch.zeros_like(t), t) for t in (got, ref, old))
            if rule == "equal" or not got.dtype.is_floating_point:
                assert torch.equal(got, ref), f"{what}: bits differ in {int((got != ref).sum())} of {got.numel()} elements"
                self.report.ratio(name, what, 0.0)
                continue
            gl, rl, ol = got, ref, old
            if p in live:
                n, ld, C = live[p]
                dead_g, dead_r = got.reshape(-1).clone(), ref.reshape(-1).clone()
                rows(dead_g, n, ld)[:, :C] = 0
                rows(dead_r, n, ld)[:, :C] = 0
                for q in written:  # another output inside this one's open-ended view (a bias gradient behind its weight gradient)
                    o = at(call.real, q)
                    if q != p and o.dtype == got.dtype and o.is_contiguous() and got.is_contiguous():
                        off = (o.data_ptr() - at(call.real, p).data_ptr()) // o.element_size()
                        if 0 <= off < dead_g.numel():
                            cnt = live[q][0] * live[q][1] if q in live else o.numel()
                            dead_g[off: off + cnt] = 0
                            dead_r[off: off + cnt] = 0
                assert _same_bits(dead_g, dead_r), f"{pstr(p)}: elements outside the {n} x {C} (stride {ld}) the op defines were written"
                gl, rl, ol = (rows(t, n, ld)[:, :C] for t in (got, ref, old))
            gl, rl, ol = gl.double(), rl.double(), ol.double().reshape(rl.shape)
            err = (gl - rl).abs().max().item() if gl.numel() else 0.0
            scale = (rl - ol if rule == "accumulate" else rl).abs().max().item() if rl.numel() else 0.0  # accumulate: of what the call adds
            bound = tol if rule == "abs" else tol * max(scale, 1e-6)
            r = err / bound if err == err else float("inf")
            self.report.ratio(name, what, r)
            assert r <= 1.0, f"{what}: max err {err:.3e} against {bound:.3e} (tolerance {tol:g})"

    # -- float64 bounds ---------------------------------------------------------------------------------------------------
    def _bounds(self, call):
        fn = BOUNDS.get(call.name)
        if fn is None:
            return
        n = 0
        for what, got, ref, layout in fn(self, call) or ():
            if getattr(self.ops, "EMULATED", False):  # a double is not held to the kernels' error model: the figure is recorded only
                worst = R.ratio(got, ref).max().item() if got.numel() else 0.0
            else:
                worst = R.assert_within(got, ref, what=what, layout=layout)
            self.report.ratio(call.name, "fp64 " + what.split(" ", 2)[2], worst)  # per op class: without "launch N"
            n += 1
        if n:
            self.report.bounded[call.name] += 1
            for f in call.flags:
                self.report.bounded_flags[f"{call.name}:{f}"] += 1

    def _untouched(self, call, groups, written):
        for sp, (now, snap) in groups.items():
            chk = now.clone()
            for p in written:
                t = at(call.real, p)
                if t.untyped_storage().data_ptr() == sp:
                    _on(t, chk).copy_(_on(t, snap))
            if not torch.equal(chk, snap):
                who = [pstr(p) for p, t in leaves(call.real) if t.untyped_storage().data_ptr() == sp]
                i = int((chk != snap).nonzero()[0])
                raise AssertionError(f"an argument the op does not write was written: byte {i} of the buffer of {who}")


def _has(tree, path):
    try:
        return isinstance(at(tree, path), torch.Tensor)
    except (KeyError, IndexError, TypeError):
        return False


_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _eq_bits(a, b):
    """element-wise: the same bits"""
    return a.contiguous().view(_INT[a.element_size()]) == b.contiguous().view(_INT[b.element_size()])


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def compare_rule(name, p, a, got):
    dt = a.get("dtype", F32)
    if name in EQUAL:
        return "equal", 0
    if name == "conv":
        if p == ("ln", "dm"):
            return "accumulate", TOL_DM
        if p in (("lnf", "rstd"), ("lnf", "mean")):
            return "close", TOL_STAT
        if p == ("loss", "sum"):
            return "accumulate", TOL_SUM
        return "close", TOL[dt]
    if name in ("conv_wgrad", "conv_wgrad_grouped"):
        return "accumulate", TOL_W[dt]
    if name == "ln_backward" and p == ("dm",):
        return "accumulate", TOL_W[dt]  # test_gpu_kernels.py:518
    if name == "colsum":
        return "accumulate", TOL_COLSUM[dt]
    if p == ("loss_sum",) or name == "sumsq":
        return "accumulate", TOL_SUM
    if name == "philox_normal":
        return "abs", N.STREAM_TOL
    if name in ("mu_sigma", "timestep_embedding"):
        return "close", 1e-6  # test_gpu_kernels.py:607/634
    if name in ("adamw_ema", "ema_update"):
        if p == ("shadow",):
            return "close", TOL_SHADOW[got.dtype]
        return "close", TOL_UPDATE if a.get("scaler") is not None else 1e-6
    if name.startswith("grad_scaler"):
        return "equal", 0  # powers of two and counters: exact in fp32 (fp64_update_ref.scaler_model)
    if name == "sq_err_levels":
        return "accumulate", TOL_SUM
    if name == "window_grad_fold_list":
        return "accumulate", TOL[F32]
    if "dtype" in a:
        return "close", TOL[dt]
    return "close", TOL[F32]  # the fp32-only kernels: the fp32 parity gate of test_gpu_kernels.py


# ------------------------------------------------------------------------------- running the restatement on the reference copy

def _call_ref(h, name, a):
    fn = h.refs.get(name)
    if fn is None:
        raise NoReference(f"no restatement of {name}")
    params = dict(inspect.signature(fn).parameters)
    if any(p.kind == p.VAR_KEYWORD for p in params.values()):  # a layered double that forwards **kw to emu_ops
        params.update(inspect.signature(getattr(emu_ops, name)).parameters)
    kw = {}
    for k, v in a.items():
        if k in params:
            kw[k] = v
        else:
            assert v is None or v is False, f"the restatement of {name} has no argument {k}"
    return fn(**kw)


def _plain(h, call, a):
    _call_ref(h, call.name, a)


def _t_conv(h, call, a):
    a = dict(a)
    if not _det_restated(h):
        a["det"] = None
    a["splitk"] = None  # another split of the same sum
    a["naive"] = False
    loss = a.get("loss")
    if loss is None:
        return _call_ref(h, "conv", a)
    # the fused loss (include/c2w_hip.h): a = the result rounded to the storage type; y = (a - eps) * gscale [* scaler[0]]; sum += sum (a - eps)^2
    g, T = a["g"], TD[a["dtype"]]
    npix, C = g["B"] * g["Hout"] * g["Wout"], loss["C"]
    pred = torch.zeros((npix, g["ldy"]), dtype=T, device=a["x"].device)
    _call_ref(h, "conv", dict(a, loss=None, det=None, y=pred))
    d = pred[:, :C].float() - rows(loss["eps"], npix, loss["lde"])[:, :C].float()
    gs = loss["gscale"] * (float(loss["scaler"].reshape(-1)[0]) if loss.get("scaler") is not None else 1.0)
    Y = rows(a["y"], npix, g["ldy"])
    Y[:] = 0
    Y[:, :C] = (d * gs).to(T)
    loss["sum"].reshape(-1)[0] += (d * d).sum()


def _eps_of(a, B, C, HW, device):
    return N.eps_nchw(B, C, HW, a["seed"] if "seed" in a else a["eps"], device).float()


def _gather(data, img_off, B, C, HW):
    flat = data.reshape(-1)
    return torch.stack([flat[o:o + C * HW] for o in img_off.tolist()]).view(B, C, HW)


def _t_nchw_noise(h, call, a):
    B, C, HW = a["B"], a["C"], a["HW"]
    x = a["x"] if "x" in a else a["data"]
    if a.get("img_off") is not None:
        x = _gather(x, a["img_off"], B, C, HW)
    eps = _eps_of(a, B, C, HW, x.device)
    if call.name == "nchw_to_nhwc_noise_rows":  # the noise rounded to half precision is what is mixed in and kept (c2w_hip.h)
        eh = eps.half()
        a["erows"].reshape(-1)[: B * HW * a["lde"]] = 0
        rows(a["erows"], B * HW, a["lde"])[:, :C] = eh.permute(0, 2, 1).reshape(B * HW, C)
        eps = eh.float()
    emu_ops.nchw_to_nhwc(x, eps, a["musig"], a["y"], B, C, HW, a["ldc"], a["dtype"])


def _t_mse_noise(h, call, a):
    eps = _eps_of(a, a["B"], a["C"], a["HW"], a["y"].device)
    a = {k: v for k, v in a.items() if k != "seed"}
    _call_ref(h, "mse_loss_grad", dict(a, eps=eps))


def _t_sq_err(h, call, a):
    if isinstance(a["eps"], int):
        a = dict(a, eps=_eps_of(a, a["B"], a["C"], a["HW"], a["y"].device))
    _call_ref(h, call.name, a)


def _t_philox(h, call, a):
    a["out"].reshape(-1)[: a["n"]] = torch.from_numpy(N.normal_stream(a["n"], a["seed"])).to(a["out"].device).float()


def _t_levels(h, call, a):
    """emu_eval_ops.sq_err_levels reads t through numpy: the device form of the same statement"""
    if isinstance(a["eps"], int):
        a = dict(a, eps=_eps_of(a, a["B"], a["C"], a["HW"], a["y"].device))
    B, C, HW, K = a["B"], a["C"], a["HW"], a["K"]
    Y = rows(a["y"], B * HW, a["ldc"])[:, :C].float().view(B, HW, C).permute(0, 2, 1)
    d = Y - a["eps"].reshape(-1)[: B * C * HW].view(B, C, HW).float()
    s = (d * d).sum(-1)
    bins = emu_eval_ops.level_bins_f32(a["t"].reshape(-1)[:B].cpu().numpy(), K)
    for b in range(B):
        a["table"][int(bins[b])] += s[b].double()
        a["count"][int(bins[b])] += 1
    if a.get("per_image") is not None:
        a["per_image"].reshape(-1)[:B] = s.sum(1)


def _det_restated(h):
    """emu_det_ops restates the scratch protocol with its OWN scratch sizes: it is the reference where it is also the launcher (the CPU
    tier); against the library the scratch is ignored -- another order of the same sum"""
    return h.mode == "det" and getattr(h.ops, "EMULATED", False)


def _t_nodet(h, call, a):
    if _det_restated(h):
        return _call_ref(h, call.name, a)
    a = dict(a)
    for k in ("det", "workspace"):
        if k in a:
            a[k] = None
    if "deterministic" in a:
        a["deterministic"] = False
    _call_ref(h, call.name, a)


TRANSLATE = {
    "conv": _t_conv, "nchw_to_nhwc_noise": _t_nchw_noise, "nchw_to_nhwc_noise_rows": _t_nchw_noise, "windows_to_nhwc_noise": _t_nchw_noise,
    "mse_loss_grad_noise": _t_mse_noise, "sq_err": _t_sq_err, "philox_normal": _t_philox, "sq_err_levels": _t_levels,
    "conv_wgrad": _t_nodet, "conv_wgrad_grouped": _t_nodet, "ln_backward": _t_nodet, "colsum": _t_nodet, "mse_loss_grad": _t_nodet,
}


# ------------------------------------------------------------------------------------------------------- the float64 bounds

def _dm_rows(dm, g_or_npix, HW, C, ldm):
    if ldm:
        return torch.as_strided(dm.reshape(-1), (g_or_npix // HW, C), (ldm, 1))
    return dm.reshape(-1)[:C].view(1, C)


def _b_conv(h, call):
    """every conv launch has its float64 bound: the chain form (resn / no_y / lnf.mean), kept statistics (ln.rstd) and both ReLU forms
    included; the ReLU pair's mask is held by its consistency with the bounded first output (fp64_ref.assert_mask_consistent)"""
    a = call.snap
    g, dt = a["g"], a["dtype"]
    T = R._T(dt)
    Cout, ldy = g["Cout"], g["ldy"]
    npix, HW = g["B"] * g["Hout"] * g["Wout"], g["Hout"] * g["Wout"]
    n_out = _conv_out_rows(a)
    pair = a["act"] in (emu_ops.ACT_SILU_PAIR, emu_ops.ACT_RELU_PAIR)
    kw = dict(bias=a["bias"], act=a["act"], res=a["res"], mul=a["mul"], mulmode=a["mulmode"], y2=a["y2"] is not None and not pair,
              pool2=bool(a["pool2"]), kvalid=int(a["kvalid"] or 0), resn=a.get("resn"), no_y=bool(a.get("no_y")))
    if a["lnf"] is not None:
        kw["lnf"] = a["lnf"]
    if a["ln"] is not None:
        kw["ln"] = a["ln"]
    ref = R.conv(a["x"], a["w"], g, dt, **kw)
    lay = R.layout(g) if not a["pool2"] else dict(B=g["B"], H=g["Hout"] // 2, W=g["Wout"] // 2, C=Cout, tile=(4, 8))
    tag = f"launch {call.index} conv"
    y = rows(call.out(("y",)), n_out, ldy)
    loss = a.get("loss")
    if a.get("no_y"):
        assert "y" not in ref  # nothing to bound: that the buffer kept its bytes is the harness's step 4
    elif loss is None:
        yield f"{tag} y", y[:, :Cout], ref["y"], lay
        if a["act"] == emu_ops.ACT_RELU_PAIR:
            R.assert_mask_consistent(y[:, :Cout], rows(call.out(("y2",)), n_out, ldy)[:, :Cout], what=f"{tag} y2")
            h.report.ratio("conv", "fp64 conv relu mask", 0.0)
    else:
        C, lde = loss["C"], loss["lde"]
        pred = R.V(ref["y"].v[:, :C], ref["y"].e[:, :C])
        d = R._sub(pred, R.exact(rows(loss["eps"], npix, lde)[:, :C]))
        gs = U.f32(loss["gscale"]) * (float(loss["scaler"].reshape(-1)[0]) if loss.get("scaler") is not None else 1.0)
        yield f"{tag} fused dy", y[:, :C], R._rnd(R._scale(d, gs), T), dict(R.layout(g), C=C)
        wg = g["B"] * -(-g["Hout"] // 16) * -(-g["Wout"] // 16)
        s = R.fused_loss_sum(pred.v, loss["eps"], C, lde, npix, wg)
        s = R.V(s.v, s.e + (2 * d.v.abs() * d.e + d.e * d.e).sum() * (1 + 2 * R.U32))  # the stored prediction is within pred.e of pred.v
        yield f"{tag} fused loss sum", call.out(("loss", "sum")).reshape(-1)[:1], R.accumulated(loss["sum"].reshape(-1)[:1], R.V(s.v.reshape(1), s.e.reshape(1))), None
    if "y2" in ref:
        yield f"{tag} y2", rows(call.out(("y2",)), n_out, ldy)[:, :Cout], ref["y2"], lay
    if "hn" in ref:
        yield f"{tag} lnf.y", rows(call.out(("lnf", "y")), npix, ldy)[:, :Cout], ref["hn"], lay
        if a["lnf"].get("rstd") is not None:
            yield f"{tag} lnf.rstd", call.out(("lnf", "rstd")).reshape(-1)[:npix], ref["rstd"], None
        if a["lnf"].get("mean") is not None:
            yield f"{tag} lnf.mean", call.out(("lnf", "mean")).reshape(-1)[:npix], ref["mean"], None
    if "dm" in ref and a["ln"].get("dm") is not None:
        ldm = a["ln"].get("ldm", 0)
        yield f"{tag} ln.dm", _dm_rows(call.out(("ln", "dm")), npix, HW, Cout, ldm), R.accumulated(_dm_rows(a["ln"]["dm"], npix, HW, Cout, ldm), ref["dm"]), None


def _b_wgrad_item(tag, x, dy, dw_old, db_old, dw_got, db_got, g):
    k = g["Cout"] * _taps(g) * g["Cin"]
    dw, db = R.wgrad(x, dy, g)
    yield f"{tag} dw", dw_got.reshape(-1)[:k].view(g["Cout"], -1), R.accumulated(dw_old.reshape(-1)[:k].view(g["Cout"], -1), dw), None
    if db_got is not None:
        yield f"{tag} dbias", db_got.reshape(-1)[: g["Cout"]], R.accumulated(db_old.reshape(-1)[: g["Cout"]], db), None


def _b_wgrad(h, call):
    a = call.snap
    yield from _b_wgrad_item(f"launch {call.index} conv_wgrad", a["x"], a["dy"], a["dw"], a["dbias"], call.out(("dw",)),
                             call.out(("dbias",)) if a["dbias"] is not None else None, a["g"])


def _b_wgrad_grouped(h, call):
    a = call.snap
    for i, (x, dy, dw, db) in enumerate(a["items"]):
        yield from _b_wgrad_item(f"launch {call.index} conv_wgrad_grouped item {i}", x, dy, dw, db, call.out(("items", i, 2)),
                                 call.out(("items", i, 3)) if db is not None else None, a["g"])


def _b_ln_forward(h, call):
    a = call.snap
    y, _ = R.ln_forward(a["x"], a["m"], a["npix"], a["HW"], a["C"], a["ldm"], a["eps"], a["unbiased"], a["dtype"])
    yield f"launch {call.index} ln_forward", rows(call.out(("y",)), a["npix"], a["C"]), y, None


def _b_ln_backward(h, call):
    a = call.snap
    dx, dm = R.ln_backward(a["dy"], a["x"], a["m"], a["dres"], a["npix"], a["HW"], a["C"], a["ldm"], a["eps"], a["unbiased"], a["dtype"])
    yield f"launch {call.index} ln_backward dx", rows(call.out(("dx",)), a["npix"], a["C"]), dx, None
    if a["dm"] is not None:
        yield (f"launch {call.index} ln_backward dm", _dm_rows(call.out(("dm",)), a["npix"], a["HW"], a["C"], a["ldm"]),
               R.accumulated(_dm_rows(a["dm"], a["npix"], a["HW"], a["C"], a["ldm"]), dm), None)


def _b_colsum(h, call):
    a = call.snap
    yield (f"launch {call.index} colsum", call.out(("out",)).reshape(-1)[: a["C"]],
           R.accumulated(a["out"].reshape(-1)[: a["C"]], R.colsum(a["a"], a["rows"], a["C"], a["lda"], a["dtype"])), None)


def _b_sumsq(h, call):
    a = call.snap
    s = R.sumsq(a["v"], a["n"])
    yield f"launch {call.index} sumsq", call.out(("out",)).reshape(-1)[:1], R.accumulated(a["out"].reshape(-1)[:1], R.V(s.v.reshape(1), s.e.reshape(1))), None


def _gs(a):
    return U.f32(a["gscale"]) * (float(a["scaler"].reshape(-1)[0]) if a.get("scaler") is not None else 1.0)


def _one(v):
    return R.V(v.v.reshape(1), v.e.reshape(1))


def _b_mse(h, call):
    a = call.snap
    B, C, HW, ldc = a["B"], a["C"], a["HW"], a["ldc"]
    yield f"launch {call.index} mse dy", rows(call.out(("dy",)), B * HW, ldc), R.mse_dy(a["y"], a["eps"], B, C, HW, ldc, _gs(a), a["dtype"]), None
    yield (f"launch {call.index} mse loss sum", call.out(("loss_sum",)).reshape(-1)[:1],
           R.accumulated(a["loss_sum"].reshape(-1)[:1], _one(R.mse_loss_sum(a["y"], a["eps"], B, C, HW, ldc))), None)


def _stream_sum(y, eps, B, C, HW, ldc, tol):
    """tests/test_gpu_noise_stream.py::_loss_sum_bound"""
    s = R.mse_loss_sum(y, eps, B, C, HW, ldc)
    d = (R._rows(y, B * HW, ldc)[:, :C].to(R.D) - N._to_rows(eps)).abs()
    return _one(R.V(s.v, s.e + (2 * d * tol + tol * tol).sum() * (1 + 2 * R.U32)))


def _b_mse_noise(h, call):
    a = call.snap
    B, C, HW, ldc = a["B"], a["C"], a["HW"], a["ldc"]
    eps = N.eps_nchw(B, C, HW, a["seed"], a["y"].device)
    yield (f"launch {call.index} mse_loss_grad_noise dy", rows(call.out(("dy",)), B * HW, ldc)[:, :C],
           N.mse_dy_rows(a["y"], eps, B, C, HW, ldc, _gs(a), a["dtype"], N.STREAM_TOL), None)
    yield (f"launch {call.index} mse_loss_grad_noise loss sum", call.out(("loss_sum",)).reshape(-1)[:1],
           R.accumulated(a["loss_sum"].reshape(-1)[:1], _stream_sum(a["y"], eps, B, C, HW, ldc, N.STREAM_TOL)), None)


def _b_sq_err(h, call):
    a = call.snap
    B, C, HW, ldc = a["B"], a["C"], a["HW"], a["ldc"]
    seeded = isinstance(a["eps"], int)
    eps = N.eps_nchw(B, C, HW, a["eps"], a["y"].device) if seeded else a["eps"].reshape(B, C, HW)
    tol = N.STREAM_TOL if seeded else 0.0
    yield f"launch {call.index} sq_err out", call.out(("out",)).reshape(-1)[: B * C * HW].view(B, C, HW), N.sq_err_planes(a["y"], eps, B, C, HW, ldc, tol), None
    if a["loss_sum"] is not None:
        s = _stream_sum(a["y"], eps, B, C, HW, ldc, tol) if seeded else _one(R.sq_err_sum(a["y"], eps, B, C, HW, ldc))
        yield f"launch {call.index} sq_err loss sum", call.out(("loss_sum",)).reshape(-1)[:1], R.accumulated(a["loss_sum"].reshape(-1)[:1], s), None


def _b_nchw_noise(h, call):
    a = call.snap
    B, C, HW = a["B"], a["C"], a["HW"]
    x = a["x"] if "x" in a else a["data"]
    if a.get("img_off") is not None:
        x = _gather(x, a["img_off"], B, C, HW)
    x = x.reshape(-1)[: B * C * HW].view(B, C, HW)
    eps = N.eps_nchw(B, C, HW, a["seed"], x.device)
    tol = N.STREAM_TOL
    if call.name == "nchw_to_nhwc_noise_rows":  # the kept rows ARE the noise: the mix is bounded from them, they from the stream
        er = rows(call.out(("erows",)), B * HW, a["lde"])[:, :C]
        e16 = R._rnd(R.V(N._to_rows(eps), torch.full((B * HW, C), N.STREAM_TOL, dtype=R.D, device=x.device)), torch.float16)
        yield f"launch {call.index} kept noise rows", er, e16, None
        eps, tol = er.to(R.D).view(B, HW, C).permute(0, 2, 1), 0.0
    yield (f"launch {call.index} {call.name}", rows(call.out(("y",)), B * HW, a["ldc"])[:, :C],
           N.xt_rows(x, eps, a["musig"].reshape(-1)[: 2 * B].view(B, 2), a["dtype"], tol), None)


def _b_nchw(h, call):
    a = call.snap
    if a["eps"] is None:
        return
    B, C, HW = a["B"], a["C"], a["HW"]
    x = a["x"].reshape(-1)[: B * C * HW].view(B, C, HW)
    yield (f"launch {call.index} nchw_to_nhwc", rows(call.out(("y",)), B * HW, a["ldc"])[:, :C],
           N.xt_rows(x, a["eps"].reshape(-1)[: B * C * HW].view(B, C, HW), a["musig"].reshape(-1)[: 2 * B].view(B, 2), a["dtype"]), None)


def _b_attn_fwd(h, call):
    a = call.snap
    B, T, C, dt = a["B"], a["T"], a["C"], a["dtype"]
    route = AB.attn_route(B, T, C, dt, os.environ.get("C2W_ATTN_VALU") == "1")
    ro, rl = R.attention_forward(a["qkv"], B, T, C, dt, route)
    yield f"launch {call.index} attention_forward ({route}) o", rows(call.out(("o",)), B * T, C), ro, R.attn_layout(B, T, C, "o")
    if a["lse"] is not None:
        yield f"launch {call.index} attention_forward ({route}) lse", call.out(("lse",)).reshape(-1)[: B * T], rl, R.attn_layout(B, T, C, ())


def _b_attn_bwd(h, call):
    a = call.snap
    B, T, C, dt = a["B"], a["T"], a["C"], a["dtype"]
    route = AB.attn_route(B, T, C, dt, os.environ.get("C2W_ATTN_VALU") == "1")
    rg = R.attention_backward(a["qkv"], a["o"], a["d_o"], a["lse"], B, T, C, dt, route)
    dq = rows(call.out(("dqkv",)), B * T, 3 * C)
    for s, i in AB.SECTION.items():
        yield f"launch {call.index} attention_backward ({route}) d{s}", dq[:, i * C:(i + 1) * C], AB.sect(rg, s, C), R.attn_layout(B, T, C, s)


def _b_adamw(h, call):
    a = call.snap
    n = a["n"]
    hyper = dict(lr=a["lr"], beta1=a["beta1"], beta2=a["beta2"], eps=a["eps"], wd=a["weight_decay"], ema_rate=a["ema_rate"])
    f = lambda t: None if t is None else t.reshape(-1)[:n]  # noqa: E731
    st = a["scaler"].reshape(-1)[:4].tolist() if a.get("scaler") is not None else None
    sh = a.get("shadow")
    pn, mi, vi, e2, s2 = U.adamw_step(f(a["p"]), f(a["g"]), f(a["m"]), f(a["v"]), f(a["ema"]), hyper, a["step"], a["grad_scale"], scaler_state=st,
                                      shadow_dtype=None if sh is None else sh.dtype, shadow_prev=f(sh))
    tag = f"launch {call.index} adamw_ema"
    for k, ref in (("p", pn), ("m", mi), ("v", vi), ("ema", e2), ("shadow", s2)):
        if ref is not None and a.get(k) is not None:
            yield f"{tag} {k}", call.out((k,)).reshape(-1)[:n], ref, None


def _b_ema(h, call):
    a = call.snap
    n = a["n"]
    yield f"launch {call.index} ema_update", call.out(("ema",)).reshape(-1)[:n], U.ema_step(a["ema"].reshape(-1)[:n], a["p"].reshape(-1)[:n], a["rate"]), None


def _b_temb(h, call):
    a = call.snap
    n, dim = a["n"], a["dim"]
    yield (f"launch {call.index} timestep_embedding", call.out(("out",)).reshape(-1)[: n * dim].view(n, dim),
           U.timestep_embedding(a["t"].reshape(-1)[:n], dim, a["max_period"]), None)


def _b_mu_sigma(h, call):
    a = call.snap
    n = a["n"]
    mu, sg = U.mu_sigma(a["t"].reshape(-1)[:n], a["eta"])
    ms = call.out(("musig",)).reshape(-1)[: 2 * n].view(n, 2)
    yield f"launch {call.index} mu", ms[:, 0], mu, None
    yield f"launch {call.index} sigma", ms[:, 1], sg, None


def _b_gemv(h, call):
    a = call.snap
    yield f"launch {call.index} gemv_f32", call.out(("y",)).reshape(-1)[: a["rows"]], U.gemv(a["x"], a["W"], a["bias"], a["rows"], a["K"], a["ldk"], a["act"]), None


def _b_predict(h, call):
    a = call.snap
    n = a["n"]
    yield f"launch {call.index} sampler_predict", call.out(("x",)).reshape(-1)[:n], U.predict(a["x"].reshape(-1)[:n], a["eps"].reshape(-1)[:n], a["a"], a["b"]), None


def _b_correct(h, call):
    a = call.snap
    n = a["n"]
    yield (f"launch {call.index} sampler_correct", call.out(("x",)).reshape(-1)[:n],
           U.correct(a["x"].reshape(-1)[:n], a["eps"].reshape(-1)[:n], a["z"].reshape(-1)[:n], a["sumsq_buf"], n, a["tau"], a["sigma_next"]), None)


def _b_silu(h, call):
    a = call.snap
    n = a["n"]
    yield f"launch {call.index} silu", call.out(("y",)).reshape(-1)[:n], U.silu(a["x"].reshape(-1)[:n], a["dtype"]), None


def _b_silu_bwd(h, call):
    a = call.snap
    n = a["n"]
    yield f"launch {call.index} silu_backward", call.out(("dx",)).reshape(-1)[:n], U.silu_backward(a["x"].reshape(-1)[:n], a["dy"].reshape(-1)[:n], a["dtype"]), None


def _b_sumpool2(h, call):
    a = call.snap
    B, H, W, C = a["B"], a["H"], a["W"], a["C"]
    yield f"launch {call.index} sumpool2", rows(call.out(("dx",)), B * H * W, C), U.sumpool2(a["g"], B, H, W, C, a["dtype"]), None


def _gam(a, F, like):
    g = a["gamma"]
    return g.reshape(-1)[:F] if isinstance(g, torch.Tensor) else torch.full((F,), U.f32(g), device=like.device)


def _b_guidance(h, call):
    a = call.snap
    F, H, W, nobs = a["F"], a["H"], a["W"], a["nobs"]
    want, spread = G.guided_eps(a["x"], a["eps"], a["yobs"], a["stdv"], _gam(a, F, a["x"]), nobs, F, H, W, a["s_step"], a["t_step"], U.f32(a["mu"]), U.f32(a["sigma"]))
    if call.name == "guidance":
        yield f"launch {call.index} guidance", call.out(("eps",)).reshape(-1)[: want.v.numel()].view(want.v.shape), want, None
    else:
        yield f"launch {call.index} guidance_delta", call.out(("delta",)).reshape(-1)[: spread.v.numel()].view(spread.v.shape), R.V(-spread.v, spread.e), None


def _b_pool_stride(h, call):
    a = call.snap
    F, H, W, nobs, s, t = a["F"], a["H"], a["W"], a["nobs"], a["s_step"], a["t_step"]
    L = a["x"].numel() // (F * H * W)
    X = a["x"].reshape(-1)[: L * F * H * W].view(L, F, H, W)
    tot = R._sum(R.exact(G._cells(X[::t][:nobs], s)), -1, chain=G._chain(s))
    ref = G._div(tot, float(s * s))
    yield f"launch {call.index} pool_stride", call.out(("y",)).reshape(-1)[: ref.v.numel()].view(ref.v.shape), ref, None


def _b_philox(h, call):
    a = call.snap
    n = a["n"]
    ref = torch.from_numpy(N.normal_stream(n, a["seed"])).to(a["out"].device)
    yield f"launch {call.index} philox_normal", call.out(("out",)).reshape(-1)[:n], R.V(ref, torch.full_like(ref, N.STREAM_TOL)), None


BOUNDS = {
    "conv": _b_conv, "conv_wgrad": _b_wgrad, "conv_wgrad_grouped": _b_wgrad_grouped, "ln_forward": _b_ln_forward, "ln_backward": _b_ln_backward,
    "colsum": _b_colsum, "sumsq": _b_sumsq, "mse_loss_grad": _b_mse, "mse_loss_grad_noise": _b_mse_noise, "sq_err": _b_sq_err,
    "nchw_to_nhwc_noise": _b_nchw_noise, "nchw_to_nhwc_noise_rows": _b_nchw_noise, "windows_to_nhwc_noise": _b_nchw_noise, "nchw_to_nhwc": _b_nchw,
    "attention_forward": _b_attn_fwd, "attention_backward": _b_attn_bwd, "adamw_ema": _b_adamw, "ema_update": _b_ema, "timestep_embedding": _b_temb,
    "mu_sigma": _b_mu_sigma, "gemv_f32": _b_gemv, "sampler_predict": _b_predict, "sampler_correct": _b_correct, "silu": _b_silu,
    "silu_backward": _b_silu_bwd, "sumpool2": _b_sumpool2, "guidance": _b_guidance, "guidance_delta": _b_guidance, "pool_stride": _b_pool_stride,
    "philox_normal": _b_philox,
}


def install(monkeypatch, ops_module, *, mode="default", planted=None) -> Report:
    """Wrap every launcher of ``ops_module``; ``mode``: which doubles restate the launchers ("default": emu_ops; "det": emu_det_ops over it;
    "exact": emu_exact_ops; "eval": emu_eval_ops).  ``planted(call)``: called after the real launcher ran and before the comparison, with
    the Call (name, index, real / snap / ref argument trees); it may alter the real tensors (CPU defects) or put a stand-in for an
    output into ``call.got[path]`` (the power checks on a device, which leave the step alone).  Returns the Report that fills as the step runs."""
    return Harness(monkeypatch, ops_module, mode, planted).report


def border_tap_defect(select=None):
    """The power check of the GPU cases: on the first conv launch that is linear in the conv sum (bias / res only, 3x3) --
    or the launch ``select(call)`` accepts -- one border tap of input channel 0 of image 0 is removed from the compared output
    (fp64_ref.conv_term, as tests/test_gpu_kernels.py does).  Returns (hook, hit): hit[0] is that launch's index once it ran."""
    hit = []

    def hook(call):
        a = call.snap
        if hit or call.name != "conv":
            return
        g = a["g"]
        ok = (a["act"] == emu_ops.ACT_NONE and a["mul"] is None and a["y2"] is None and a["ln"] is None and a["lnf"] is None
              and not a["pool2"] and a["loss"] is None and g["mode"] == emu_ops.CONV_S1 and g["Hout"] >= 4)
        if select is not None:
            ok = ok and select(call)
        if not ok:
            return
        hit.append(call.index)
        t = R.conv_term(a["x"], a["w"], g, 0, slice(0, 1), 4, R.border_mask(g["Hout"], g["Wout"]))
        y = at(call.real, ("y",)).clone()
        yr = rows(y, g["B"] * g["Hout"] * g["Wout"], g["ldy"])
        yr[:, : g["Cout"]] = (yr[:, : g["Cout"]].double() - t).to(y.dtype)
        call.got[("y",)] = y
    return hook, hit
