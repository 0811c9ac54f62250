"""Host-side engine: lays the ScoreUNet parameters out for the HIP kernels and sequences the launches of one
forward (and, for training / exact guidance, the hand-written backward) of the reference's hot path

    ScoreUNet.forward  (model/score.py:59-70)  ->  UNet.forward  (model/nn.py:220-242)
    ModResidualBlock   (model/nn.py:27-28)         AttentionBlock (model/nn.py:49-59)

Data layout in HBM
  * parameters: ONE flat fp32 buffer; every nn.Parameter is a strided view into it.  Conv2d weights are stored
    [Cout][kh][kw][Cin] (a channels_last view of the reference's OIHW tensor) which is exactly the K-contiguous
    operand the implicit GEMM wants; the 30 modulation Linears sit back to back so that one GEMM produces every
    block's modulation vector.  The 16-bit modes (bf16, fp16) keep a shadow of the same buffer in their format (same offsets).
  * gradients: one flat fp32 buffer with the same offsets (a single RCCL all-reduce covers all 228 tensors).
  * activations: NHWC rows [B*H*W][C] in the compute dtype (fp32 or bf16); the reference's NCHW fp32 tensors only
    exist at the module boundary.
Everything runs on torch's current stream; torch is the allocator, nothing else.
"""
from __future__ import annotations

import os

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import torch

from . import ops
from .forward import LN_EPS, ForwardPass
from .nn import BlockSpec, LevelSpec
from .ops import (ACT_NONE, ACT_RELU, ACT_RELU_PAIR, ACT_SILU, ACT_SILU_PAIR, CONV_1X1, CONV_S1, CONV_S2, CONV_TS2, CONV_UP, DTYPE_BF16, DTYPE_F16, DTYPE_F32, MUL_DSILU, MUL_PLAIN, TORCH_DTYPE)

import weakref

_ENGINE_BY_PARAM_ID: Dict[int, "weakref.ReferenceType"] = {}  # id(Parameter) -> weakref(Engine); nothing is stored ON the Parameter (they are pickled / deep-copied)


def engine_of_parameter(p):
    """The Engine whose flat buffer the Parameter OBJECT ``p`` is bound to, or None (optim.AdamW finds its engine through this).
    An engine keeps its Parameters alive, so an id cannot be recycled while its entry is valid; the identity check covers the rest."""
    ref = _ENGINE_BY_PARAM_ID.get(id(p))
    eng = ref() if ref is not None else None
    if eng is None:
        _ENGINE_BY_PARAM_ID.pop(id(p), None)
        return None
    return eng if eng._bound_by_id.get(id(p)) is p else None


ALIGN = 64  # elements; keeps every region 256-B aligned in fp32 and 128-B aligned in the bf16 shadow


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


@dataclass
class ConvRec:
    """One weight matrix [rows][taps][cin] (+ bias[rows]) inside the flat buffer -- dense, so that every Parameter is a
    non-overlapping dense view (optimizers, DDP bucket views and the autograd layout contract all assume that)."""
    name: str
    rows: int  # Cout
    cin: int  # real input channels
    kstride: int  # channel stride of the forward operand (>= cin, padded for the network input)
    taps: int
    w_off: int = 0
    b_off: int = 0
    lin: bool = False  # fp32-only GEMM (time MLP, modulation projections)
    dg_ld: int = 0  # K stride of the input-gradient operand = channel stride of this layer's output rows
    dg_off: int = -1  # offset inside the dgrad weight buffer (-1: not needed)
    flip: bool = False


class Layout:
    """Flat parameter layout derived from the module tree."""

    def __init__(self, net):
        unet = net.unet
        self.levels: List[LevelSpec] = unet.spec()
        self.E = unet.mod_features
        self.in_channels, self.out_channels = unet.in_channels, unet.out_channels
        self.cin_pad = _round_up(unet.in_channels, 64)
        self.cout_pad = _round_up(unet.out_channels, 64)
        self.noise_features = net.noise_features
        self.activation = getattr(unet, "activation_kind", "silu")  # of the residual blocks (model/nn.py:156); the time MLP is always SiLU
        self.convs: Dict[str, ConvRec] = {}
        self.views: Dict[str, Tuple[int, Tuple[int, ...], Tuple[int, ...]]] = {}  # param name -> (offset, shape, strides)
        off = 0
        self._off = 0
        # Flat order = reverse of the order in which backward finalises gradients (time MLP last, output conv first), so
        # the finished part of the gradient buffer is always a growing suffix -> bucketed all-reduce can chase it.
        self.forcing_dim = net.map_forcing.in_features if getattr(net, "map_forcing", None) is not None else 0
        if self.forcing_dim:  # model/score.py:49-51; its gradient is final together with map_layer1's: same place in the flat order
            self._add("map_forcing", self.E, self.forcing_dim, 1, kstride=_round_up(self.forcing_dim, 32), lin=True)
        self._add("map_layer0", self.E, self.noise_features, 1, lin=True)
        self._add("map_layer1", self.E, self.E, 1, lin=True)
        off = self._off
        # modulation projections, back to back in execution order:  Wp_all [sumC][E], bp_all [sumC]
        blocks: List[BlockSpec] = []
        for lv in self.levels:
            blocks += [b for b in lv.descent if b.kind == "res"]
        for lv in reversed(self.levels):
            blocks += [b for b in lv.ascent if b.kind == "res"]
        mo = 0
        for b in blocks:
            b.mod_offset = mo
            mo += b.channels
        self.sum_c = mo
        self.proj_w_off = off
        for b in blocks:
            self.views[f"unet.{b.key}.project.0.weight"] = (off, (b.channels, self.E), (self.E, 1))
            off += b.channels * self.E
        off = _round_up(off, ALIGN)
        self.proj_b_off = off
        for b in blocks:
            self.views[f"unet.{b.key}.project.0.bias"] = (off, (b.channels,), (1,))
            off += b.channels
        off = _round_up(off, ALIGN)
        self.convs["proj"] = ConvRec("proj", self.sum_c, self.E, self.E, 1, self.proj_w_off, self.proj_b_off, lin=True, dg_ld=self.sum_c)

        self._off = off
        add = self._add

        L = len(self.levels)
        for i, lv in enumerate(self.levels):
            if i == 0:
                add("unet." + lv.head_key, lv.channels, self.in_channels, 9, kstride=self.cin_pad, dg_ld=lv.channels, flip=True)
            else:
                add("unet." + lv.head_key, lv.channels, self.levels[i - 1].channels, 9, flip=False)
            for b in lv.descent:
                self._add_block(add, b)
        for i in reversed(range(L)):
            lv = self.levels[i]
            for b in lv.ascent:
                self._add_block(add, b)
            if i > 0:
                add("unet." + lv.tail_key, self.levels[i - 1].channels, lv.channels, 9, flip=True)
            else:
                add("unet." + lv.tail_key, self.out_channels, lv.channels, 9, dg_ld=self.cout_pad, flip=True)
        self.numel = self._off
        # dgrad operand buffers: [cin][taps][dg_ld]
        dg = 0
        dgl = 0
        for rec in self.convs.values():
            if rec.name in ("map_layer0", "map_forcing"):
                continue
            size = _round_up(rec.cin * rec.taps * rec.dg_ld, ALIGN)
            if rec.lin:
                rec.dg_off = dgl
                dgl += size
            else:
                rec.dg_off = dg
                dg += size
        self.dg_numel, self.dg_lin_numel = dg, dgl

    def _add(self, name: str, rows: int, cin: int, taps: int, kstride: Optional[int] = None, lin=False, dg_ld=None, flip=False, ndim=4):
        off = self._off
        rec = ConvRec(name, rows, cin, kstride or cin, taps, lin=lin, dg_ld=dg_ld if dg_ld is not None else rows, flip=flip)
        rec.w_off = off
        ks = cin  # storage is dense; a layer whose operand stride differs (kstride > cin) reads a padded copy (Engine._w)
        if taps == 9:
            self.views[name + ".weight"] = (off, (rows, cin, 3, 3), (9 * ks, 1, 3 * ks, ks))
        elif ndim == 3:
            self.views[name + ".weight"] = (off, (rows, cin, 1), (ks, 1, 1))
        else:
            self.views[name + ".weight"] = (off, (rows, cin), (ks, 1))
        off = _round_up(off + rows * taps * ks, ALIGN)
        rec.b_off = off
        self.views[name + ".bias"] = (off, (rows,), (1,))
        self._off = _round_up(off + rows, ALIGN)
        self.convs[name] = rec
        return rec

    @staticmethod
    def _add_block(add, b: BlockSpec):
        p = "unet." + b.key
        if b.kind == "res":
            add(p + ".residue.1", b.channels, b.channels, 9, flip=True)
            add(p + ".residue.3", b.channels, b.channels, 9, flip=True)
        else:
            add(p + ".qkv", 3 * b.channels, b.channels, 1, ndim=3)
            add(p + ".proj_out", b.channels, b.channels, 1, ndim=3)


class Tape:
    """Backward closures recorded by a training forward (applied in reverse)."""

    def __init__(self):
        self.steps: List[Callable] = []
        self.gskip: Dict[int, torch.Tensor] = {}
        self.meta: dict = {}
        # called with the lowest flat offset whose gradient is final AND whose weights the rest of this backward no longer reads from
        # the flat parameter buffer (input-gradient operands are copies made before): the trainer may all-reduce and UPDATE that suffix
        self.progress: Optional[Callable[[int], None]] = None

    def done(self, off: int) -> None:
        if self.progress is not None:
            self.progress(off)


class Engine:
    LINEAR_DGRAD_SPLIT_MIN_ROWS = 2048  # Linear layers at least this wide take the split-reduction input-gradient route
    # switches that are class attributes (the others are set per engine in __init__); tests set them on the class or an engine
    use_center_conv = True  # the sampler's output conv computes the kept centre-frame rows only (c2w_conv_center) instead of all w * F channels
    # Opt-in (C2W_LN_CHAIN=1 or the attribute): the chain form of a level side -- residual-block outputs that only the next block reads are
    # not written, the next block rebuilds its residual from the LayerNorm rows this one emitted (forward.py: res_block).  Measured at B = 128, bf16
    # (profiles/r06_experiments.md): -0.23 ms per step (five 128-channel launches lose their 537 / 134 MB store), but the rebuilt
    # residual carries the rounding of h = LN(x + m) scaled by sigma -- 2^-9 |x + m - mean| instead of 2^-9 |x| -- and where the modulation
    # dominates the block input that is MORE than rounding x itself: against the CPU oracle the worst gradient tensor moves from
    # 8.7e-3 to 1.7e-2 relative L2 (bf16; fp16 5e-3 -> 8.5e-3 of the output scale).  Parity before 0.5 %: off.
    chain_blocks = os.environ.get("C2W_LN_CHAIN") == "1"
    fuse_loss = os.environ.get("C2W_NO_LOSS_FUSION") is None  # off: the loss tail as its own pass (rounds 1-5); the library reads the same variable

    def __init__(self, net):
        self.layout = Layout(net)
        self.ln_unbiased = bool(getattr(net, "ln_unbiased", True))
        self.flat: Optional[torch.Tensor] = None
        self.flat_grad: Optional[torch.Tensor] = None
        self.shadows: Dict[int, torch.Tensor] = {}   # 16-bit dtype -> copy of the flat buffer in that format
        self._shadow_ver: Dict[int, object] = {}
        self.dg: Dict[int, torch.Tensor] = {}
        self.dg_lin: Optional[torch.Tensor] = None
        self._dg_ver: Dict[object, int] = {}
        self._dg_desc: Dict[object, tuple] = {}
        self._wpad: Dict[object, tuple] = {}   # (name, dtype) -> (version, zero-padded operand copy)
        # stage-major packed copies of the 3x3 weights for the 16x16-tile kernel (ops.pack_conv_weights_batched): "f" forward operands
        # (from the 16-bit shadow), "d" input-gradient operands (from the transposed copies); (kind, dtype) -> buffer / version / table
        self._pk: Dict[tuple, torch.Tensor] = {}
        self._pk_tab: Dict[tuple, tuple] = {}
        self._pk_ok: Dict[tuple, bool] = {}    # launch geometry -> does c2w_conv_forward take packed weights there
        self._pk_want: Dict[tuple, dict] = {}   # (kind, dtype) -> {name of a matrix that is kept packed: weight version of its copy}
        self._pk_desc: Dict[tuple, torch.Tensor] = {}  # ((kind, dtype), names) -> descriptor table of one pack launch
        self._pk_sync: Dict[tuple, list] = {}  # (kind, dtype) -> [(event behind a pack launch, ids of the streams ordered behind it)]
        self.use_packed_weights = True
        self._gwpad: Dict[str, torch.Tensor] = {}  # name -> padded fp32 weight-gradient scratch
        self._manual_ver = 0
        self._wg_stream = None  # second HIP stream for the weight-gradient launches (see _wg)
        # C2W_WGRAD_STREAM=1 (read once, here; or set the attribute): the two-stream mode -- weight gradients on a second stream.  Off by
        # default: every kernel alone on the chip, on the caller's stream (profiles/r05_experiments.md section 8).
        self.use_grad_stream = os.environ.get("C2W_WGRAD_STREAM", "0") == "1"
        # part of the two-stream mode: input-gradient operands rebuilt on the side stream beside the next forward (prefetch_backward_operands)
        self.prefetch_dgrad = self.use_grad_stream
        self._dg_ready = None  # event behind input-gradient operands that were rebuilt on the gradient stream (prefetch_backward_operands)
        # Weight gradients of the residual-block convs are collected per geometry during the backward and launched together at the level
        # boundaries (ops.conv_wgrad_grouped), on levels whose grid is at most group_wgrads_max_side pixels high at the reference's batch (_wg)
        self.group_wgrads = True
        self.group_wgrads_max_side = 64
        self._wg_groups: Dict[tuple, list] = {}  # (geometry, dtype) -> [(x, dY, record, geometry)] not launched yet
        self._wg_group_ok: Dict[tuple, bool] = {}
        self._done_releases: list = []  # one callback per live backward_steps generator: hands on the "done" offsets it held back while a group was pending
        self._pub = None  # ops.HostRing of published scalars (publish / published)
        self._skip_dw = False  # inside backward(want_dw=False): weight-gradient launches are skipped
        self._ws: Dict[int, torch.Tensor] = {}  # stream handle -> split-K scratch of the weight-gradient launches on that stream
        # Deterministic mode (opt-in; C2W_DETERMINISTIC=1 sets the default, Trainer(deterministic=...) / ScoreUNet.deterministic the
        # engine's): the bias gradients, the LayerNorm modulation gradients and the loss sum -- everything a training step adds up with
        # fp32 atomics -- go through per-stream scratch buffers in a fixed order instead (include/c2w_hip.h, C2W_CONV_DETERMINISTIC).
        # Off: no launch, no ops.* call and no keyword argument differs from before.
        self.deterministic = os.environ.get("C2W_DETERMINISTIC", "0") not in ("", "0")
        self._det_ws: Dict[int, torch.Tensor] = {}  # stream handle -> scratch of the fixed-order reductions on that stream
        self._det_need: Dict[tuple, int] = {}  # (kind, geometry, dtype, knobs) -> bytes (pure size queries, asked once)
        self._splitk_plans: Dict[tuple, tuple] = {}  # conv geometry -> (workgroups per tile, scratch bytes) (_splitk)
        self.debug_trace: Optional[list] = None  # diagnostics: a list collects (name, output tensor[, operands of a conv]) of every conv / attention launch of a forward
        self.attach(net)

    # ------------------------------------------------------------------ parameter storage
    def attach(self, net) -> None:
        """(Re)build the flat buffer from the module's current parameters and make them views into it."""
        lay = self.layout
        params = dict(net.named_parameters())
        missing = set(lay.views) ^ set(params)
        if missing:
            raise RuntimeError(f"parameter set mismatch between module and layout: {sorted(missing)[:4]} ...")
        dev = next(iter(params.values())).device
        flat = torch.zeros(lay.numel, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for name, (off, shape, strides) in lay.views.items():
                view = torch.as_strided(flat, shape, strides, off)
                view.copy_(params[name].detach().to(torch.float32))
                # the Parameter OBJECT stays (optimizers, DDP reducers and EMA copies made before the first forward hold it, as
                # training_loop.py:116-131 does); only its storage moves into the flat buffer
                params[name].data = view
        # `p.data = view` leaves each Parameter its own version counter: writes through the Parameter objects (torch.optim steps,
        # load_state_dict, EMA copies) never bump flat._version, so the cache key folds the Parameters' counters in (_version)
        self._bound = [params[name] for name in lay.views]
        me = weakref.ref(self)
        self._bound_by_id = {id(prm): prm for prm in self._bound}
        for i in self._bound_by_id:
            _ENGINE_BY_PARAM_ID[i] = me
        self.generation = getattr(self, "generation", 0) + 1  # bumped per (re-)attach: holders of flat-layout plans re-validate
        self._slots, self._slots_net, self._links = None, (lambda: None), []
        self._offs4 = [4 * off for off, _, _ in lay.views.values()]
        self._pver = self._param_versions()
        self.flat = flat
        self.flat_grad = None
        self.shadows.clear()
        self.dg.clear()
        self.dg_lin = None
        self._shadow_ver.clear()
        self._dg_ver.clear()
        self._dg_desc.clear()
        self._wpad.clear()
        self._pk.clear()
        self._pk_tab.clear()
        self._pk_ok.clear()
        self._pk_want.clear()
        self._pk_desc.clear()
        self._pk_sync.clear()
        self._gwpad.clear()

    def is_attached(self, net) -> bool:
        """Are the module's parameters still the objects bound at attach() AND still views into the flat buffer?  Runs at the top of
        every forward (and of every EMA / optimizer call that looks the engine up), on the host's critical path when the caller
        synchronises once per step (training_loop.py:385: loss.item()): the (module, attribute) slots are resolved once per attach."""
        if self.flat is None:
            return False
        slots = self._slots
        if slots is None or self._slots_net() is not net:
            slots = self._slots = [_resolve(net, name) for name in self.layout.views]
            self._slots_net = weakref.ref(net)
            self._links = _module_links(net, self.layout.views)
        for parent, key, child in self._links:  # module surgery after the first forward (net.unet.x = new_module): the cached slots are stale
            if parent._modules.get(key) is not child:
                self._slots = None
                return False
        base = self.flat.data_ptr()
        for (mod, attr), bound, off in zip(slots, self._bound, self._offs4):
            p = mod._parameters[attr]
            if p is not bound or p.data_ptr() != base + off or p.dtype != torch.float32:
                return False
        return True

    def ensure_grad_buffer(self, net=None, bind: bool = False) -> torch.Tensor:
        """Flat fp32 gradient buffer (same offsets as the parameters).  With ``bind`` every Parameter's ``.grad`` becomes
        a view into it, so optimizers / all-reduce see one contiguous tensor."""
        if self.flat_grad is None:
            self.flat_grad = torch.zeros_like(self.flat)
        if bind and net is not None:
            for name, (off, shape, strides) in self.layout.views.items():
                mod, attr = _resolve(net, name)
                mod._parameters[attr].grad = torch.as_strided(self.flat_grad, shape, strides, off)
        return self.flat_grad

    def _param_versions(self) -> int:
        return sum(p._version for p in self._bound)

    def refresh_version(self) -> None:
        """Re-read the bound Parameters' version counters (once per forward: 228 attribute reads, not one set per launch)."""
        self._pver = self._param_versions()

    def _version(self):
        """Key of every cache derived from the weights (16-bit shadow, padded input-conv operand, input-gradient operands):
        in-place writes on the flat buffer, raw-pointer writers (weights_changed) and writes through the Parameter objects."""
        return (self.flat._version, self._manual_ver, self._pver)

    def weights_changed(self, shadow_fresh: Optional[int] = None) -> None:
        """Call after the flat buffer was rewritten through raw pointers (fused optimizer): torch's version counter
        does not see those writes.  ``shadow_fresh``: the 16-bit dtype whose shadow the writer also refreshed."""
        self._manual_ver += 1
        self.refresh_version()
        if shadow_fresh is not None and shadow_fresh in self.shadows:
            self._shadow_ver[shadow_fresh] = self._version()

    def shadow_for(self, dt: int) -> torch.Tensor:
        """The flat parameter buffer in the 16-bit format ``dt``, refreshed if the weights changed since the last cast."""
        sh = self.shadows.get(dt)
        if sh is None:
            sh = self.shadows[dt] = torch.empty(self.layout.numel, dtype=TORCH_DTYPE[dt], device=self.flat.device)
        if self._shadow_ver.get(dt) != self._version():
            ops.cast_f32(self.flat, sh, self.layout.numel, dt)
            self._shadow_ver[dt] = self._version()
        return sh

    def _w(self, rec: ConvRec, dt: int) -> torch.Tensor:
        if rec.kstride != rec.cin:  # network-input conv: the kernels want K in whole 128-byte chunks -> zero-padded operand copy
            key = (rec.name, dt)
            ent = self._wpad.get(key)
            if ent is None or ent[0] != self._version():
                buf = ent[1] if ent is not None else torch.zeros(rec.rows * rec.taps * rec.kstride, dtype=TORCH_DTYPE[dt], device=self.flat.device)
                buf.view(rec.rows, rec.taps, rec.kstride)[:, :, : rec.cin].copy_(
                    self.flat[rec.w_off: rec.w_off + rec.rows * rec.taps * rec.cin].view(rec.rows, rec.taps, rec.cin))
                self._wpad[key] = (self._version(), buf)
                ent = self._wpad[key]
            return ent[1]
        if rec.lin or dt == DTYPE_F32:
            return self.flat[rec.w_off:]
        return self.shadow_for(dt)[rec.w_off:]

    def prepare_forward(self, dt: int) -> None:
        """Build every lazily cached forward operand (16-bit weight shadow, padded input-conv weights) on the current stream,
        so that forwards issued afterwards on other streams only read them."""
        self.refresh_version()
        for rec in self.layout.convs.values():
            self._w(rec, DTYPE_F32 if rec.lin else dt)
        if self.use_packed_weights:
            # only what earlier launches asked for (the levels the 16x16-tile kernel serves at the batch sizes seen so far), one launch;
            # a matrix that a later geometry asks for first is packed on the stream that asks and the others wait on its event (_packed)
            self.repack_wanted(dt)

    def _b(self, rec: ConvRec) -> torch.Tensor:
        return self.flat[rec.b_off:]

    def _wT(self, rec: ConvRec, dt: int) -> torch.Tensor:
        """Operand of the input-gradient GEMM for ``rec`` ([cin][taps][dg_ld]); rebuilt when the weights changed."""
        lay = self.layout
        key = "lin" if rec.lin else dt
        if rec.lin:
            if self.dg_lin is None:
                self.dg_lin = torch.zeros(max(lay.dg_lin_numel, 1), dtype=torch.float32, device=self.flat.device)
            buf, d = self.dg_lin, DTYPE_F32
        else:
            if dt not in self.dg:
                self.dg[dt] = torch.zeros(max(lay.dg_numel, 1), dtype=TORCH_DTYPE[dt], device=self.flat.device)
            buf, d = self.dg[dt], dt
        if self._dg_ver.get(key, -1) != self._version():
            if key not in self._dg_desc:  # one launch for all matrices of the group: descriptor table built once
                recs = [r for r in lay.convs.values() if r.dg_off >= 0 and r.lin == rec.lin]
                tab = [v for r in recs for v in (r.w_off, r.dg_off, r.rows, r.taps, r.cin, r.cin, r.dg_ld, int(bool(r.flip)))]
                self._dg_desc[key] = (torch.tensor(tab, dtype=torch.int64, device=self.flat.device), len(recs))
            desc, n = self._dg_desc[key]
            if n:
                ops.weight_transpose_batched(self.flat, buf, desc, n, d)
            self._dg_ver[key] = self._version()
        return buf[rec.dg_off:]

    def _packed(self, kind: str, rec: ConvRec, dt: int) -> Optional[torch.Tensor]:
        """Stage-major packed copy of ``rec``'s forward (kind "f") or input-gradient (kind "d") operand in the 16-bit format ``dt``, or
        None when the matrix has none (1x1 / Linear / fp32 / the padded network-input operand).

        Addresses are STABLE: the buffer of a (kind, dtype) is laid out once for every eligible matrix (72 M elements = 144 MB of address
        space, touched only where something is packed) and never reallocated, so a captured hipGraph that reads a packed matrix
        (score_fn._score_graphed) stays valid when another launch geometry later asks for a matrix that was not packed before.  Only the
        matrices some launch asked for are kept packed (at B = 128 the levels the 16x16-tile kernel serves hold 11 of the 72 M
        parameters): one launch repacks all of them when the weights changed, one launch packs a newcomer."""
        if dt == DTYPE_F32 or rec.lin or rec.taps != 9:
            return None
        key = (kind, dt)
        tab = self._pk_tab.get(key)
        if tab is None:  # fixed offsets of every eligible matrix, in layout order
            offs, total = {}, 0
            for r in self.layout.convs.values():
                if r.lin or r.taps != 9:
                    continue
                if kind == "f":
                    if r.kstride != r.cin or r.cin % 32:
                        continue
                    ent = (r.w_off, r.rows, r.cin)
                else:
                    if r.dg_off < 0 or r.dg_ld % 32:
                        continue
                    ent = (r.dg_off, r.cin, r.dg_ld)
                offs[r.name] = (total,) + ent
                total += ops.packed_conv_weights_numel(ent[1], ent[2])
            tab = self._pk_tab[key] = (offs, total)
        offs, total = tab
        ent = offs.get(rec.name)
        if ent is None:
            return None
        if kind == "f":
            src = self.shadow_for(dt)
        else:
            self._wT(rec, dt)  # refreshes the transposed copies if the weights changed
            src = self.dg[dt]
        buf = self._pk.get(key)
        if buf is None:
            buf = self._pk[key] = torch.empty(max(total, 1), dtype=TORCH_DTYPE[dt], device=self.flat.device)
        want = self._pk_want.setdefault(key, {})  # name -> weight version its packed copy was made from
        ver = self._version()
        if want.get(rec.name) != ver:
            want[rec.name] = None
            stale = tuple(n for n, v in want.items() if v != ver)  # everything wanted after an update; the newcomer alone otherwise
            desc = self._pk_desc.get((key, stale))
            if desc is None:
                rows_t = [v for n in stale for v in (offs[n][1], offs[n][0], offs[n][2], offs[n][3])]
                desc = self._pk_desc[(key, stale)] = torch.tensor(rows_t, dtype=torch.int64, device=self.flat.device)
            ops.pack_conv_weights_batched(src, buf, desc, len(stale), dt)
            for n in stale:
                want[n] = ver
            if buf.is_cuda:  # forwards on OTHER streams (score_fn: window batches alternate between streams) must see this launch
                ev = torch.cuda.Event()
                ev.record()
                rec_ = (ev, {torch.cuda.current_stream().cuda_stream})
                # one record per pack launch that is still the newest writer of some matrix: a launch that rewrote EVERYTHING wanted
                # supersedes the older ones; a newcomer's launch joins them (a stream that packs a newcomer has not thereby waited for
                # the packs other streams made earlier)
                if len(stale) == len(want):
                    self._pk_sync[key] = [rec_]
                else:
                    self._pk_sync.setdefault(key, []).append(rec_)
        if buf.is_cuda and key in self._pk_sync:
            sid = torch.cuda.current_stream().cuda_stream
            for ev, seen in self._pk_sync[key]:
                if sid not in seen:  # once per (pack launch, stream): order this stream behind every launch that wrote copies it may read
                    torch.cuda.current_stream().wait_event(ev)
                    seen.add(sid)
        return buf[ent[0]:]

    def repack_wanted(self, dt: int) -> None:
        """Refresh, with one launch per kind, the packed copies earlier launches asked for (prepare_forward)."""
        for (kind, d), want in self._pk_want.items():
            if d == dt and want:
                self._packed(kind, self.layout.convs[next(iter(want))], dt)

    def prefetch_backward_operands(self, dt: int) -> None:
        """Rebuild the input-gradient operands (transposed copies of every weight matrix, and the packed copies the 16x16-tile launches
        asked for) NOW, on the gradient stream, behind everything enqueued so far on the current stream (= the optimizer's update):
        0.18 ms of HBM-bound passes that then run next to the following forward's matrix-core launches instead of in front of the
        backward.  ``backward`` waits for them (``_dg_ready``); without a gradient stream nothing happens and backward builds them itself."""
        side = self.side_stream() if self.prefetch_dgrad else None
        if side is None:
            return
        self.refresh_version()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for grp_lin in (False, True):
                rec0 = next((r for r in self.layout.convs.values() if r.dg_off >= 0 and r.lin == grp_lin), None)
                if rec0 is not None:
                    self._wT(rec0, DTYPE_F32 if grp_lin else dt)
            want = self._pk_want.get(("d", dt))
            if want and self.use_packed_weights:
                self._packed("d", self.layout.convs[next(iter(want))], dt)
            ev = torch.cuda.Event()
            ev.record()
        self._dg_ready = ev

    def _conv_weights(self, kind: str, rec: ConvRec, dt: int, g: dict, fused_ln_bwd: bool = False):
        """(operand, wpacked flag) for a conv launch of geometry ``g``: the packed copy where the launch goes to the 16x16-tile kernel
        (ops.conv_wpacked_supported; -4.6 % on the dominant launch, bit-identical results), else the plain one."""
        plain = self._w(rec, dt) if kind == "f" else self._wT(rec, dt)
        if not self.use_packed_weights or dt == DTYPE_F32:
            return plain, False
        key = (kind, rec.name, dt, g["B"], g["Hin"], g["Win"], g["Hout"], g["Wout"], g["Cout"], g["mode"], ops.KNOBS_GENERATION)
        ok = self._pk_ok.get(key)
        if ok is None:
            ok = self._pk_ok[key] = bool(ops.conv_wpacked_supported(g, dt))
        if not ok:
            return plain, False
        pk = self._packed(kind, rec, dt)
        return (pk, True) if pk is not None else (plain, False)

    def _gw(self, rec: ConvRec) -> torch.Tensor:
        return self.flat_grad[rec.w_off:]

    def _gb(self, rec: ConvRec) -> torch.Tensor:
        return self.flat_grad[rec.b_off:]

    # ------------------------------------------------------------------ weight gradients on a second stream
    def grad_stream(self):
        """The stream every write into ``flat_grad`` is enqueued on, or None (CPU tensors / ``use_grad_stream`` off, the default since
        round 5: the current stream).  A layer's weight gradient and its input gradient both depend only on the layer's output
        gradient; with one launch per layer (rounds 1-4) the chip idled through every kernel's last round of workgroups, the split-K
        reduction launches and the launch gaps on one stream, and a second stream filled those holes (the LDS footprints forbid real
        co-residency: 160 KB + 2 x 71.7 KB > 160 KB).  Grouped launches leave no such holes."""
        if self.flat is None or not self.flat.is_cuda or not self.use_grad_stream:
            return None
        return self.side_stream()

    def side_stream(self):
        """A second HIP stream on another hardware queue than the caller's (streams.py), or None on the CPU: the gradient stream when
        ``use_grad_stream`` is on, and in any case where the next backward's operands are rebuilt beside the forward
        (prefetch_backward_operands)."""
        if self.flat is None or not self.flat.is_cuda:
            return None
        if self._wg_stream is None or self._wg_stream.device != self.flat.device:
            from .streams import independent_stream
            self._wg_stream = independent_stream(self.flat.device)  # on another hardware queue than the caller's stream (streams.py)
        return self._wg_stream

    def publish(self, scalar: torch.Tensor):
        """Enqueue, behind the launch that produced the fp32 device scalar ``scalar``, its copy into a slot of pinned host memory
        (ops.HostRing); returns (slot, sequence number) for ``published``."""
        if self._pub is None:
            self._pub = ops.HostRing()
        return self._pub.publish(scalar)

    def published(self, slot: int, seq: int, timeout_s: float = 20.0):
        """The value of publication ``seq`` as a Python float once the device has written it (polling host memory: no stream is
        synchronised), or None if the slot has been reused or nothing arrived in ``timeout_s``."""
        import struct
        bits = self._pub.read_bits(slot, seq, timeout_s)
        return None if bits is None else struct.unpack("<f", struct.pack("<i", bits))[0]

    def _on_grad_stream(self, fn, *tensors) -> None:
        """Run ``fn`` (launches that read ``tensors`` and write gradient memory) on the gradient stream, behind everything
        enqueued so far on the current stream.  The tensors were allocated on the current stream and may be dropped by the
        caller before the gradient stream has read them: record_stream defers the reuse of their memory."""
        side = self.grad_stream()
        if side is None:
            fn()
            return
        side.wait_stream(torch.cuda.current_stream())
        for t in tensors:
            t.record_stream(side)
        with torch.cuda.stream(side):
            fn()

    def join_grad_stream(self) -> None:
        """Make the current stream wait for every gradient launch enqueued so far."""
        self.flush_wgrad_groups()
        side = self.grad_stream()
        if side is not None:
            torch.cuda.current_stream().wait_stream(side)

    def workspace(self, min_bytes: int = 0) -> Optional[torch.Tensor]:
        """Split-K scratch for a weight-gradient launch on torch's CURRENT stream.  One buffer per (engine, stream): launches on one
        stream are ordered, so they can share it; two engines, or one engine's backward on two streams (training on the gradient
        stream next to an exact-guidance backward elsewhere), never see each other's partial sums.  ``min_bytes``: a grouped launch's
        need (ops.conv_wgrad_grouped_workspace_bytes); a larger buffer replaces the stream's (the old one is freed behind the launches
        that used it: same stream)."""
        if self.flat is None or not (self.flat.is_cuda or self.deterministic):
            return None
        # (CPU tensors -- the emulated tier of the tests -- have no split to hold; the deterministic mode's bias rows live here too)
        key = torch.cuda.current_stream(self.flat.device).cuda_stream if self.flat.is_cuda else 0
        ws = self._ws.get(key)
        if ws is None or ws.device != self.flat.device or ws.numel() * 4 < min_bytes:
            ws = self._ws[key] = ops.new_workspace(self.flat.device, max(ops.WORKSPACE_BYTES, (min_bytes + (1 << 20) - 1) >> 20 << 20))
        return ws

    # ------------------------------------------------------------------ deterministic mode: scratch sizes and buffers
    def _det_bytes(self, key: tuple, query) -> int:
        key = key + (ops.KNOBS_GENERATION,)
        n = self._det_need.get(key)
        if n is None:
            n = self._det_need[key] = int(query())
        return n

    def det_scratch(self, nbytes: int) -> torch.Tensor:
        """Scratch of a fixed-order reduction launched on torch's CURRENT stream (one buffer per stream, like ``workspace``; it only
        grows, so a training run allocates it during its first step and never again)."""
        key = torch.cuda.current_stream(self.flat.device).cuda_stream if self.flat.is_cuda else 0
        ws = self._det_ws.get(key)
        if ws is None or ws.device != self.flat.device or ws.numel() * 4 < nbytes:
            ws = self._det_ws[key] = torch.empty(max((nbytes + 3) // 4, 1 << 16), dtype=torch.float32, device=self.flat.device)
        return ws

    def loss_det_kw(self) -> dict:
        """Keyword arguments of the loss launchers (ops.mse_loss_grad, mse_loss_grad_noise, sq_err): nothing unless the mode is on."""
        return self._det_kw(("loss",), lambda: ops.loss_det_scratch_bytes())

    def _det_kw(self, key: tuple, query) -> dict:
        """``det=`` argument of a launch that reduces in a fixed order (``query``: its scratch size): nothing unless the mode is on"""
        return dict(det=self.det_scratch(self._det_bytes(key, query))) if self.deterministic else {}

    @staticmethod
    def _gkey(g: dict) -> tuple:
        return (g["B"], g["Hin"], g["Win"], g["Cin"], g["Hout"], g["Wout"], g["Cout"], g["ldy"], g["wrows"], g["mode"])

    def _wgrad_kw(self, g: dict, dt: int) -> dict:
        """workspace (+ deterministic) arguments of one ops.conv_wgrad launch on the current stream"""
        if not self.deterministic:
            return dict(workspace=self.workspace())
        need = self._det_bytes(("wgrad", self._gkey(g), dt), lambda: ops.conv_wgrad_workspace_bytes(g, dt, deterministic=True))
        return dict(workspace=self.workspace(need), deterministic=True)

    def _splitk(self, g: dict, dt: int, act: int):
        """(scratch, workgroups per tile) if this inference launch should deal its K chunks to several workgroups (ops.conv_splitk_plan:
        fewer output tiles than the chip has CUs -- the deep levels of a sampler step on a short trajectory), else None.  The plan is
        a pure function of geometry and knobs: remembered per geometry."""
        if self.flat is None or not self.flat.is_cuda:
            return None
        key = self._gkey(g) + (dt, act, ops.KNOBS_GENERATION)
        plan = self._splitk_plans.get(key)
        if plan is None:
            plan = self._splitk_plans[key] = ops.conv_splitk_plan(g, dt, act)
        ns, nbytes = plan
        if ns <= 1:
            return None
        return self.workspace(nbytes), ns

    def _wg(self, x: torch.Tensor, gy: torch.Tensor, rec: ConvRec, g: dict, dt: int, group: bool = False) -> None:
        """dW, dbias of ``rec`` (dense operand) into the flat gradient buffer, on the gradient stream.  ``group``: the layer is one of
        several with this geometry whose output gradients appear one after the other (the residual-block convs of a level side): it is
        queued and launched with the others at the next flush_wgrad_groups()."""
        if self._skip_dw:
            return
        # "up to N x N grids" is meant at the reference's batch of 128 per GPU: what decides is the layer's K extent (B x H x W pixels;
        # the deep variant's 128x128 level at B = 32 is the default network's 64x64 level at B = 128)
        npx = g["B"] * g["Hout"] * g["Wout"]
        small = npx <= 128 * self.group_wgrads_max_side ** 2
        # one size up -- the 128x128 level at 64 windows per GPU, the reference's global batch of 512 on 8 GPUs: groups of three
        # (round 6, B = 64: 26.00 -> 25.84 ms per step; at B = 128 the same grouping costs 0.25 ms: profiles/r05_experiments.md);
        # above that one launch per layer
        cap = 16 if small else 3 if npx <= 256 * self.group_wgrads_max_side ** 2 else 1
        if group and self.group_wgrads and cap > 1:
            # (_gkey without ``wrows``, on purpose: these fields decide which layers share a grouped launch)
            key = (g["B"], g["Hin"], g["Win"], g["Cin"], g["Hout"], g["Wout"], g["Cout"], g["ldy"], g["mode"], dt, ops.KNOBS_GENERATION)
            ok = self._wg_group_ok.get(key)
            if ok is None:
                ok = self._wg_group_ok[key] = bool(ops.conv_wgrad_grouped_supported(g, 2, dt))
            if ok:
                lst = self._wg_groups.setdefault(key, [])
                lst.append((x, gy, rec, g))
                if len(lst) >= cap:
                    self._flush_group(key)
                    if not self._wg_groups:
                        self._release_done()
                return
        self._on_grad_stream(lambda: ops.conv_wgrad(x, gy, self._gw(rec), g, dt, dbias=self._gb(rec), **self._wgrad_kw(g, dt)), x, gy)

    def _flush_group(self, key: tuple) -> None:
        lst = self._wg_groups.pop(key, None)
        if not lst:
            return
        g, dt = lst[0][3], key[9]
        if len(lst) == 1 or not ops.conv_wgrad_grouped_supported(g, len(lst), dt):
            for x, gy, rec, gi in lst:
                self._on_grad_stream(lambda x=x, gy=gy, rec=rec, gi=gi: ops.conv_wgrad(x, gy, self._gw(rec), gi, dt, dbias=self._gb(rec),
                                                                                    **self._wgrad_kw(gi, dt)), x, gy)
            return

        def run():
            kw = dict(deterministic=True) if self.deterministic else {}
            ws = self.workspace(ops.conv_wgrad_grouped_workspace_bytes(g, len(lst), dt, **kw))
            ops.conv_wgrad_grouped([(x, gy, self._gw(rec), self._gb(rec)) for x, gy, rec, _ in lst], g, dt, workspace=ws, **kw)
        self._on_grad_stream(run, *[t for x, gy, _, _ in lst for t in (x, gy)])

    def flush_wgrad_groups(self) -> None:
        """Launch every queued weight gradient (one launch per geometry) and hand on the "done" offsets that were held back for them."""
        for key in list(self._wg_groups):
            self._flush_group(key)
        self._release_done()

    def _release_done(self) -> None:
        for rel in list(self._done_releases):
            rel()

    def _wgrad(self, rec: ConvRec, x: torch.Tensor, gy: torch.Tensor, g: dict, dt: int) -> None:
        """dW (+ dbias) of ``rec`` into the flat gradient buffer; a padded-operand layer goes through a padded scratch."""
        if self._skip_dw:
            return
        if rec.kstride == rec.cin:
            self._wg(x, gy, rec, g, dt)
            return

        def run():
            n = rec.rows * rec.taps * rec.kstride
            buf = self._gwpad.get(rec.name)
            if buf is None or buf.device != self.flat.device:
                buf = self._gwpad[rec.name] = torch.zeros(n, dtype=torch.float32, device=self.flat.device)
            else:
                buf.zero_()
            ops.conv_wgrad(x, gy, buf, g, dt, dbias=self._gb(rec), **self._wgrad_kw(g, dt))
            self.flat_grad[rec.w_off: rec.w_off + rec.rows * rec.taps * rec.cin].view(rec.rows, rec.taps, rec.cin).add_(
                buf.view(rec.rows, rec.taps, rec.kstride)[:, :, : rec.cin])
        self._on_grad_stream(run, x, gy)

    # ------------------------------------------------------------------ small helpers
    @staticmethod
    def _geom(B, Hin, Win, Cin, Hout, Wout, Cout, ldy, wrows, mode):
        return dict(B=B, Hin=Hin, Win=Win, Cin=Cin, Hout=Hout, Wout=Wout, Cout=Cout, ldy=ldy, wrows=wrows, mode=mode)

    def _linear(self, name: str, x: torch.Tensor, rows: int, act: int, tape: Optional[Tape], need_dx: bool = True) -> torch.Tensor:
        """fp32 GEMM  y[rows_x][out] = x . W^T + b  on the fp32 matrix-core path (Linear layers of model/score.py:56-57,
        model/nn.py:149)."""
        rec = self.layout.convs[name]
        y = torch.empty((rows, rec.rows), dtype=torch.float32, device=x.device)
        if rows == 1 and tape is None and act in (ACT_NONE, ACT_SILU, ACT_RELU):
            # one t for the whole batch (the sampler): a matrix-vector product instead of a 16-pixel MFMA tile with one live column
            ops.gemv_f32(x, self._w(rec, DTYPE_F32), self._b(rec), y, rec.rows, rec.cin, rec.kstride, act)
            return y
        g = self._geom(rows, 1, 1, rec.kstride, 1, 1, rec.rows, rec.rows, rec.rows, CONV_1X1)
        ops.conv(x, self._w(rec, DTYPE_F32), self._b(rec), y, g, DTYPE_F32, act=act)
        if tape is not None:
            def bw(gy: torch.Tensor) -> Optional[torch.Tensor]:
                self._wgrad(rec, x, gy, g, DTYPE_F32)  # (a padded operand -- map_forcing -- goes through its padded scratch)
                if not need_dx:
                    tape.done(rec.w_off)
                    return None
                if rec.rows >= self.LINEAR_DGRAD_SPLIT_MIN_ROWS and rec.kstride == rec.cin:
                    # few rows, very long reduction (proj: B x 8448 -> 512): as a forward GEMM that is 4 workgroups walking
                    # K = 8448.  It is also the weight-gradient GEMM of a 1x1 conv over rec.rows "pixels" with the weight
                    # matrix as the input and gy^T as the output gradient -- which splits the reduction over the whole chip.
                    ld = (rows + 3) // 4 * 4
                    gyT = torch.zeros((rec.rows, ld), dtype=torch.float32, device=x.device)
                    # LDS-tiled transpose (torch's strided copy of the 128 x 8448 matrix took 0.49 ms per step)
                    ops.weight_transpose(gy, gyT, rows, 1, rec.rows, rec.rows, ld, False, DTYPE_F32)
                    dx = torch.zeros((rows, rec.cin), dtype=torch.float32, device=x.device)
                    gt = self._geom(rec.rows, 1, 1, rec.cin, 1, 1, rows, ld, rows, CONV_1X1)
                    # same kernels, same split-K workspace as the weight gradients: same stream, then wait for the result
                    wmat = self._w(rec, DTYPE_F32)
                    self._on_grad_stream(lambda: ops.conv_wgrad(wmat, gyT, dx, gt, DTYPE_F32, **self._wgrad_kw(gt, DTYPE_F32)), gyT, dx)
                    self.join_grad_stream()
                    # only now: this route reads the layer's weights from the flat buffer itself, and "done" may start the
                    # optimizer on them (Trainer: the update chases the backward)
                    tape.done(rec.w_off)
                    return dx
                dx = torch.empty((rows, rec.cin), dtype=torch.float32, device=x.device)
                gd = self._geom(rows, 1, 1, rec.dg_ld, 1, 1, rec.cin, rec.cin, rec.cin, CONV_1X1)
                ops.conv(gy, self._wT(rec, DTYPE_F32), None, dx, gd, DTYPE_F32)
                tape.done(rec.w_off)
                return dx
            tape.steps.append(bw)
        return y

    # ------------------------------------------------------------------ forward
    def forward(self, x: torch.Tensor, t: torch.Tensor, dt: int, tape: Optional[Tape] = None, noise: Optional[Tuple] = None,
                want_dx: bool = False, nhwc_out: bool = False, x_nhwc: Optional[torch.Tensor] = None, shape=None,
                forcing: Optional[torch.Tensor] = None, fold: Optional[dict] = None, loss: Optional[dict] = None):
        """eps_pred = ScoreUNet(x, t).  x: (B,C,H,W) fp32 on the GPU; t: numel 1 or B.
        ``fold`` (inference, with ``nhwc_out``): dict(segs=[(eps trajectory (L,F,H,W) fp32, first window, count, first batch row)], k, F,
        nwin) -- the batch rows are windows of trajectories and only what src/thor/score.py:76-88 keeps of them is wanted: where the
        kernel exists the output convolution computes the centre frame's F rows only and writes them into the trajectories
        (ops.conv_center; the other frames of a trajectory's first / last window through the full convolution of that one window) and
        None is returned; otherwise the NHWC output rows are returned and the caller scatters them.
        noise = (eps, musig): fuse the forward noise process x_t = mu x + sigma eps into the input conversion; eps may be an int
        seed instead of a tensor: the kernel regenerates the Philox stream of that seed (ops.philox_normal) and eps never exists.
        ``loss`` (training, with ``nhwc_out`` and a noise SEED): dict(sum, gscale[, scaler]) -- fuse the loss tail of src/thor/pipelines.py:35
        into the output convolution where the kernel exists (ops.conv_loss_supported): the input conversion keeps the noise it mixes in
        (half-precision rows), the returned rows are dY = (prediction - eps) * gscale, ``sum`` has received sum (prediction - eps)^2 and
        ``tape.meta["loss_fused"]`` is True; otherwise nothing changes.
        With ``tape`` every op records its backward closure (training / exact guidance)."""
        lay = self.layout
        self.refresh_version()
        B, C, H, W = shape if x_nhwc is not None else x.shape  # x_nhwc: rows already in the network's input layout (the sampler's fused window gather)
        dev = (x_nhwc if x_nhwc is not None else x).device
        L = len(lay.levels)
        if C != lay.in_channels:
            raise ValueError(f"expected {lay.in_channels} channels, got {C}")
        if H % (1 << (L - 1)) or W % (1 << (L - 1)):
            raise ValueError("spatial size must be divisible by 2**(levels-1) (skip connections, model/nn.py:238)")
        ck = ops.CK[dt]
        for lv in lay.levels:
            if lv.channels % ck:
                raise ValueError(f"hidden_channels must be multiples of {ck} for this compute dtype")
        lazy = x_nhwc is None and hasattr(x, "materialize")  # data.WindowBatch: windows still inside the dataset array
        if x_nhwc is None and not lazy:
            x = x.contiguous().float()
        tt = t.reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
        Bt = tt.numel()
        if Bt not in (1, B):
            raise ValueError("t must hold 1 or B values (model/score.py:60)")
        ldm = lay.sum_c if (Bt == B and B > 1) else 0
        fp = ForwardPass(self, tape, dt, dev, B, ldm, want_dx)  # the launches: forward.py
        fp.embed(tt, Bt, forcing)
        x0, loss_rows = (x_nhwc, None) if x_nhwc is not None else fp.to_nhwc(x, lazy, noise, C, H, W, loss, nhwc_out)
        outs = fp.descend(x0, H, W)
        cur = fp.ascend(outs, H >> (L - 1), W >> (L - 1))
        cur = fp.output(cur, H, W, fold if nhwc_out else None, loss, loss_rows)
        if cur is None:  # folded: the trajectories were written
            return None
        if tape is not None:
            tape.meta.update(B=B, C=C, H=H, W=W, dt=dt, out_nhwc=cur, ldm=ldm, Bt=Bt)
        if nhwc_out:
            return cur
        y = torch.empty((B, C, H, W), dtype=torch.float32, device=dev)
        ops.nhwc_to_nchw(cur, y, B, lay.out_channels, H * W, lay.cout_pad, dt)
        return y


    def _fold_output(self, fold: dict, name: str, xin: torch.Tensor, B: int, H: int, W: int, dt: int) -> bool:
        """The output convolution of a batch of trajectory windows, restricted to the frames fold() keeps (see forward).  False: not
        available for this shape / type -- nothing was written."""
        lay = self.layout
        rec = lay.convs[name]
        k, F, nwin = int(fold["k"]), int(fold["F"]), int(fold["nwin"])
        w = 2 * k + 1
        if not self.use_center_conv or rec.rows != w * F or rec.kstride != rec.cin or \
                not ops.conv_center_supported(H, W, rec.cin, F, dt):
            return False
        HW = H * W
        wts, bias = self._w(rec, dt), self._b(rec)
        T = TORCH_DTYPE[dt]
        for eps, i0, nw, pos in fold["segs"]:
            rows = xin[pos * HW:]
            ops.conv_center(rows, wts, bias, eps[i0 + k:], nw, H, W, rec.cin, rec.rows, k * F, F, F * HW, dt)
            for gi in sorted({0, nwin - 1}):  # a trajectory's first / last window keeps k more frames: the full convolution of that one window
                if not i0 <= gi < i0 + nw:
                    continue
                one = xin[(pos + gi - i0) * HW: (pos + gi - i0 + 1) * HW]
                g = self._geom(1, H, W, rec.kstride, H, W, lay.cout_pad, lay.cout_pad, rec.rows, CONV_S1)
                wop, wpk = self._conv_weights("f", rec, dt, g)
                y1 = torch.empty((HW, lay.cout_pad), dtype=T, device=xin.device)
                ops.conv(one, wop, bias, y1, g, dt, wpacked=wpk)
                ops.window_scatter(y1, eps, 1, F, HW, k, gi, nwin, lay.cout_pad, dt)
        return True

    def _mlp_layer(self, name: str, x: torch.Tensor, rows: int, tape: Optional[Tape], need_dx: bool = True,
                   add: Optional[torch.Tensor] = None, add_bw: Optional[Callable] = None) -> torch.Tensor:
        """silu(Linear(x) [+ add]) of the time-embedding MLP (model/score.py:62-67; ``add`` = the forcing projection, :65-66); keeps the
        pre-activation when taping."""
        if tape is None and add is None:
            return self._linear(name, x, rows, ACT_SILU, None)
        z = self._linear(name, x, rows, ACT_NONE, None)
        if add is not None:
            z.add_(add)  # (rows, E) fp32: the one tensor-arithmetic line of the forward; its adjoint hands gz to both Linears unchanged
        h = torch.empty_like(z)
        ops.silu(z, h, z.numel(), DTYPE_F32)
        if tape is None:
            return h
        rec = self.layout.convs[name]
        g = self._geom(rows, 1, 1, rec.kstride, 1, 1, rec.rows, rec.rows, rec.rows, CONV_1X1)

        def bw(gh: torch.Tensor) -> Optional[torch.Tensor]:
            gz = torch.empty_like(z)
            ops.silu_backward(z, gh, gz, z.numel(), DTYPE_F32)
            if add_bw is not None:  # z = Linear(x) + add: the same gz is the output gradient of whatever produced `add`
                add_bw(gz)
            self._wg(x, gz, rec, g, DTYPE_F32)
            if not need_dx:
                tape.done(rec.w_off)
                return None
            dx = torch.empty((rows, rec.cin), dtype=torch.float32, device=x.device)
            ops.conv(gz, self._wT(rec, DTYPE_F32), None, dx, self._geom(rows, 1, 1, rec.dg_ld, 1, 1, rec.cin, rec.cin, rec.cin, CONV_1X1),
                     DTYPE_F32)
            tape.done(rec.w_off)
            return dx
        tape.steps.append(bw)
        return h

    # ------------------------------------------------------------------ backward
    def backward(self, tape: Tape, gy_nhwc: torch.Tensor, want_dx: bool = False, want_dw: bool = True) -> Optional[torch.Tensor]:
        """Run the recorded closures in reverse.  ``gy_nhwc``: gradient w.r.t. the network output in NHWC rows
        [B*H*W][cout_pad] (padding channels zero).  Parameter gradients are ACCUMULATED into ``flat_grad``.
        ``want_dw=False``: input gradient only -- no weight-gradient launch, no modulation path (exact guidance through a network
        whose parameters do not require gradients, src/thor/score.py:28-33 on the frozen copy exp/downscaling.py:110-126 loads)."""
        if not want_dw:
            self._skip_dw = True
            try:
                return self._backward(tape, gy_nhwc, want_dx, False)
            finally:
                self._skip_dw = False
        if self.flat_grad is None:
            raise RuntimeError("call ensure_grad_buffer() before backward")
        return self._backward(tape, gy_nhwc, want_dx, True)

    def _backward(self, tape: Tape, gy_nhwc: torch.Tensor, want_dx: bool, want_dw: bool) -> Optional[torch.Tensor]:
        it = self.backward_steps(tape, gy_nhwc, want_dx, want_dw)
        try:
            while True:
                next(it)
        except StopIteration as done:
            return done.value

    def backward_steps(self, tape: Tape, gy_nhwc: torch.Tensor, want_dx: bool = False, want_dw: bool = True):
        """``backward`` as a generator: yields after every recorded closure the lowest flat offset whose gradient is final so far
        (``layout.numel`` before the first; see Tape.progress) -- a caller may hand finished suffixes of the gradient buffer on while
        the rest of the pass is still to be enqueued (score.py::_GradSegment: torch's DistributedDataParallel all-reduces a bucket as
        soon as its gradients have been delivered).  The generator's return value is dx (or None)."""
        low = [self.layout.numel]
        outer = tape.progress
        held = [None]

        def emit(off: int) -> None:
            low[0] = min(low[0], off)
            if outer is not None:
                outer(off)

        def progress(off: int) -> None:
            if self._wg_groups:  # a weight gradient at or above ``off`` is still queued (grouped launches): not final yet
                held[0] = off if held[0] is None else min(held[0], off)
                return
            emit(off)

        def release() -> None:
            if held[0] is not None and not self._wg_groups:
                off, held[0] = held[0], None
                emit(off)
        # Grouped weight gradients queued by ANOTHER backward that is still being consumed on this engine (two recorded forwards whose
        # backward generators interleave: score.py::_GradSegment chains driven by autograd) are legitimate pending work: launch them and
        # let that backward hand on the offsets it held, instead of dropping them silently (round-5 advisor finding).  What a backward
        # that RAISED left behind is dropped by its own generator (the finally clause below), never seen here.
        if self._wg_groups:
            self.flush_wgrad_groups()
        tape.progress = progress
        self._done_releases.append(release)
        completed = False
        try:
            dx0, m = yield from self._backward_body(tape, gy_nhwc, want_dx, want_dw, low, outer)
            completed = True
        finally:
            if release in self._done_releases:
                self._done_releases.remove(release)
            if not completed:  # raised or closed half-way: queued launches hold tensors of a pass that will never finish
                self._wg_groups.clear()
                tape.progress = outer
        if not want_dx or dx0 is None:
            return None
        dx = torch.empty((m["B"], m["C"], m["H"], m["W"]), dtype=torch.float32, device=dx0.device)
        ops.nhwc_to_nchw(dx0, dx, m["B"], m["C"], m["H"] * m["W"], self.layout.cin_pad, m["dt"])
        return dx

    def _backward_body(self, tape: Tape, gy_nhwc: torch.Tensor, want_dx: bool, want_dw: bool, low, outer):
        if self._dg_ready is not None:  # operands prefetched on the gradient stream: this stream reads them from here on
            torch.cuda.current_stream().wait_event(self._dg_ready)
            self._dg_ready = None
        # Build the input-gradient operands (transposed copies of ALL weights, read from the flat buffer) before the first launch on
        # the gradient stream: whoever updates a finished part of the flat buffer from that stream while backward is still running
        # (Trainer: optimizer chasing the backward) is then ordered behind these reads by the stream's first wait on this one.
        for grp_lin in (False, True):
            rec0 = next((r for r in self.layout.convs.values() if r.dg_off >= 0 and r.lin == grp_lin), None)
            if rec0 is not None:
                self._wT(rec0, DTYPE_F32 if grp_lin else tape.meta["dt"])
        steps = tape.steps
        n_mlp = 3  # map_layer0, map_layer1, proj were recorded first
        g = gy_nhwc
        for bw in reversed(steps[n_mlp:]):
            g = bw(g)
            yield low[0]
        dx0 = g
        self.flush_wgrad_groups()
        # modulation path: dm_all -> proj -> map_layer1 -> map_layer0 (parameter gradients only: t carries none)
        if want_dw:
            gm = tape.meta["dm_all"]
            for bw in reversed(steps[:n_mlp]):
                gm = bw(gm)
                yield low[0]
        self.join_grad_stream()  # every gradient is in flat_grad for whoever runs next on this stream (optimizer, autograd)
        tape.steps = []
        tape.gskip.clear()
        tape.progress = outer
        return dx0, tape.meta


def _module_links(net, names):
    """(parent module, child key, child module) for every module on the path to one of the parameters ``names``, each link once."""
    links, seen = [], set()
    for name in names:
        mod = net
        for p in name.split(".")[:-1]:
            child = mod._modules[p]
            if (id(mod), p) not in seen:
                seen.add((id(mod), p))
                links.append((mod, p, child))
            mod = child
    return links


def _resolve(net, name: str):
    parts = name.split(".")
    mod = net
    for p in parts[:-1]:
        mod = getattr(mod, p) if not p.isdigit() else mod[int(p)]
    return mod, parts[-1]
