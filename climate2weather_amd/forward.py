"""One forward of the engine (engine.Engine.forward) as a per-call object: the launches of the time-embedding MLP, the input conversion, the
level walks and the output convolution, and the backward closures they record on the tape.  The object holds the call's constants and
NO activation tensor: a backward closure keeps alive what it names, and it names the pass."""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import torch

from . import ops
from .nn import BlockSpec
from .ops import (ACT_NONE, ACT_RELU, ACT_RELU_PAIR, ACT_SILU, ACT_SILU_PAIR, CONV_1X1, CONV_S1, CONV_S2, CONV_TS2, CONV_UP, DTYPE_F32, MUL_DSILU,
                  MUL_PLAIN, TORCH_DTYPE)

LN_EPS = 1e-5


class LnRows(NamedTuple):
    """LayerNorm output rows a conv epilogue emitted for its consumer, with the statistics it kept (training: 1/sigma; chain form: the mean)."""
    rows: torch.Tensor
    rstd: Optional[torch.Tensor] = None
    mean: Optional[torch.Tensor] = None


class ForwardPass:
    __slots__ = ("eng", "lay", "tape", "dt", "T", "dev", "B", "ldm", "train", "want_dx", "m_all", "dm_all")

    def __init__(self, eng, tape, dt: int, dev, B: int, ldm: int, want_dx: bool):
        self.eng, self.lay, self.tape, self.dt, self.T, self.dev, self.B, self.ldm = eng, eng.layout, tape, dt, TORCH_DTYPE[dt], dev, B, ldm
        self.train, self.want_dx = tape is not None, want_dx
        self.m_all = self.dm_all = None

    def embed(self, tt: torch.Tensor, Bt: int, forcing: Optional[torch.Tensor]) -> None:
        """time embedding MLP + all modulation vectors (fp32): sets m_all (and, training, dm_all)"""
        eng, lay, tape, dev, B = self.eng, self.lay, self.tape, self.dev, self.B
        pe = torch.empty((Bt, lay.noise_features), dtype=torch.float32, device=dev)
        ops.timestep_embedding(tt, pe, Bt, lay.noise_features)
        emb = eng._mlp_layer("map_layer0", pe, Bt, tape, need_dx=False)
        zf = forcing_bw = None
        if lay.forcing_dim:  # emb = silu(map_layer1(.) + map_forcing(forcing))  (model/score.py:64-67)
            if forcing is None:
                raise ValueError("forcing_dim > 0: the forcing vector is required")
            rf = lay.convs["map_forcing"]
            fr = forcing.reshape(-1, lay.forcing_dim).to(device=dev, dtype=torch.float32)
            if fr.shape[0] not in (1, Bt) and not (Bt == 1 and fr.shape[0] == B):
                raise ValueError(f"forcing has {fr.shape[0]} rows for {Bt} time values / {B} batch items")
            if Bt == 1 and fr.shape[0] == B and B > 1:  # scalar t, per-item forcing: the embedding becomes per item
                raise NotImplementedError("per-item forcing with a scalar t: pass t with one value per batch item")
            fpad = torch.zeros((Bt, rf.kstride), dtype=torch.float32, device=dev)
            fpad[:, : lay.forcing_dim] = fr if fr.shape[0] == Bt else fr.expand(Bt, -1)
            zf = eng._linear("map_forcing", fpad, Bt, ACT_NONE, None)  # not on the tape: its gradient is map_layer1's pre-activation gradient
            g_f = eng._geom(Bt, 1, 1, rf.kstride, 1, 1, rf.rows, rf.rows, rf.rows, CONV_1X1)
            if tape is not None:
                def forcing_bw(gz):
                    eng._wgrad(rf, fpad, gz, g_f, DTYPE_F32)
                    tape.done(rf.w_off)
        elif forcing is not None:
            raise ValueError("forcing passed to a network built with forcing_dim == 0 (model/score.py:60)")
        emb = eng._mlp_layer("map_layer1", emb, Bt, tape, add=zf, add_bw=forcing_bw)
        self.m_all = eng._linear("proj", emb, Bt, ACT_NONE, tape)
        if self.train:
            self.dm_all = tape.meta["dm_all"] = torch.zeros_like(self.m_all)

    def to_nhwc(self, x, lazy: bool, noise, C: int, H: int, W: int, loss, nhwc_out: bool):
        """Network input -> NHWC rows, the forward noise process mixed in.  Returns (x0, (noise rows, channel stride) the conversion kept
        for the fused loss tail, or None).  The attempts, in this order; each kernel may refuse the shape:"""
        eng, lay, dt, dev, B = self.eng, self.lay, self.dt, self.dev, self.B
        x0 = torch.empty((B * H * W, lay.cin_pad), dtype=self.T, device=dev)
        regen = noise is not None and isinstance(noise[0], int)  # regenerated noise: (seed, musig)
        # 1. Fused loss tail (round 6): where the output conv takes it (ops.conv_loss_supported), the input conversion KEEPS the noise it
        # mixes in -- rounded to half precision, as NHWC rows -- and the output conv's epilogue reads it back: the generator runs
        # once per step instead of twice and the prediction is never written.  The step's noise is then the rounded stream.
        if loss is not None and self.train and nhwc_out and regen and eng.fuse_loss and dt != DTYPE_F32 and lay.out_channels == C and (H * W) % 4 == 0:
            rec_o = lay.convs["unet." + lay.levels[0].tail_key]
            g_o = eng._geom(B, H, W, rec_o.kstride, H, W, lay.cout_pad, lay.cout_pad, rec_o.rows, CONV_S1)
            if ops.conv_loss_supported(g_o, dt):
                lde = (C + 7) // 8 * 8
                erows = torch.empty((B * H * W, lde), dtype=torch.float16, device=dev)
                src, offs = (x.data, x.offsets()) if lazy else (x, None)
                if (not lazy or (x.data.is_contiguous() and x.data.dtype == torch.float32)) and \
                        ops.nchw_to_nhwc_noise_rows(src, offs, noise[0], noise[1], x0, erows, B, C, H * W, lay.cin_pad, lde, dt):
                    return x0, (erows, lde)
        if lazy:
            # 2. windows still inside the dataset array: convert them in place where the fused kernel takes the shape
            if regen and x.data.is_contiguous() and x.data.dtype == torch.float32 and \
                    ops.windows_to_nhwc_noise(x.data, x.offsets(), noise[0], noise[1], x0, B, C, H * W, lay.cin_pad, dt):
                return x0, None
            x = x.materialize().contiguous().float()  # 3.
        if not regen:  # 6. noise given as a tensor, or none
            ops.nchw_to_nhwc(x, noise[0] if noise else None, noise[1] if noise else None, x0, B, C, H * W, lay.cin_pad, dt)
        elif not ops.nchw_to_nhwc_noise(x, noise[0], noise[1], x0, B, C, H * W, lay.cin_pad, dt):  # 4. the regenerated-noise kernel
            eps = torch.empty_like(x)  # 5. the same stream, materialised
            ops.philox_normal(eps, eps.numel(), noise[0])
            ops.nchw_to_nhwc(x, eps, noise[1], x0, B, C, H * W, lay.cin_pad, dt)
        return x0, None

    def conv3(self, name, xin, Hi, Wi, Ho, Wo, mode, act=ACT_NONE, res=None, ldy=None, cout=None, y2=None, want_ln=None, loss=None,
              resn=None, no_y=False):
        """want_ln: None, or the consumer's LayerNorm to emit from this conv's epilogue: ("mod", modulation rows) for a
        residual block, ("plain", None) for an up-block.  Returns (y, geometry, record, LnRows or None: not asked for / not fused here).
        The chain form (res_block): ``resn`` = dict(rstd, mean, m) -- ``res`` holds normalised rows and the residual is rebuilt from
        them; ``no_y`` -- the result is not written (y is None), the emitted LayerNorm keeps its mean next to its 1/sigma."""
        eng, dt, T, dev, train = self.eng, self.dt, self.T, self.dev, self.train
        rec = self.lay.convs[name]
        ldy_ = ldy or rec.rows
        npix = self.B * Ho * Wo
        y = torch.empty((npix, ldy_), dtype=T, device=dev) if not no_y else None
        g = eng._geom(self.B, Hi, Wi, rec.kstride, Ho, Wo, cout or rec.rows, ldy_, rec.rows, mode)
        hn = lnf = None
        if want_ln is not None and act == ACT_NONE and y2 is None and ops.conv_lnfwd_supported(g, dt):
            rows = torch.empty((npix, ldy_), dtype=T, device=dev)
            lnf = dict(y=rows, m=want_ln[1], ldm=self.ldm if want_ln[1] is not None else 0, eps=LN_EPS, unbiased=eng.ln_unbiased)
            if train and want_ln[0] == "mod":
                # training: the epilogue also leaves every pixel row's 1/sigma; the block's backward then takes its LayerNorm
                # statistics from here and the normalised rows (kept anyway: conv1's input) instead of recomputing both (res_block)
                lnf["rstd"] = torch.empty((npix,), dtype=torch.float32, device=dev)
            if no_y:
                lnf["mean"] = torch.empty((npix,), dtype=torch.float32, device=dev)
            hn = LnRows(rows, lnf.get("rstd"), lnf.get("mean"))
        if no_y or resn is not None:  # (the rebuilt residual lives in the LayerNorm-emitting epilogue; an output that is not written needs its statistics kept)
            assert hn is not None and (not no_y or hn.rstd is not None), "chain form without a fused LayerNorm (run_blocks decides both from the same answers)"
        # padded operand (network input at C = 65: rows of 128 channels): channels >= rec.cin are zero in x and in w -- a promise the
        # 16x16-tile kernel turns into fewer K steps
        wop, wpk = eng._conv_weights("f", rec, dt, g)
        # (deterministic mode: the workgroups' loss sums in a fixed order)
        kw = eng._det_kw(("conv_loss", eng._gkey(g), dt), lambda: ops.conv_det_scratch_bytes(g, dt, loss=True)) if loss is not None else {}
        ops.conv(xin, wop, eng._b(rec), y if y is not None else hn.rows, g, dt, act=act, res=res, y2=y2, lnf=lnf,
                 kvalid=rec.cin if rec.kstride != rec.cin else 0, wpacked=wpk, loss=loss, resn=resn, no_y=no_y, **kw,
                 splitk=eng._splitk(g, dt, act) if (not train and lnf is None and y2 is None and loss is None and not wpk) else None)
        if eng.debug_trace is not None and y is not None:
            eng.debug_trace.append((name, y, dict(x=xin, w=eng._w(rec, dt), g=g, act=act, res=res)))
            if hn is not None:
                eng.debug_trace.append((name + " [LayerNorm emitted]", hn.rows))
        return y, g, rec, hn

    def dgrad(self, rec, gy, Hi, Wi, Ho, Wo, mode, ld_out, mul=None, res=None, ln=None, mulmode=MUL_DSILU):
        """input gradient = implicit GEMM over gy with the transposed (and flipped) weights; (Hi,Wi) = gy's grid.
        ``ln``: LayerNorm-backward arguments to fuse into the epilogue; returns None when the kernel cannot fuse them."""
        eng, dt = self.eng, self.dt
        g = eng._geom(self.B, Hi, Wi, rec.dg_ld, Ho, Wo, ld_out, ld_out, rec.cin, mode)
        if ln is not None and not ops.conv_lnbwd_supported(g, dt):
            return None
        dx = torch.empty((self.B * Ho * Wo, ld_out), dtype=self.T, device=self.dev)
        # output conv at C = 65: gy rows are padded to dg_ld = 128 channels, the padding is zero (mse_loss_grad) and so are the
        # operand's columns there
        wop, wpk = eng._conv_weights("d", rec, dt, g, fused_ln_bwd=ln is not None)
        kw = {}
        if ln is not None and ln.get("dm") is not None:  # deterministic mode: the modulation gradient in a fixed order
            kw = eng._det_kw(("conv_ln", eng._gkey(g), dt, ln["ldm"]), lambda: ops.conv_det_scratch_bytes(g, dt, ln_ldm=ln["ldm"]))
        ops.conv(gy, wop, None, dx, g, dt, res=res, mul=mul, mulmode=mulmode, ln=ln,
                 kvalid=rec.rows if rec.dg_ld != rec.rows else 0, wpacked=wpk, **kw)
        return dx

    def res_block(self, b: BlockSpec, xin, Hc, Wc, ln0: Optional[LnRows] = None, want_ln=None, elide=False):
        """ln0: LN(xin + m) if the producer of xin already emitted it; want_ln: the consumer's LayerNorm to emit from
        conv2's epilogue (see conv3).  Returns (block output, consumer's LN input or None).
        The chain form (round 6; training, 16-bit, 128-channel levels on the 16x16-tile kernel): ``xin`` None -- the previous block did
        not write its output; this block's residual is rebuilt inside conv2's epilogue from ln0's rows and statistics
        (x = h0 / rstd + mean - m); ``elide`` -- this block does not write ITS output either (returned as None): the next block of the
        side is its only reader besides the LayerNorm emitted here."""
        eng, tape, dt, ldm, train, dgrad = self.eng, self.tape, self.dt, self.ldm, self.train, self.dgrad
        p = "unet." + b.key
        Cc = b.channels
        npix = self.B * Hc * Wc
        m = self.m_all.view(-1)[b.mod_offset:]
        rstd0 = ln0.rstd if ln0 is not None else None
        if xin is None:
            assert rstd0 is not None and ln0.mean is not None, "chain form: the producer kept no LayerNorm statistics"
        if ln0 is not None:
            h0 = ln0.rows
        else:
            h0 = torch.empty((npix, Cc), dtype=self.T, device=self.dev)
            ops.ln_forward(xin, m, h0, npix, Hc * Wc, Cc, ldm, LN_EPS, eng.ln_unbiased, dt)
        # training: conv1's epilogue writes silu(a) for the next conv and silu'(a) for the backward pass; the pre-activation
        # itself is never stored
        d1 = torch.empty((npix, Cc), dtype=self.T, device=self.dev) if train else None
        act_inf, act_train = (ACT_RELU, ACT_RELU_PAIR) if self.lay.activation == "relu" else (ACT_SILU, ACT_SILU_PAIR)
        h1, g1, r1, _ = self.conv3(p + ".residue.1", h0, Hc, Wc, Hc, Wc, CONV_S1, act=act_train if train else act_inf, y2=d1)
        resn = dict(rstd=rstd0, mean=ln0.mean, m=m) if xin is None else None
        out, g2, r2, hn = self.conv3(p + ".residue.3", h1, Hc, Wc, Hc, Wc, CONV_S1, res=xin if xin is not None else h0, want_ln=want_ln,
                                     resn=resn, no_y=elide)
        if train:
            dm_all = self.dm_all

            def bw(gy):
                eng._wg(h1, gy, r2, g2, dt, group=True)
                da1 = dgrad(r2, gy, Hc, Wc, Hc, Wc, CONV_S1, Cc, mul=d1, mulmode=MUL_PLAIN)
                eng._wg(h0, da1, r1, g1, dt, group=True)
                dm = dm_all.view(-1)[b.mod_offset:]
                # conv1's input gradient feeds LN's backward directly: fused into the conv epilogue where the kernel
                # holds whole channel rows (128-channel levels in bf16), a separate pass otherwise
                if rstd0 is not None:  # the producer's epilogue kept the statistics: h0 = the normalised rows, rstd0 their 1/sigma
                    lnb = dict(x=h0, rstd=rstd0, m=None, dm=dm, ldm=ldm, eps=LN_EPS, unbiased=eng.ln_unbiased)
                else:
                    lnb = dict(x=xin, m=m, dm=dm, ldm=ldm, eps=LN_EPS, unbiased=eng.ln_unbiased)
                dx = dgrad(r1, da1, Hc, Wc, Hc, Wc, CONV_S1, Cc, res=gy, ln=lnb)
                if dx is None:
                    assert xin is not None, "chain form: the fused LayerNorm backward this block was built on is gone (knobs changed between forward and backward?)"
                    dh0 = dgrad(r1, da1, Hc, Wc, Hc, Wc, CONV_S1, Cc)
                    dx = torch.empty_like(dh0)
                    kw = eng._det_kw(("ln", npix, Hc * Wc, Cc, ldm), lambda: ops.ln_backward_det_scratch_bytes(npix, Hc * Wc, Cc, ldm))
                    ops.ln_backward(dh0, xin, m, gy, dx, dm, npix, Hc * Wc, Cc, ldm, LN_EPS, eng.ln_unbiased, dt, **kw)
                tape.done(r1.w_off)  # behind the block's last launch: "done" = gradients final AND weights (copies included) no longer read
                return dx
            tape.steps.append(bw)
        return out, hn

    def attn_block(self, b: BlockSpec, xin, Hc, Wc):
        eng, lay, tape, dt, T, dev, B, train = self.eng, self.lay, self.tape, self.dt, self.T, self.dev, self.B, self.train
        p = "unet." + b.key
        Cc = b.channels
        Tn = Hc * Wc
        npix = B * Tn
        rq, rp = lay.convs[p + ".qkv"], lay.convs[p + ".proj_out"]
        hl = torch.empty((npix, Cc), dtype=T, device=dev)
        ops.ln_forward(xin, None, hl, npix, Tn, Cc, 0, LN_EPS, eng.ln_unbiased, dt)
        qkv = torch.empty((npix, 3 * Cc), dtype=T, device=dev)
        gq = eng._geom(npix, 1, 1, Cc, 1, 1, 3 * Cc, 3 * Cc, 3 * Cc, CONV_1X1)
        ops.conv(hl, eng._w(rq, dt), eng._b(rq), qkv, gq, dt)
        o = torch.empty((npix, Cc), dtype=T, device=dev)
        lse = torch.empty((npix,), dtype=torch.float32, device=dev) if train else None
        ops.attention_forward(qkv, o, lse, B, Tn, Cc, dt)
        if eng.debug_trace is not None:
            eng.debug_trace += [(p + " qkv", qkv), (p + " attention", o)]
        out = torch.empty((npix, Cc), dtype=T, device=dev)
        gp = eng._geom(npix, 1, 1, Cc, 1, 1, Cc, Cc, Cc, CONV_1X1)
        ops.conv(o, eng._w(rp, dt), eng._b(rp), out, gp, dt, res=xin)
        if train:
            def bw(gy):
                eng._wg(o, gy, rp, gp, dt, group=True)  # the six proj_out / six qkv weight gradients of the level: one launch each
                do = torch.empty((npix, Cc), dtype=T, device=dev)
                ops.conv(gy, eng._wT(rp, dt), None, do, eng._geom(npix, 1, 1, Cc, 1, 1, Cc, Cc, Cc, CONV_1X1), dt)
                dqkv = torch.empty_like(qkv)
                delta = torch.empty((npix,), dtype=torch.float32, device=dev)
                ops.attention_backward(qkv, o, do, lse, delta, dqkv, B, Tn, Cc, dt)
                eng._wg(hl, dqkv, rq, gq, dt, group=True)
                dhl = torch.empty((npix, Cc), dtype=T, device=dev)
                ops.conv(dqkv, eng._wT(rq, dt), None, dhl, eng._geom(npix, 1, 1, 3 * Cc, 1, 1, Cc, Cc, Cc, CONV_1X1), dt)
                tape.done(rq.w_off)
                dx = torch.empty_like(dhl)
                ops.ln_backward(dhl, xin, None, gy, dx, None, npix, Tn, Cc, 0, LN_EPS, eng.ln_unbiased, dt)
                return dx
            tape.steps.append(bw)
        return out

    def mod_of(self, b: Optional[BlockSpec]):
        """what conv3's ``want_ln`` asks for when ``b`` consumes the conv's output: its modulated LayerNorm if it is a residual block"""
        return ("mod", self.m_all.view(-1)[b.mod_offset:]) if b is not None and b.kind == "res" else None

    def chain_ok(self, Cc, Hc, Wc) -> bool:
        """Do conv2's chain form (LayerNorm emitted with its mean, rebuilt residual, no output) and the next block's fused LayerNorm backward exist here?"""
        g = self.eng._geom(self.B, Hc, Wc, Cc, Hc, Wc, Cc, Cc, Cc, CONV_S1)
        return self.dt != DTYPE_F32 and ops.conv_lnfwd_chain_supported(g, self.dt) and ops.conv_lnbwd_supported(g, self.dt)

    def run_blocks(self, blocks, cur, Hc, Wc, hn: Optional[LnRows], tail_ln):
        """The blocks of one level side in order.  Each residual block asks its producer -- the previous block's second
        conv -- for its LayerNorm input; ``tail_ln`` is what the consumer after the last block wants.  Returns the
        output and that consumer's LN input (None if it was not fused)."""
        eng = self.eng

        def want_of(j):  # the LayerNorm block j's second conv emits for its consumer
            return self.mod_of(blocks[j + 1]) if j + 1 < len(blocks) else tail_ln
        for j, b in enumerate(blocks):
            if b.kind == "res":
                nb = blocks[j + 1] if j + 1 < len(blocks) else None
                # chain form: this block's output has no reader but the next block of the side (its LayerNorm comes out of this
                # block's conv2, its residual add can rebuild the sum) -- where the kernels exist, it is not written.  The rebuilding
                # lives in the LayerNorm-emitting epilogue, so the NEXT block's conv2 must emit one too (a side's last block does
                # only in front of an up-block)
                elide = self.train and eng.chain_blocks and nb is not None and nb.kind == "res" and \
                    want_of(j + 1) is not None and self.chain_ok(b.channels, Hc, Wc)
                cur, hn = self.res_block(b, cur, Hc, Wc, ln0=hn, want_ln=want_of(j), elide=elide)
            else:
                cur, hn = self.attn_block(b, cur, Hc, Wc), None
        return cur, hn

    def descend(self, x0, H, W) -> List[torch.Tensor]:
        """Head convs and descent sides of every level.  Returns the levels' outputs, top level first: the skip operands and, last, the
        deepest level's output (``ascend`` pops them; nobody else holds them)."""
        outs: List[torch.Tensor] = []
        Hc, Wc = H, W
        for i, lv in enumerate(self.lay.levels):
            cur, hn, Hc, Wc = self.head(i, lv, x0 if i == 0 else outs[-1], Hc, Wc)
            cur, _ = self.run_blocks(lv.descent, cur, Hc, Wc, hn, None)
            outs.append(cur)
        return outs

    def head(self, i, lv, xin, Hp, Wp):
        """Level i's head conv on xin (Hp x Wp): the network-input conv, which emits the first residual block's LayerNorm input from its
        epilogue like every block's second conv, or a stride-2 conv.  Returns (output, its LnRows or None, output grid)."""
        eng, tape, dt = self.eng, self.tape, self.dt
        if i == 0:
            Hc, Wc = Hp, Wp
            cur, g, rec, hn = self.conv3("unet." + lv.head_key, xin, Hp, Wp, Hc, Wc, CONV_S1, want_ln=self.mod_of(lv.descent[0] if lv.descent else None))
        else:
            Hc, Wc = Hp // 2, Wp // 2
            cur, g, rec, hn = self.conv3("unet." + lv.head_key, xin, Hp, Wp, Hc, Wc, CONV_S2)
        if self.train:
            def bw_head(gy):
                eng.flush_wgrad_groups()  # the level below is complete: its residual-block weight gradients go out together
                if i == 0:
                    eng._wgrad(rec, xin, gy, g, dt)
                    dx = self.dgrad(rec, gy, Hp, Wp, Hp, Wp, CONV_S1, self.lay.cin_pad) if self.want_dx else None
                else:
                    eng._wg(xin, gy, rec, g, dt)
                    # dx of the stride-2 conv + the gradient that arrived through the skip connection (model/nn.py:238)
                    dx = self.dgrad(rec, gy, Hc, Wc, Hp, Wp, CONV_TS2, rec.cin, res=tape.gskip.pop(i - 1))
                tape.done(rec.w_off)
                return dx
            tape.steps.append(bw_head)
        return cur, hn, Hc, Wc

    def ascend(self, outs: List[torch.Tensor], Hc, Wc):
        """Ascent sides and up-convs, deepest level first.  ``outs``: what ``descend`` returned, (Hc, Wc) the deepest grid.  Returns the
        top level's last block output (the output convolution's input)."""
        levels = self.lay.levels
        cur = outs.pop()
        h0_carry = None  # LN input of the level's first block when the up-conv below already produced it
        for i in reversed(range(len(levels))):
            cur, hl_ready = self.run_blocks(levels[i].ascent, cur, Hc, Wc, h0_carry, ("plain", None) if i > 0 else None)
            if i > 0:
                nxt = levels[i - 1].ascent[0] if levels[i - 1].ascent else None
                cur, h0_carry = self.up(i, levels[i], cur, hl_ready, outs.pop(), Hc, Wc, self.mod_of(nxt))
                Hc, Wc = Hc * 2, Wc * 2
        return cur

    def up(self, i, lv, xin, hl_ready: Optional[LnRows], skip, Hl, Wl, want_ln):
        """Level i's up-conv: LayerNorm (``hl_ready`` if the last block emitted it), conv on the upsampled rows + skip operand; it also emits
        the next level's first LayerNorm input (``want_ln``).  Returns (output on the doubled grid, its LnRows or None)."""
        eng, tape, dt, T, dev, B = self.eng, self.tape, self.dt, self.T, self.dev, self.B
        Cc = lv.channels
        npix = B * Hl * Wl
        if hl_ready is not None:
            hl = hl_ready.rows
        else:
            hl = torch.empty((npix, Cc), dtype=T, device=dev)
            ops.ln_forward(xin, None, hl, npix, Hl * Wl, Cc, 0, LN_EPS, eng.ln_unbiased, dt)
        Hu, Wu = Hl * 2, Wl * 2
        # Upsample(nearest, x2) is never materialised (model/nn.py:184): the halo-patch kernels fetch patch pixel (ih, iw) from
        # (ih >> 1, iw >> 1) of the low-resolution map (conv and weight gradient alike); grids they do not tile go to the gather
        # kernel, which folds the upsampling into its per-tap gather.
        cur, g, rec, hn = self.conv3("unet." + lv.tail_key, hl, Hl, Wl, Hu, Wu, CONV_UP, res=skip, want_ln=want_ln)
        if self.train:
            def bw_tail(gy):
                eng.flush_wgrad_groups()  # the ascent side of the level above is complete
                tape.gskip[i - 1] = gy  # the skip operand receives the same gradient
                eng._wg(hl, gy, rec, g, dt)
                # gradient w.r.t. the low-resolution map = 2x2 sums of the gradient w.r.t. its upsampling (adjoint of Upsample):
                # summed in the input-gradient kernel's epilogue where it supports that -- the full-resolution gradient is
                # then never written (537 MB at the top level) -- else a pooling pass behind it
                gd = eng._geom(B, Hu, Wu, rec.dg_ld, Hu, Wu, Cc, Cc, rec.cin, CONV_S1)
                gl = torch.empty((npix, Cc), dtype=T, device=dev)
                if ops.conv_pool2_supported(gd, dt):
                    wop, wpk = eng._conv_weights("d", rec, dt, gd)
                    ops.conv(gy, wop, None, gl, gd, dt, pool2=True, wpacked=wpk)
                else:
                    gu = self.dgrad(rec, gy, Hu, Wu, Hu, Wu, CONV_S1, Cc)
                    ops.sumpool2(gu, gl, B, Hl, Wl, Cc, dt)
                dx = torch.empty_like(gl)
                ops.ln_backward(gl, xin, None, None, dx, None, npix, Hl * Wl, Cc, 0, LN_EPS, eng.ln_unbiased, dt)
                tape.done(rec.w_off)
                return dx
            tape.steps.append(bw_tail)
        return cur, hn

    def output(self, xin, H, W, fold, loss, loss_rows):
        """The output convolution on the top level's rows: the sampler's fold shortcut (returns None: the trajectories were written), the
        fused loss tail (``loss_rows``: what to_nhwc kept), or the plain conv.  Returns the NHWC output rows."""
        eng, lay, tape = self.eng, self.lay, self.tape
        lv = lay.levels[0]
        if fold is not None and not self.train and eng._fold_output(fold, "unet." + lv.tail_key, xin, self.B, H, W, self.dt):
            return None
        lfuse = None
        if loss_rows is not None:
            lfuse = dict(sum=loss["sum"], gscale=loss["gscale"], scaler=loss.get("scaler"), eps=loss_rows[0], lde=loss_rows[1], C=lay.out_channels)
        cur, g, rec, _ = self.conv3("unet." + lv.tail_key, xin, H, W, H, W, CONV_S1, ldy=lay.cout_pad, cout=lay.cout_pad, loss=lfuse)
        if self.train:
            tape.meta["loss_fused"] = lfuse is not None
            Cc = lv.channels

            def bw_tail0(gy):
                gw = dict(g)
                gw["Cout"] = rec.rows
                eng._wg(xin, gy, rec, gw, self.dt)
                dxt = self.dgrad(rec, gy, H, W, H, W, CONV_S1, Cc)
                tape.done(rec.w_off)
                return dxt
            tape.steps.append(bw_tail0)
        return cur
