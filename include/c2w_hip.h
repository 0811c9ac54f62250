/* c2w_hip.h -- C ABI of libc2w_hip.so, the MI355X (gfx950) kernel library under
 * climate2weather_amd.
 *
 * The reference (schmidtjonathan/Climate2Weather) is pure Python and has no FFI:
 * its hot path dispatches torch ops.  Each entry point below names
 * the reference call sites whose arithmetic it replaces.  Conventions:
 *   - caller owns every buffer (device pointers from the caller's allocator); nothing is
 *     allocated, freed or synchronised inside; work is enqueued on `stream` (a hipStream_t);
 *   - activations are NHWC: [B][H][W][ld] with `ld` the channel stride in elements;
 *   - `dtype` selects the storage/MFMA-operand type: C2W_DTYPE_F32 (exact fp32 matrix-core
 *     path, the <=1e-4 parity mode), C2W_DTYPE_BF16 (throughput mode) or C2W_DTYPE_F16 (IEEE half, the type the
 *     reference's Fabric "16-mixed" autocast computes in, train.py:98: same kernels and layouts as bf16 with the f16
 *     matrix-core opcode; its narrow range needs the loss scale of c2w_grad_scaler_* in training); accumulation and all
 *     pointwise math are fp32 in all three;
 *   - return value: 0 on success, a positive hipError_t, or a negative C2W_ERR_* code.
 *     Nothing throws across this boundary.
 */
#ifndef C2W_HIP_H
#define C2W_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { C2W_DTYPE_F32 = 0, C2W_DTYPE_BF16 = 1, C2W_DTYPE_F16 = 2 };
enum { C2W_ERR_BAD_ARG = -1, C2W_ERR_BAD_SHAPE = -2, C2W_ERR_UNSUPPORTED = -3 };

/* geometry of the implicit GEMM */
enum {
    C2W_CONV_1X1 = 0, /* Linear / Conv1d(k=1): model/nn.py:45,47,149; model/score.py:56-57 */
    C2W_CONV_S1 = 1,  /* Conv2d 3x3 stride 1 pad 1: model/nn.py:155,157,193-194 (and its dgrad with flipped weights) */
    C2W_CONV_S2 = 2,  /* Conv2d 3x3 stride 2 pad 1: model/nn.py:169-174 */
    C2W_CONV_UP = 3,  /* Upsample(nearest,x2) -> Conv2d 3x3: model/nn.py:184-189, upsample folded into the gather */
    C2W_CONV_TS2 = 4  /* input-gradient of C2W_CONV_S2 (x := dy, y := dx) */
};
/* C2W_ACT_SILU_PAIR (training): with a = the conv result as stored, y = silu(a) and y2 = silu'(a) -- the activation the next
 * conv reads and the factor the backward pass multiplies by (model/nn.py:156 forward/backward), so the pre-activation itself
 * is never written and the backward epilogue needs no transcendental. */
/* C2W_ACT_RELU / C2W_ACT_RELU_PAIR: the same for torch.nn.ReLU, the default `activation` of the reference's UNet (model/nn.py:118):
 * y = max(a, 0), y2 = (a > 0) -- the backward pass multiplies by y2 with C2W_MUL_PLAIN. */
enum { C2W_ACT_NONE = 0, C2W_ACT_SILU = 1, C2W_ACT_SILU_PAIR = 2, C2W_ACT_RELU = 3, C2W_ACT_RELU_PAIR = 4 };
enum { C2W_MUL_PLAIN = 0, C2W_MUL_DSILU = 1 };
enum { C2W_CONV_POOL2 = 1, C2W_CONV_WPACKED = 2, C2W_CONV_NO_Y = 4, C2W_CONV_DETERMINISTIC = 8 }; /* C2wConvArgs.flags (bit set) */
/* Deterministic mode (opt-in, per call; the library keeps no mode state).  Most of a training step is bit-reproducible run to run
 * as it is; the bias gradients, the LayerNorm modulation gradients and the loss scalar are summed with fp32 atomics whose order the
 * hardware picks.  With C2W_CONV_DETERMINISTIC set in C2wConvArgs.flags (c2w_conv_wgrad, c2w_conv_wgrad_grouped, c2w_conv_forward with
 * a fused LayerNorm backward or loss) and through the c2w_*_det siblings of the pointwise launchers, every workgroup that would issue
 * such an atomic STORES its contribution into a slot of a caller-owned fp32 scratch -- the slot a pure function of the launch
 * geometry, every slot read is written by the same call, nothing is zero-filled -- and a small launch behind it on the same stream
 * adds the slots onto the destination (still accumulated into) in a fixed order.  Same arguments, same knob settings => same bits.
 * Every other output of the call is bit-identical to the default mode's; the reduced values differ from it in summation order only.
 * A missing or short scratch is C2W_ERR_BAD_ARG, never a fall-back to atomics.  One scratch per stream (contents undefined before
 * and after a call), like c2w_conv_wgrad's workspace. */

/* y[q][co] = act( sum_{tap,ci} w[co][tap][ci] * x[src(q,tap)][ci] + bias[co] ) (* mul' ) (+ res)
 * q runs over the B*Hout*Wout output pixels in NHWC raster order.
 *
 * Geometry the launchers take (c2w_conv_forward, c2w_conv_wgrad and its siblings; anything else is C2W_ERR_BAD_SHAPE, before a launch):
 *   - Cout <= ldy.  A row of y, y2, res, mul (and of dY) holds ldy channels of which the first Cout are live: the columns [Cout, ldy) of
 *     every output are left untouched, and what the inputs hold there is never used.
 *   - The output grid is the mode's function of the input grid, per axis: Hout == Hin for C2W_CONV_1X1 and C2W_CONV_S1; (Hin + 1) / 2 or
 *     Hin / 2 for C2W_CONV_S2; 2 * Hin for C2W_CONV_UP; 2 * Hin - 1 or 2 * Hin for C2W_CONV_TS2 (the two input sizes a stride-2 conv
 *     maps to Hin) -- and the same for Wout from Win.  No other grid has a definition: the gather would walk into the next image.
 * The kernels take every zero they need (halos, weight rows >= wrows, the bias tail, the missing partner of an odd batch) from the range
 * check of buffer descriptors built from exactly these sizes: nothing outside an operand is ever read into a result.
 * Alignment is a precondition the launchers do NOT verify: every operand pointer (x, w, res, mul, y, y2, dY, dw, the workspaces) must be
 * 16-byte aligned -- nothing stronger is asked for; bias and dbias are read and written as single floats. */
typedef struct C2wConvArgs {
    const void* x;     /* [B][Hin][Win][Cin]  (Cin = channel stride; multiple of 32 (f32) / 64 (bf16)) */
    const void* w;     /* [wrows][taps][Cin], taps = 1 or 9 (kh*3+kw); rows >= wrows read as zero */
    const float* bias; /* [wrows] fp32 or NULL */
    const void* res;   /* [B*Hout*Wout][ldy] added last, or NULL   (residual / skip: model/nn.py:28,238) */
    const void* mul;   /* [B*Hout*Wout][ldy] or NULL: y *= mul (C2W_MUL_PLAIN) or y *= silu'(mul) (C2W_MUL_DSILU) */
    void* y;           /* [B*Hout*Wout][ldy] */
    void* y2;          /* optional second output [B*Hout*Wout][ldy]: silu(y) (training keeps the pre-activation too) */
    int32_t B, Hin, Win, Cin;
    int32_t Hout, Wout, Cout, ldy;
    int32_t wrows;
    int32_t mode;    /* C2W_CONV_* */
    int32_t act;     /* C2W_ACT_* */
    int32_t mulmode; /* C2W_MUL_* */
    /* Optional fused LayerNorm backward (see c2w_conv_lnbwd_supported): with ln_x != NULL the conv result g is not stored;
     * instead y = res + dLN(g; ln_x + ln_m[b]) and ln_dm[b][c] += sum over the image's pixels of the LN part -- exactly
     * c2w_ln_backward(dy = g, x = ln_x, m = ln_m, dres = res, dx = y, dm = ln_dm) applied to the conv's output tile while
     * it is still on chip (model/nn.py:28,154 backward: the input gradient of conv1 feeds LN's backward directly). */
    const void* ln_x;   /* [B*Hout*Wout][ldy] LN input rows (the block input), or NULL = no fusion */
    const float* ln_m;  /* [B][ln_ldm] fp32 modulation rows added to ln_x before the norm, or NULL */
    float* ln_dm;       /* [B][ln_ldm] fp32 modulation gradient, accumulated (atomics), or NULL */
    int32_t ln_ldm;
    int32_t ln_unbiased;
    float ln_eps;
    int32_t flags;      /* C2W_CONV_POOL2: y is [B][Hout/2][Wout/2][ldy] and receives the 2x2 SUMS of the result -- the adjoint of
                         * Upsample(nearest, x2) (model/nn.py:184) applied to the input gradient of the conv behind it, on chip: the
                         * full-resolution gradient is never written (see c2w_conv_pool2_supported) */
                        /* C2W_CONV_WPACKED: w is the stage-major copy c2w_pack_conv_weights_batched makes ([tap][Cin / 32][rows padded to 128][32 ci],
                         * 8 KiB per K stage of the 16x16-tile kernel in one piece); accepted only where c2w_conv_wpacked_supported says so */
    /* Optional fused LayerNorm FORWARD of the consumer (see c2w_conv_lnfwd_supported): with lnf_y != NULL the kernel also
     * writes lnf_y = LN_C(y + lnf_m[b]) -- c2w_ln_forward(x = y as stored, m = lnf_m, ldm = ln_ldm, eps = ln_eps,
     * unbiased = ln_unbiased) -- i.e. the next residual block's normalised input (model/nn.py:28,154) leaves the conv that
     * produced the block input, without a separate pass over it. */
    void* lnf_y;        /* [B*Hout*Wout][ldy] or NULL */
    const float* lnf_m; /* [B][ln_ldm] fp32 modulation rows of the CONSUMER block, or NULL (plain LayerNorm) */
    /* Optional promise about channel padding: 0, or the number of leading input channels that can be non-zero -- channels kvalid..Cin-1
     * of x (or of w) are ALL ZERO (the network-input conv at C = 65 reads rows padded to 128 channels, model/nn.py:193; the input
     * gradient of the output conv reads a gradient whose padding channels are zero, :194).  Kernels may skip the multiplications
     * the promise makes void (conv_patch_t3_kernel: whole 32-channel half chunks); results are unchanged. */
    int32_t kvalid;
    /* Optional per-pixel statistics of the fused LayerNorms (16-bit launches; both NULL: rounds 1-4 behaviour):
     *   lnf_rstd (with lnf_y): the forward also writes 1/sqrt(var + eps) of every pixel row it normalises, [B*Hout*Wout] fp32;
     *   ln_rstd (with ln_x): the backward is handed what the forward kept -- ln_x then holds the NORMALISED rows (the lnf_y the
     *   forward wrote = the conv input of model/nn.py:155, which training keeps anyway) and ln_rstd their 1/sigma; ln_m is not
     *   read.  dLN = rstd * (g - mean(g) - xhat * sum(g * xhat) / den) needs neither the mean nor the variance again: two of the
     *   four 16-lane reductions per pixel row and the modulation add leave the epilogue (model/nn.py:28,154 backward). */
    float* lnf_rstd;
    const float* ln_rstd;
    /* Optional, with lnf_y (round 6; see c2w_conv_lnfwd_chain_supported) -- a chain of residual blocks (model/nn.py:27-28,146-159) whose
     * intermediate outputs are never written: block k's second conv reads its residual x_k, adds its result, and emits the next
     * block's normalised input h_{k+1} = LN(x_{k+1} + m_{k+1}) together with that LayerNorm's per-pixel mean and 1/sigma; x_{k+1} itself
     * is read by nothing but block k+1's residual add, which can rebuild it from what was emitted:  x = h / rstd + mean - m.
     *   lnf_mean:  [B*Hout*Wout] fp32, the mean of every pixel row this launch normalises (next to lnf_rstd), or NULL;
     *   res_rstd, res_mean, res_m (all or none): `res` holds NORMALISED rows h = LN(x + res_m[b]) (an earlier launch's lnf_y) and these
     *     are that LayerNorm's lnf_rstd / lnf_mean and its modulation rows (stride ln_ldm, NULL = none): the residual added is
     *     h / res_rstd + res_mean - res_m[b];
     *   flags & C2W_CONV_NO_Y: y is not written (pass any valid pointer); lnf_y then normalises the fp32 sum instead of its 16-bit
     *     rounding.  537 MB less per launch at 128 channels x 128^2 x 128 windows. */
    float* lnf_mean;
    const float* res_rstd;
    const float* res_mean;
    const float* res_m;
    /* Optional fused training loss (round 6; see c2w_conv_loss_supported): with loss_sum != NULL the conv result itself is not
     * stored.  Instead, with eps = the noise rows loss_eps ([B*Hout*Wout][loss_lde] IEEE half, NHWC like y; written by
     * c2w_nchw_to_nhwc_noise_rows next to the noised input they were mixed into) and a = the result rounded to the storage type,
     * loss_sum += sum (a - eps)^2 over the loss_C real channels and y = (a - eps) * loss_gscale [* loss_scaler[0]] (channels >=
     * loss_C: zero) -- c2w_mse_loss_grad applied to the network-output conv's tile while it is still on chip
     * (src/thor/pipelines.py:35, training_loop.py:376-377: the loss and the gradient the backward pass starts from; the prediction
     * is used by nothing else in a training step). */
    float* loss_sum;          /* one fp32, accumulated (atomics), or NULL = no fusion */
    const float* loss_scaler; /* device-resident loss scale (fp16 training, c2w_grad_scaler_*) or NULL */
    const void* loss_eps;     /* half rows, channels loss_C .. loss_lde-1 zero */
    float loss_gscale;
    int32_t loss_C;
    int32_t loss_lde;         /* channel stride of loss_eps: a multiple of 8, loss_C <= loss_lde <= 128 */
    /* Optional split-K (round 6; c2w_conv_splitk_plan): splitk > 1 deals every output tile's K chunks to that many workgroups; their fp32
     * partial tiles go through the caller's scratch splitk_ws (splitk_ws_bytes >= what the plan asked for; contents undefined before and
     * after; one buffer per stream, like c2w_conv_wgrad's workspace) and a second launch on the same stream adds them in a fixed order
     * and applies bias / activation / mul / res.  For launches of fewer workgroups than the chip has CUs (the deep levels of a
     * sampler step on a short trajectory, exp/configs/000_on-model-eval/s16_t6.yml: 37 windows): such a launch costs its chain of K
     * stages whatever it carries.  Results are bit-reproducible; they differ from the unsplit launch in summation order only. */
    float* splitk_ws;
    unsigned long long splitk_ws_bytes;
    int32_t splitk;           /* 0 / 1: no split; else exactly c2w_conv_splitk_plan's answer for these arguments */
    /* Deterministic mode of c2w_conv_forward (flags & C2W_CONV_DETERMINISTIC with ln_dm or loss_sum): the scratch the fused epilogue's
     * per-workgroup sums go through, at least c2w_conv_det_scratch_bytes() of it. */
    float* det_ws;
    unsigned long long det_ws_bytes;
} C2wConvArgs;

/* 1 when c2w_conv_forward / c2w_conv_wgrad run this geometry on the halo-patch kernels (3x3 stride-1, image tiled exactly
 * by 8 x 16-pixel tiles), 0 when it takes the general gather kernels. */
int c2w_conv_patch_supported(const C2wConvArgs* args, int dtype);
/* 1 when c2w_conv_forward can store the 2x2-pooled result (flags & C2W_CONV_POOL2): halo-patch geometry, stride 1, no
 * res / mul / y2 / activation / LayerNorm fusion.  Otherwise callers run the conv and c2w_sumpool2. */
int c2w_conv_pool2_supported(const C2wConvArgs* args, int dtype);
/* 1 when c2w_conv_forward can also emit the consumer's LayerNorm (lnf_y): same shape conditions as the backward fusion,
 * residual allowed. */
int c2w_conv_lnfwd_supported(const C2wConvArgs* args, int dtype);
/* 1 when c2w_conv_forward can run args with the fused LayerNorm backward (bf16, Cout == ldy == 128, 3x3 stride-1 on an
 * image the halo-patch kernel tiles, no mul / act / y2), else 0.  Callers fall back to conv + c2w_ln_backward. */
int c2w_conv_lnbwd_supported(const C2wConvArgs* args, int dtype);
/* 1 when c2w_conv_forward takes lnf_mean / res_rstd + res_mean + res_m / C2W_CONV_NO_Y for this geometry (c2w_conv_lnfwd_supported's
 * conditions on the 16x16-tile kernel).  Elsewhere those fields make the call fail with C2W_ERR_BAD_SHAPE. */
int c2w_conv_lnfwd_chain_supported(const C2wConvArgs* args, int dtype);
/* 1 when c2w_conv_forward can run args with the fused training loss (loss_sum / loss_eps / loss_gscale / loss_C / loss_lde): 16-bit,
 * 3x3 stride-1 on the 16x16-tile kernel, at most 80 weight rows in rows of 128 channels (the network-output conv, model/nn.py:194),
 * loss_C == wrows (the epilogue takes every channel below loss_lde into the loss: channels [wrows, loss_lde) are zero in the tile and in
 * loss_eps, channels [loss_C, wrows) would not be), no res / mul / act / y2 / LayerNorm fusion.  Otherwise callers run the conv and
 * c2w_mse_loss_grad[_noise]. */
int c2w_conv_loss_supported(const C2wConvArgs* args, int dtype);
/* Workgroups per output tile c2w_conv_forward can deal the K chunks of these arguments to (1: no split -- geometry outside the 8x16-tile
 * kernels, fused epilogues other than bias / activation / mul / res, or a launch that already has a workgroup per CU), and through
 * *ws_bytes (may be NULL) the scratch it then needs.  A pure function of the arguments' geometry, epilogue fields and the dtype. */
int c2w_conv_splitk_plan(const C2wConvArgs* args, int dtype, unsigned long long* ws_bytes);
/* Bytes of det_ws c2w_conv_forward needs for these arguments under C2W_CONV_DETERMINISTIC (0: no fused reduction in this call), or a
 * negative C2W_ERR_* status.  A pure function of the arguments' geometry, fusion fields and the dtype. */
long long c2w_conv_det_scratch_bytes(const C2wConvArgs* args, int dtype);

/* Which kernel family c2w_conv_forward (naive == 0) / c2w_conv_wgrad run these arguments on -- a pure function of the geometry,
 * the dtype and the fusion fields; the parity tests assert with it that a case reaches the kernel it is meant to cover.
 * GATHER: conv_igemm / wgrad gather kernels; PATCH_8X16: conv_patch_half_kernel / wgrad_patch_kernel; PATCH_16X16:
 * conv_patch_t3_kernel<16> (16-bit launches of >= 512 workgroups of that tile); PATCH_PAIR: 8-pixel-wide images, two per tile; PATCH_TS2: the
 * stride-2 input gradient per output-parity class; PATCH_S2: the stride-2 FORWARD on the parity planes of the halo patch (16-bit; output
 * tiled by 8x16 pixels, or 8 pixels wide with two images per tile; only with C2W_CONV_S2_PATCH=1, from four K chunks on or up to 2048 workgroups, or =2, wherever the geometry allows). */
enum { C2W_KERNEL_GATHER = 0, C2W_KERNEL_PATCH_8X16 = 1, C2W_KERNEL_PATCH_16X16 = 2, C2W_KERNEL_PATCH_PAIR = 3, C2W_KERNEL_PATCH_TS2 = 4, C2W_KERNEL_PATCH_S2 = 5 };
int c2w_conv_dispatch(const C2wConvArgs* args, int dtype);
int c2w_conv_wgrad_dispatch(const C2wConvArgs* args, int dtype);

/* naive == 0: product path (halo-patch MFMA kernel for 3x3 stride-1 on 16x16-tileable images, general gather MFMA
 * kernel otherwise); naive == 2: force the gather MFMA kernel; naive == 1: one-thread-per-output direct convolution
 * with identical semantics (debug cross-check only). */
int c2w_conv_forward(const C2wConvArgs* args, int dtype, int naive, void* stream);

/* dW[co][tap][ci] (fp32) += sum_q dY[q][co] * x[src(q,tap)][ci]  -- weight gradient of the same geometry.
 * Pass the forward call's block with y := dY; w/bias/res/mul/act are ignored.  The reduction over pixels is split across
 * workgroups: zero dw (or leave the value to accumulate onto) beforehand.
 * dbias (may be NULL): [Cout] fp32, += sum_q dY[q][co] (the bias gradient, from the same pass over dY).
 * workspace / workspace_bytes: caller-owned device scratch (16-byte aligned) for the split's partial sums, handed over PER CALL --
 * the library keeps no pointer, so the entry point is re-entrant: with it the workgroups store their partial tiles and a second
 * launch on the same stream reduces them in a fixed order (75 MB of coalesced stores + reads per launch instead of 75 MB of fp32
 * atomics; dw is then bit-reproducible run to run -- dbias only with args->flags & C2W_CONV_DETERMINISTIC: by default every split workgroup adds its
 * column sums with fp32 atomics; with the flag the workgroups' bias rows ride behind the partial tiles in the same workspace and a
 * sibling of the reduce launch adds them in split order, or, without a split, one workgroup per channel updates dbias by plain
 * read-modify-write); NULL, or fewer bytes than c2w_conv_wgrad_workspace_bytes() asks for: fp32 atomics -- under the flag
 * C2W_ERR_BAD_ARG instead, as is C2W_WGRAD_ATOMICS=1.
 * Contents are undefined before and after the call.  One buffer must not be handed to launches that may run concurrently
 * (different streams without an ordering between them): give each stream its own.
 * Replaces autograd's weight/bias backward of every Conv2d/Conv1d/Linear cited above. */
int c2w_conv_wgrad(const C2wConvArgs* args, float* dw, float* dbias, void* workspace, unsigned long long workspace_bytes, int dtype,
                   void* stream);
/* Scratch bytes c2w_conv_wgrad uses for this geometry and dtype (0: no split), or a negative C2W_ERR_* status.  With
 * args->flags & C2W_CONV_DETERMINISTIC: including the bias rows. */
long long c2w_conv_wgrad_workspace_bytes(const C2wConvArgs* args, int dtype);

/* The weight gradients of n layers that share ONE geometry (`args`: the forward block of any of them; x / y are ignored) as one launch:
 * items[i] = {x, dy, dw, dbias} of layer i, each with the meaning c2w_conv_wgrad gives them (dw, dbias accumulated into).  The
 * residual-block convs of a UNet level (model/nn.py:146-159: 6 or 12 layers of one shape) have their output gradients one after the
 * other during the backward pass and independent weight gradients; a launch per layer must split its pixel reduction over the whole
 * chip (at 8x8: 8 K tiles per workgroup, each followed by 295 KB of partial sums), together the layers fill it with a fraction of
 * the splits.  `items` is a HOST array, copied into the kernel arguments (nothing is kept).  The dw results are deterministic (a fixed reduction order; dbias too with
 * args->flags & C2W_CONV_DETERMINISTIC, by default fp32 atomics across the split workgroups: last-bit order noise) but differ in rounding from n single calls (another split of the same sum).
 * c2w_conv_wgrad_grouped_supported: 1 when the n layers run as one launch (2 <= n <= 16; the halo-patch geometries on
 * wgrad_patch_group_kernel, 1x1 layers -- the attention level's qkv / proj_out, model/nn.py:45,47 -- on wgrad_group_kernel); otherwise
 * the call returns C2W_ERR_UNSUPPORTED and the caller issues n c2w_conv_wgrad calls.  workspace must hold
 * c2w_conv_wgrad_grouped_workspace_bytes(args, n, dtype) bytes (0 when the plan does not split; more under C2W_CONV_DETERMINISTIC). */
typedef struct C2wWgradItem {
    const void* x;
    const void* dy;
    float* dw;
    float* dbias; /* may be NULL */
} C2wWgradItem;
int c2w_conv_wgrad_grouped_supported(const C2wConvArgs* args, int n, int dtype);
long long c2w_conv_wgrad_grouped_workspace_bytes(const C2wConvArgs* args, int n, int dtype);
int c2w_conv_wgrad_grouped(const C2wConvArgs* args, const C2wWgradItem* items, int n, void* workspace, unsigned long long workspace_bytes,
                           int dtype, void* stream);

/* y = LN_C(x + m[b]): parameter-free channel LayerNorm (zuko.nn.LayerNorm at model/nn.py:44,154,183) fused with
 * the time-modulation add of model/nn.py:28.  x,y: [npix][C]; m: fp32 rows of C (row b = pixel / HW, stride ldm;
 * ldm == 0 -> one row shared by every pixel; m == NULL -> no add).  unbiased selects the N-1 variance. */
int c2w_ln_forward(const void* x, const float* m, void* y, long long npix, int HW, int C, int ldm, float eps,
                   int unbiased, int dtype, void* stream);
/* dx = dres + dLN(dy; x+m);  dm[b][c] += sum over the image's pixels of the LN part (fp32 atomics: c2w_ln_backward_det for a fixed
 * order; dm may be NULL). */
int c2w_ln_backward(const void* dy, const void* x, const float* m, const void* dres, void* dx, float* dm,
                    long long npix, int HW, int C, int ldm, float eps, int unbiased, int dtype, void* stream);
/* Deterministic mode: the same with dm summed in a fixed order through `scratch` (>= c2w_ln_backward_det_scratch_bytes(); not read
 * when dm == NULL); dx is bit-identical to c2w_ln_backward's. */
int c2w_ln_backward_det(const void* dy, const void* x, const float* m, const void* dres, void* dx, float* dm,
                        long long npix, int HW, int C, int ldm, float eps, int unbiased, float* scratch, unsigned long long scratch_bytes,
                        int dtype, void* stream);
long long c2w_ln_backward_det_scratch_bytes(long long npix, int HW, int C, int ldm);

/* out[c] += sum_rows a[row][c]   (bias gradients; fp32 atomics) */
int c2w_colsum(const void* a, float* out, long long rows, int C, int lda, int dtype, void* stream);
/* Deterministic mode: a fixed summation order through `scratch` (>= c2w_colsum_det_scratch_bytes(rows, C)) */
int c2w_colsum_det(const void* a, float* out, long long rows, int C, int lda, float* scratch, unsigned long long scratch_bytes, int dtype,
                   void* stream);
long long c2w_colsum_det_scratch_bytes(long long rows, int C);
/* y = silu(x) ; dx = dy * silu'(x)   (the activation train.py:171 passes; model/nn.py:156, model/score.py:63,67) */
int c2w_silu(const void* x, void* y, long long n, int dtype, void* stream);
int c2w_silu_backward(const void* x, const void* dy, void* dx, long long n, int dtype, void* stream);
/* adjoint of Upsample(nearest, x2) (model/nn.py:184): dx[b][h][w] = sum of the 2x2 block of g ([B][2H][2W][C]) */
int c2w_sumpool2(const void* g, void* dx, int B, int H, int W, int C, int dtype, void* stream);

/* Upsample(nearest, x2) (model/nn.py:184) on NHWC rows: y[b][2h+i][2w+j] = x[b][h][w] */
int c2w_upsample2(const void* x, void* y, int B, int H, int W, int C, int dtype, void* stream);
/* NCHW fp32 <-> NHWC (padded to ldc channels).  With eps != NULL the forward noise process of
 * src/thor/pipelines.py:22-25 is fused: y = mu[b] x + sigma[b] eps, musig = {mu_0, sigma_0, mu_1, ...}. */
int c2w_nchw_to_nhwc(const float* x, const float* eps, const float* musig, void* y, int B, int C, int HW, int ldc,
                     int dtype, void* stream);
int c2w_nhwc_to_nchw(const void* y, float* out, int B, int C, int HW, int ldc, int dtype, void* stream);
/* c2w_nchw_to_nhwc_noise (below) that also KEEPS the noise it mixed in: erows [B*HW][lde] IEEE half (lde = a multiple of 8 >= C,
 * channels C .. lde-1 zero) receives eps rounded to half precision, and y = mu x + sigma * (that rounded value) -- the step's noise IS
 * the rounded stream, so the loss tail (C2wConvArgs.loss_eps) reads back exactly what the input was noised with instead of running
 * Philox + Box-Muller a second time (0.2 ms of VALU work per 128 windows).  img_off (may be NULL): as in c2w_windows_to_nhwc_noise.
 * HW % 4 == 0.  C2W_ERR_UNSUPPORTED: shape outside the kernel (callers fall back to the *_noise pair). */
int c2w_nchw_to_nhwc_noise_rows(const float* x, const long long* img_off, unsigned long long seed, const float* musig, void* y, void* erows,
                                int B, int C, int HW, int ldc, int lde, int dtype, void* stream);
/* loss tail (src/thor/pipelines.py:35, training_loop.py:377): loss_sum += sum (y-eps)^2 ; dy = (y-eps) * gscale */
int c2w_mse_loss_grad(const void* y, const float* eps, void* dy, float* loss_sum, int B, int C, int HW, int ldc,
                      float gscale, int dtype, void* stream);
/* same with dy additionally multiplied by the device-resident loss scale scaler_state[0] (NULL = 1): fp16 training */
int c2w_mse_loss_grad_scaled(const void* y, const float* eps, void* dy, float* loss_sum, int B, int C, int HW, int ldc,
                             float gscale, const float* scaler_state, int dtype, void* stream);
/* Regenerated noise.  The training step's eps = randn_like(x) (src/thor/pipelines.py:22-25) is consumed twice -- by the forward
 * process x_t = mu x + sigma eps and by the loss (eps_pred - eps)^2 -- and nowhere else.  A counter-based generator (Philox4x32-10 on
 * the index of a block of four consecutive elements, Box-Muller) lets both kernels compute eps[e] instead of reading it:
 *   c2w_philox_normal        out[e] = N(0,1) stream of `seed`                                 (tests; fallback for shapes the fused
 *                                                                                             kernels do not take)
 *   c2w_nchw_to_nhwc_noise   c2w_nchw_to_nhwc with eps := that stream (element index = NCHW linear index)
 *   c2w_mse_loss_grad_noise  c2w_mse_loss_grad_scaled with eps := that stream
 * Same seed => bit-identical eps in all three.  C2W_ERR_UNSUPPORTED: channel rows too wide for the LDS tile (use the fallback). */
int c2w_philox_normal(float* out, long long n, unsigned long long seed, void* stream);
int c2w_nchw_to_nhwc_noise(const float* x, unsigned long long seed, const float* musig, void* y, int B, int C, int HW, int ldc,
                           int dtype, void* stream);
/* The same with the B images picked out of a dataset array: image b is the C*HW contiguous floats at data + img_off[b] (a window of
 * consecutive frames: dataset.py:114-126; img_off[b] a multiple of 4).  The noise stream is addressed with the dense (B,C,H,W) index,
 * so the result equals c2w_nchw_to_nhwc_noise on the gathered batch bit for bit -- the batch tensor itself is never written. */
int c2w_windows_to_nhwc_noise(const float* data, const long long* img_off, unsigned long long seed, const float* musig, void* y, int B, int C,
                              int HW, int ldc, int dtype, void* stream);
int c2w_mse_loss_grad_noise(const void* y, unsigned long long seed, void* dy, float* loss_sum, int B, int C, int HW, int ldc,
                            float gscale, const float* scaler_state, int dtype, void* stream);
/* The UNREDUCED loss tensor src/thor/pipelines.py:35 returns, `(eps_pred - eps) ** 2` (the caller takes .mean(), training_loop.py:377),
 * for the module path: out[b][c][px] (NCHW fp32) = (y[b][px][c] - eps[b][c][px])^2 from the network's NHWC output rows; eps read
 * from memory (c2w_sq_err) or regenerated from the step's stream (c2w_sq_err_noise); loss_sum (optional) += the sum of `out`, so
 * the caller's mean costs no second pass.  C2W_ERR_UNSUPPORTED: HW % 4 != 0 or rows too wide for the LDS tile (caller converts the
 * layout and uses tensor arithmetic). */
int c2w_sq_err(const void* y, const float* eps, float* out, float* loss_sum, int B, int C, int HW, int ldc, int dtype, void* stream);
int c2w_sq_err_noise(const void* y, unsigned long long seed, float* out, float* loss_sum, int B, int C, int HW, int ldc, int dtype,
                     void* stream);
/* Deterministic mode of the loss launchers: loss_sum += the waves' sums in a fixed order through `scratch` (>= c2w_loss_det_scratch_bytes(),
 * one size for all of them); dy / out are bit-identical to the default launchers'.  c2w_mse_loss_grad_det covers c2w_mse_loss_grad and
 * c2w_mse_loss_grad_scaled (scaler_state may be NULL). */
long long c2w_loss_det_scratch_bytes(void);
int c2w_mse_loss_grad_det(const void* y, const float* eps, void* dy, float* loss_sum, int B, int C, int HW, int ldc, float gscale,
                          const float* scaler_state, float* scratch, unsigned long long scratch_bytes, int dtype, void* stream);
int c2w_mse_loss_grad_noise_det(const void* y, unsigned long long seed, void* dy, float* loss_sum, int B, int C, int HW, int ldc,
                                float gscale, const float* scaler_state, float* scratch, unsigned long long scratch_bytes, int dtype,
                                void* stream);
int c2w_sq_err_det(const void* y, const float* eps, float* out, float* loss_sum, int B, int C, int HW, int ldc, float* scratch,
                   unsigned long long scratch_bytes, int dtype, void* stream);
int c2w_sq_err_noise_det(const void* y, unsigned long long seed, float* out, float* loss_sum, int B, int C, int HW, int ldc, float* scratch,
                         unsigned long long scratch_bytes, int dtype, void* stream);
/* Held-out validation: the same squared error resolved by noise-level bin x output channel, never written as a (B,C,H,W) tensor.
 *   table[bin(t_b)][c] (double [K][C])  += sum over the pixels of image b of (y[b][px][c] - eps[b][c][px])^2,  c < C only (the padding
 *                                          channels C .. ldc-1 of the rows are never read into a sum)
 *   count[bin(t_b)]    (int64 [K])      += 1 per image
 *   per_image[b]       (fp32 [B], may be NULL) = the image's sum over its C channels
 * table and count ACCUMULATE across calls (zero them once; the host need not synchronise between batches).  eps is read from memory
 * (fp32 NCHW, any shape and alignment) or regenerated from the Philox stream of `seed` addressed by the dense NCHW index, bit-identical
 * to c2w_philox_normal -- on a 16-byte aligned tensor of that stream both forms give the same bits.
 * THE BIN RULE is part of the interface:  bin = min(K - 1, (int)floorf(t_b * (float)K))  with t_b clamped to [0, 1] and ONE fp32
 * multiply.  An fp64 evaluation of the same formula gives another bin at ordinary values (K = 10: t = 0.7f -> 7 here, 6 in double;
 * 0.9f -> 9 here, 8 in double); host code that predicts a bin must use fp32 arithmetic.
 * Two launches, no atomics: each image is cut into slabs of whole 64-pixel tiles, their number a function of (B, HW) only (about 2048
 * workgroups in all, never a slab across two images); a workgroup stores its slab's per-channel sums into `scratch` (plain fp32 stores,
 * every slot read is written by the same call), then ONE workgroup walks the images in ascending order, adds an image's slabs in
 * ascending order (fp32) and adds that sum onto the table in double.  Same operands => same bits, whatever else runs.
 * scratch must hold c2w_sq_err_levels_scratch_bytes(B, C, HW) bytes; NULL or fewer is C2W_ERR_BAD_ARG, never a fall-back to atomics.
 * C2W_ERR_UNSUPPORTED (seed form only): HW % 4 != 0 or rows too wide for the LDS tile -- materialise the stream with
 * c2w_philox_normal and call the tensor form, which takes every shape. */
long long c2w_sq_err_levels_scratch_bytes(int B, int C, int HW);
int c2w_sq_err_levels(const void* y, const float* eps, const float* t, double* table, long long* count, float* per_image, int B, int C, int HW,
                      int ldc, int K, float* scratch, unsigned long long scratch_bytes, int dtype, void* stream);
int c2w_sq_err_levels_noise(const void* y, unsigned long long seed, const float* t, double* table, long long* count, float* per_image, int B,
                            int C, int HW, int ldc, int K, float* scratch, unsigned long long scratch_bytes, int dtype, void* stream);
/* Ensemble spectra: the radially averaged power spectral density of n_fields dense fp32 fields x[n_fields][H][W] (16-byte aligned),
 * spec[n_fields][H/2] fp32, un-normalised.  The definition is the radial spectrum the reference's scores take from a radar library
 * (exp/metrics.py:67), restated here from memory of that library and not checked against it:
 *   P[u][v]  = |sum_ij x[i][j] exp(-2 pi i (u i / H + v j / W))|^2 / (H W)
 *   ku, kv   = the centred integer wavenumbers of u and v (-H/2 .. H/2 - 1 at an even size, as after an fftshift)
 *   r        = round(sqrt(ku^2 + kv^2)); a sum of two squares is never (k + 1/2)^2, so  k^2 - k < ku^2 + kv^2 <= k^2 + k  <=>  r = k
 *   spec[k]  = the mean of P over the cells with r = k,  k = 0 .. H/2 - 1; cells with a larger r are dropped.
 * bin 0 is the single cell P[0][0] = (sum x)^2 / (H W), formed from the field's sum in double; the mean is taken off before the
 * transform, so a large mean never enters an fp32 butterfly.  Frequencies, wavelengths and the division by sum_k spec[k] are the caller's.
 * One launch, one read of each field, nothing else in global memory, no scratch, no allocation, no atomics: a field is transformed in
 * LDS (two real rows per complex row transform, column transforms over the H/2 columns that can reach a bin, twiddles rounded from
 * double) and every sum has one order fixed by H, so a field's H/2 outputs are the same bits wherever it lies in the batch.  A NaN in
 * a field gives that field a NaN spectrum.  Fields of 8, 16 and 32 share a workgroup (16, 8, 4 of them); rows of spec past n_fields
 * are never written.  Supported: H == W in {8, 16, 32, 64, 128}; everything else returns C2W_ERR_UNSUPPORTED and writes nothing. */
int c2w_rapsd_supported(int H, int W); /* 1 or 0 */
int c2w_rapsd(const float* x, float* spec, long long n_fields, int H, int W, void* stream);
/* Ensemble SSIM: the mean structural similarity of n_pairs field pairs under a uniform win x win window, out[n_pairs] double.
 * x[n_pairs][H][W] and y[n_truth][H][W] are dense fp32, 16-byte aligned; pair i is (x[i], y[i % n_truth]) -- the layout that samples
 * [M][T][F] against truth [T][F] gives; data_range[n_truth] is a DEVICE array, one range per truth slot (variables may differ), read by
 * the kernel: nothing synchronises to fetch it.  The definition is the image library's structural_similarity with its defaults as the
 * reference calls it (exp/metrics.py:201-210: uniform window, sample covariance), restated here from memory of that library and not
 * checked against it.  With NP = win^2, cn = NP / (NP - 1), R = data_range:
 *   u_a  = the mean of a over the window, for a in x, y, xx, yy, xy
 *   vx   = cn (u_xx - u_x^2), vy likewise, vxy = cn (u_xy - u_x u_y);   C1 = (0.01 R)^2, C2 = (0.03 R)^2
 *   S    = (2 u_x u_y + C1)(2 vxy + C2) / ((u_x^2 + u_y^2 + C1)(vx + vy + C2))
 *   out  = the mean of S over the (H - win + 1)(W - win + 1) windows that lie inside the field (the library's crop by (win - 1) / 2, so
 *          its border mode never matters).
 * Numerics: both fields of a pair have p = the mean of y (double sum) taken off before any product is formed -- variances and the
 * covariance do not move, and the luminance factor is formed as 1 - (u_x - u_y)^2 / (u_x^2 + u_y^2 + C1) with u_x = p + mean(x - p);
 * window sums are direct fp32 sums, down the columns and then along the rows; the mean over the windows is a double sum.
 * One launch, one read of each x field (y is read twice: for p, then with x), nothing but `out` written to global memory, no scratch,
 * no atomics; every sum has one order fixed by (H, W, win), so out[i] is the same bits whatever i, n_pairs and n_truth are.  A NaN in a
 * pair gives that pair NaN and no other; a NaN data_range gives NaN to the pairs of its slot.  Rows of out past n_pairs are never
 * written.  Pairs with W <= 32 share a workgroup, four of them.  Supported: H and W multiples of 8 from 16 to 128 (rectangular
 * included), win in {7, 11, 15}; everything else returns C2W_ERR_UNSUPPORTED and writes nothing. */
int c2w_ssim_supported(int H, int W, int win); /* 1 or 0 */
int c2w_ssim(const float* x, const float* y, const float* data_range, double* out, long long n_pairs, long long n_truth, int H, int W, int win,
             void* stream);
/* Ensemble sliced Wasserstein distance (exp/metrics.py:13-44: ot.sliced_wasserstein_distance(a, b, n_projections=100, seed=0) per member
 * on arrays reshaped to (time, cells)).  The definition is restated from memory of that library (its sliced distance and its 1-D
 * distance) and not checked against it.  For one variable, samples X (T, d), truth Y (T, d), d = H W, P projections, p = 2:
 *   theta    = numpy.random.RandomState(seed).randn(d, P) in float64, every column divided by its Euclidean norm -- the same for every
 *              variable, since the reference passes seed=0 each time (the caller's: climate2weather_amd.wasserstein.projections)
 *   a, b     = X theta_p, Y theta_p;   D_p = mean_i (sort(a)_i - sort(b)_i)^2  (uniform weights, equal counts: the quantile form)
 *   SWD      = sqrt(mean_p D_p)        (the caller's)
 * and the reference normalises both arrays by the truth's moments first (exp/metrics.py:254-258): x^ = (x - shift[f]) * scale[f].
 * c2w_swd_project: proj[n_rep][F][P][T] fp32 = x^ theta for all n_rep T F fields of x[n_rep][T][F][d] (dense fp32, 16-byte aligned);
 * theta[P][d] fp32, 16-byte aligned, the float64 columns rounded once; shift[F], scale[F] DEVICE fp32.  Numerics: x^ is formed in fp32
 * on the loaded value BEFORE any product -- never (theta x - shift sum theta) * scale, a difference of two numbers near 1e5 on a
 * pressure field.  An fp32-input MFMA GEMM (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain), a workgroup owning 128 fields x all P
 * projections; a sum is d / 256 chunk sums, each a 256-long chain in a fixed k order, added in ascending order.  No atomics, no
 * scratch: a field's P outputs are the same bits wherever it lies in the batch; a NaN stays in its field's P outputs; nothing is
 * written past n_rep F P T.  Supported: d a multiple of 64 from 64 to 65536, 1 <= P <= 128.
 * c2w_swd_project_pair: the same for x and for the truth y[T][F][d] -> proj_y[F][P][T] in ONE launch (the truth's T F fields are too
 * few to fill the chip on their own); the same bits as two c2w_swd_project calls.  y == NULL: x only.
 * c2w_swd_distance: out[n_rep][F][P] double = D_p of the columns proj_x[rep][f][p][0..T) and proj_y[f][p][0..T): one workgroup per
 * pair sorts both columns in LDS (bitonic, padded with +inf to a power of two, the padding never enters the sum); differences,
 * squares and the sum over i < T in double, in an order fixed by T.  A NaN in either column is detected at load and NaN is written
 * for that (rep, f, p) explicitly; +-inf inputs are unspecified.  Supported: 1 <= T <= 16384 (two padded columns = 128 KiB of LDS).
 * Everything unsupported returns C2W_ERR_UNSUPPORTED and writes nothing. */
int c2w_swd_supported(int d, int P, int T); /* 1 or 0 */
int c2w_swd_project(const float* x, const float* theta, const float* shift, const float* scale, float* proj, long long n_rep, int T, int F,
                    int d, int P, void* stream);
int c2w_swd_project_pair(const float* x, const float* y, const float* theta, const float* shift, const float* scale, float* proj_x,
                         float* proj_y, long long n_rep, int T, int F, int d, int P, void* stream);
int c2w_swd_distance(const float* proj_x, const float* proj_y, double* out, long long n_rep, int F, int P, int T, void* stream);
/* Ensemble marginals and calibration (exp/figures.py:23-241, kde_and_pmf): the Gaussian kernel density estimate of every member's and the
 * truth's values per variable (:52-80, scipy.stats.gaussian_kde with its defaults, evaluated at N = 1000 points), and the rank
 * histogram of the truth within the ensemble (:86, :178-192).  The KDE formula below is VERIFIED against scipy.stats.gaussian_kde
 * (tests/test_kde_cpu.py prints the agreement); the rank count is the reference's own line of numpy.
 *   KDE   f(g) = (1 / (n h sqrt(2 pi))) * sum_i exp(-(g - x_i)^2 / (2 h^2)),  h = factor * std(x, ddof = 1), factor = n^(-1/5) (Scott,
 *         scipy's default), (3 n / 4)^(-1/5) for "silverman", or a number taken as the factor itself (the caller's:
 *         climate2weather_amd.marginals.bandwidth).  One data set is one (member, variable) or (truth, variable) over all T times and
 *         hw cells, n = T hw, and every data set has its own h.  The report's grid per variable is linspace(min(truth.min,
 *         samples.min), max(truth.max, samples.max), N) in float64 (the caller's).
 *   PIT   r = #{m : sample_m <= truth} per (time, variable, cell) with IEEE <=: ties count, a NaN on either side compares false;
 *         counts[f][r], r = 0 .. M.  The reference's PIT value is r / M, its density=True histogram counts * M / counts.sum().
 * c2w_kde_eval: dens[D][N] double for the D = n_rep F (+ F with y) data sets of x[n_rep][T][F][hw] and of the truth y[T][F][hw] (dense
 * fp32, 16-byte aligned; y == NULL: x only) in ONE launch pair; data set ds < n_rep F is member ds / F, variable ds % F, the rest are
 * the truth's variables; h[D] DEVICE doubles in that order.  Numerics: the grid arrives as fp32 offsets[F][N] = g_j - pivot[f],
 * computed in float64 and rounded once, from an fp32 pivot[f] near the middle of variable f's grid (both DEVICE arrays); the kernel
 * forms x - pivot in fp32 ON THE LOADED VALUE, before anything else touches it -- exact whenever x and the pivot lie within a factor
 * of two of each other.  A pressure field lies at 101325 +- 1200 and with n in the millions h is a few tens: a float64 grid point
 * rounded to fp32 moves by up to 0.004, 1e-4 of h, several 1e-4 relative in a tail term -- never evaluate g - x on raw fp32 values.
 * exp(-u^2 / 2) = exp2(-((g - x) k)^2), k = sqrt(log2(e) / 2) / h rounded to fp32 once per data set: per pair one fma (against g k,
 * formed in double and rounded once per grid point), one multiply, one v_exp_f32 (terms below 2^-126 flush to zero), one add.
 * Dense and exact: no pair is dropped, no truncation radius.  kde_partial_kernel: a workgroup owns one data set and one chunk of its
 * values, a thread up to four grid points as fp32 accumulators; a chain holds at most 256 terms before it joins a double, in value
 * order; a chunk's N doubles go to scratch as partial[D][chunks][N].  The chunk length is a function of n alone (n / 64 rounded up to
 * whole tiles of 1024 values), not of D or of the device: dens[ds] is the same bits whatever else rides in the launch and wherever
 * the data set lies in it.  kde_fold_kernel adds the chunks in index order and multiplies by 1 / (n h sqrt(2 pi)), both in double.
 * No atomics.  A NaN or inf value makes its data set's whole row NaN, written explicitly, and touches no other row; n < 2 or zero
 * spread (h NaN or 0) gives a NaN row as the formula does.  scratch: c2w_kde_scratch_bytes(D, T hw, N) bytes, 8-byte aligned, every
 * byte of it written before it is read.  Supported: hw a multiple of 4, 1 <= N <= 1024.  c2w_kde_partial and c2w_kde_fold are the two
 * launches of c2w_kde_eval on their own (the same bits), for a caller that times or schedules them apart.
 * c2w_pit_counts: counts[F][M + 1] int64 (zeroed by the call, on the stream) from x[M][T][F][hw] against y[T][F][hw] (dense fp32,
 * 16-byte aligned).  pit_count_kernel: a workgroup stays inside one variable's (t, f) planes, reads the truth with 16-byte loads and
 * the M members at stride T F hw, counts per cell in registers, bins in an LDS histogram and issues one global integer add per
 * (workgroup, bin) -- integer sums are exact in any order.  Supported: hw a multiple of 4, 1 <= M <= 64.
 * Everything unsupported returns C2W_ERR_UNSUPPORTED and writes nothing. */
int c2w_kde_supported(int hw, int N); /* 1 or 0 */
long long c2w_kde_scratch_bytes(long long D, long long n, int N);
int c2w_kde_eval(const float* x, const float* y, const float* offsets, const float* pivot, const double* h, double* scratch,
                 unsigned long long scratch_bytes, double* dens, long long n_rep, int T, int F, int hw, int N, void* stream);
int c2w_kde_partial(const float* x, const float* y, const float* offsets, const float* pivot, const double* h, double* scratch,
                    unsigned long long scratch_bytes, long long n_rep, int T, int F, int hw, int N, void* stream);
int c2w_kde_fold(const double* scratch, const double* h, double* dens, long long D, long long n, int N, void* stream);
int c2w_pit_supported(int hw, int M); /* 1 or 0 */
int c2w_pit_counts(const float* x, const float* y, long long* counts, int M, int T, int F, int hw, void* stream);
/* Exact quantiles on the device (data/xarray_preproc.py::compute_quantiles: xds.quantile(levels, dim=["time", "rlat", "rlon"]) per
 * variable, the constants data/pipeline.py::normalize_ds scales by; evaluated per ensemble member they are the tail diagnostic).
 * Definition.  A data set is every value of one variable, indexed as for c2w_kde_eval: data set d = rep * F + f is x[rep][t][f][:] for
 * all t < T; with a truth y[T][F][hw] its F data sets follow as d = n_rep * F + f; D data sets in all, n = T * hw values each, dense
 * fp32.  For data set d and level q in [0, 1]:
 *   1. nv = the number of non-NaN values
 *   2. v = (nv - 1) * q in float64
 *   3. lo = floor(v), hi = min(lo + 1, nv - 1), t = v - lo
 *   4. a, b = the lo-th and hi-th smallest non-NaN values, exact, as fp32 bit patterns
 *   5. the result, float64: a + (b - a) * t where t < 0.5, b - (b - a) * (1 - t) where t >= 0.5
 * This is numpy.quantile(x.astype(float64), q, method="linear") with numpy's own _lerp (checked against numpy 2.2.6 by
 * tests/test_quantiles_cpu.py), applied uniformly: an infinite neighbour gives what numpy gives (NaN at q = 0 when the minimum is
 * -inf).  A zero result may carry either sign.  skipna != 0 (numpy.nanquantile): NaNs are counted and left out; skipna == 0
 * (numpy.quantile): any NaN makes the data set's whole row NaN; nv == 0 gives a NaN row.
 * c2w_quantiles: out[D][Q] double, stats[D][Q][2] fp32 (the two order statistics a, b), n_valid[D] int64 (nv, whatever skipna is).
 * q: a HOST array of Q doubles, passed to the kernels by value; a level that is NaN or outside [0, 1] is C2W_ERR_BAD_ARG.
 * Method: radix select on the monotone key k = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000) of the loaded bit pattern -- no float
 * arithmetic touches a value, denormals are kept, -0.0 sorts just below +0.0, a NaN goes to the data set's NaN counter and never to a
 * bin.  Three counting passes over key digits of 12 / 10 / 10 bits, most significant first, each one full read of the data with
 * 16-byte loads: quantile_count_kernel (a workgroup owns one data set and a slab of its planes, counts in LDS ints -- all 4096 bins
 * in pass 0, 1024 bins per active slot later -- and issues one 64-bit integer add per non-zero bin), then quantile_locate_kernel
 * (one workgroup per data set: nv and the 2 Q target ranks in double after pass 0, each rank's bin and residual rank by a scan in
 * index order, equal prefixes merged into slots, the slot table of the next pass; after the last pass the keys, inverted to values,
 * and the interpolation without contraction).  All on the caller's stream, nothing read back by the host in between.  The result is
 * a function of integer counts only: independent of the grid, the slab arithmetic and the order of the adds, the same bits wherever
 * a data set lies in the launch.  No float atomics.  scratch: c2w_quantile_scratch_bytes(D, Q) bytes, 16-byte aligned; the call
 * zeroes its tables with hipMemsetAsync on the stream.  Supported: hw a multiple of 4, 1 <= Q <= 16.  A workgroup's slab of 2^31
 * values or more is C2W_ERR_BAD_SHAPE.  Everything unsupported returns C2W_ERR_UNSUPPORTED and writes nothing. */
int c2w_quantile_supported(int hw, int Q); /* 1 or 0 */
long long c2w_quantile_scratch_bytes(long long D, int Q);
int c2w_quantiles(const float* x, const float* y, const double* q, int Q, int skipna, void* scratch, unsigned long long scratch_bytes,
                  double* out, float* stats, long long* n_valid, long long n_rep, int T, int F, int hw, void* stream);
/* Ensemble CRPS and spread-skill: the M members of one cell judged jointly against that cell's truth.
 * Definition.  One cell (t, f, c) has the members x_1 .. x_M = x[m][t][f][c] and the truth y = y[t][f][c], fp32 inputs read as exact
 * real numbers.  Four non-negative terms per cell:
 *   A = (1 / M) sum_m |x_m - y|
 *   B = sum_{m < m'} |x_m - x_m'|, with the members sorted = sum_{k = 1}^{M - 1} k (M - k) (x_(k + 1) - x_(k))
 *   E = (mean_m x_m - y)^2
 *   V = sum_m (x_m - mean x)^2 / (M - 1)                                                  (M = 1: NaN)
 * and from their means over the cells of a (t, f) plane, or over any larger set (the caller's: climate2weather_amd.crps):
 *   crps      = mean A - mean B / M^2         the empirical-CDF form, integral (F_M(z) - 1[z >= y])^2 dz, VERIFIED against that
 *                                             integral evaluated exactly in float64 (tests/test_crps_cpu.py), not recalled
 *   crps_fair = mean A - mean B / (M (M - 1))                                              (M = 1: NaN)
 *   rmse = sqrt(mean E), spread = sqrt(mean V), ratio = sqrt((M + 1) / M) * spread / rmse  (1: a statistically consistent ensemble)
 * Non-finite values: a member or a truth that is NaN or infinite makes the four terms of its cell, and with them the four sums of
 * its (t, f) entry, NaN, written explicitly; no other entry is touched.
 * c2w_crps_terms: sums[T][F][4] double = the sums of A, B, E, V over the hw cells of every plane, from x[M][T][F][hw] against
 * y[T][F][hw] (dense fp32, 16-byte aligned); cells, if not NULL: [4][T][F][hw] fp32, the planes A, B, E, V per cell (16-byte aligned).
 * Numerics: a straight fp32 port fails on the fields this project downscales -- on a pressure field at 101325 +- 1200 with a member
 * spread of 0.05 - 3 the mean and the variance of the raw values put V off by orders of magnitude -- so the kernel forms only
 * differences of nearby numbers and sums of non-negative terms.  crps_terms_kernel: a workgroup of 256 owns one plane, or one chunk of
 * 4096 cells of it (a function of hw alone); a thread owns V adjacent cells at a time and holds their K x V member values in
 * registers, K = M rounded up to 8, 16, 32 or 64 and (K, V) one of (8, 4), (16, 4), (32, 2), (64, 1), loaded as wide as V allows with
 * all loads in flight before the first use (K loads in a straight line: row i asks for member min(i, M - 1), so a row from M on hits
 * the line the last member's load has just brought in); non-finite values are found on the loaded values (min and max drop a NaN);
 * rows M .. K - 1 are then set to +inf.  The rows are sorted by Batcher's odd-even merge network of v_min_f32 / v_max_f32 pairs with static indices (no scratch
 * memory); every sum runs over the first M rows only.  B from the neighbour gaps times the exact weights k (M - k); the pivot
 * p = x_(M / 2), e_i = x_(i) - p, ebar = (sum e) / M, V = sum (e_i - ebar)^2 / (M - 1), E = ((p - y) + ebar)^2; A = sum |x_(i) - y| / M;
 * no multiply fused with an add.  Identical members give B = 0 and V = 0 exactly.  Per-cell values are fp32; they join four double
 * accumulators per thread in cell order, the workgroup folds those by the fixed-order sum of csrc/ordered_sum.h (sixteen threads at a
 * time, then the sixteen group totals), and when a plane has several chunks fold_parts_kernel adds them in index order: at most two launches on the
 * caller's stream, no atomics, no host read-back, the same bits for a plane wherever it lies in the launch.  Per cell the error is at
 * most (M + 16) 2^-24 s with s the float64 value itself for A, B, V and A^2 for E; a sum's at most (M + 16) 2^-24 times the sum of
 * its cells' s (tests/fp64_crps_ref.py).  scratch: c2w_crps_scratch_bytes(T, F, hw) bytes (0 while a plane is one chunk: the pointer
 * may then be NULL), 8-byte aligned, every byte of it written before it is read.  Supported: hw a multiple of 4, 1 <= M <= 64.
 * Everything unsupported returns C2W_ERR_UNSUPPORTED and writes nothing. */
int c2w_crps_supported(int hw, int M); /* 1 or 0 */
long long c2w_crps_scratch_bytes(int T, int F, int hw);
int c2w_crps_terms(const float* x, const float* y, double* sums, float* cells, double* scratch, unsigned long long scratch_bytes, int M,
                   int T, int F, int hw, void* stream);
/* Wind power of an ensemble: hub-height speed, turbine power curve, domain sums (the reference's exp/figures.py::_calc_windpower).
 * Definition.  One cell of one (d, t) plane -- d a data set: a member, the truth, the coarse observation; t a time -- has the fp32 wind
 * components u, v in m/s (fields DE-NORMALISED), read as exact real numbers.
 *   hub factor  c = (hub_height / reference_height)^alpha, formed in float64 by the caller (defaults 100, 10, 1/7), passed as a float
 *   speed       = sqrt(u u + v v) c                         (the reference writes np.sqrt(u**2 + v**2), not hypot)
 *   power       = numpy.interp(speed, xs, ps, left = 0, right = 0), the curve having K >= 2 knots, xs strictly increasing, ps in W:
 *                 ps[j] + (speed - xs[j]) slope_j for xs[j] <= speed < xs[j + 1]; ps[K - 1] at speed == xs[K - 1]; 0 strictly above
 *                 it (cut-out) and below xs[0]; NaN for a NaN speed; 0 for +inf
 *   sums[d][t]  = {S_speed, S_power}, the sums of the two over the hw cells of the plane, in double
 * and from them (the caller's: climate2weather_amd.windpower) mean power = S_power / hw and the cumulative energy series
 * cumsum_t(mean power / 1e3).  That windpowerlib's ModelChain with its defaults is this numpy.interp call is RECALLED (README, statement
 * 9); numpy.interp itself is the float64 reference of every test.  No turbine's data is shipped: the caller passes the curve.
 * Non-finite values: a NaN u or v makes the two values of its cell, and with them the two sums of its (d, t) entry, NaN, written
 * explicitly; no other entry is touched.  An infinite u or v gives speed +inf and power 0.
 * c2w_wind_table (pure host code) fills the packed table of c2w_wind_table_bytes(K) = 32 + 16 (K - 1) + 512 bytes at table_host, 16-byte
 * aligned: a header {x^_0, x^_{K-1}, p_{K-1}, buckets per m/s, K, mode}; the K - 1 intervals as {x^_j, p_j, slope_j, x^_{j+1}} fp32, one
 * 16-byte LDS read per interpolation; 256 two-byte starting knots of a uniform bucket index over [x^_0, x^_{K-1}].  The knots are rounded
 * to fp32 (x^) and must still increase strictly; slope_j = (p_{j+1} - p_j) / (x^_{j+1} - x^_j) is formed in float64 from the rounded
 * knots and rounded once, so the table is the piecewise-linear curve through (x^_j, p_j).  C2W_ERR_BAD_ARG for K outside 2 .. 256, a
 * knot, a power or a slope that is not finite in fp32, and knots that do not increase strictly (as given, or once rounded).  The caller
 * copies the table to the device.
 * c2w_wind_power: fields is [planes][F][hw] dense fp32, 16-byte aligned; the u and v planes of every (d, t) sit at u_index and v_index
 * of its F, so 2 / F of the tensor is read, every value once, 16 bytes a load.  sums[planes][2] double; derived, if not NULL:
 * [planes][2][hw] fp32, speed in plane 0 and power in plane 1 (16-byte aligned) -- the layout c2w_kde_eval takes as F = 2 variables.
 * wind_power_kernel: a workgroup of 256 owns one plane, or one chunk of 4096 cells of it (a function of hw alone), and copies the table
 * to LDS once.  The lookup is bucket -> starting knot -> 2 forward steps, none behind a branch, where no bucket holds more than 2 knots (mode 0), a
 * binary search over the intervals otherwise (mode 1: curves whose knots crowd a bucket).  The arithmetic is fp32, no multiply fused
 * with an add, the square root correctly rounded.  Per-cell values join two double accumulators per thread in cell order, the
 * workgroup folds those by the fixed-order sum of csrc/ordered_sum.h (sixteen threads at a time, then the sixteen group totals), and when
 * a plane has several chunks fold_parts_kernel adds them in index order: at most two launches on the caller's stream, no atomics, no host
 * read-back, the same bits for a plane wherever it lies in the launch.  Error against float64 (tests/fp64_wind_ref.py): the speed within
 * 6 * 2^-24 of itself plus 2^-62 c where the squares underflow; the power between the least and the largest value of the float64 curve
 * over the speed's window widened by the rounding of a knot, give or take 9 * 2^-24 of the larger power at the interval's ends; a sum
 * within the sum of its cells' bounds.  A float64 u u + v v beyond the fp32 range gives speed +inf.  scratch:
 * c2w_wind_scratch_bytes(planes, hw) bytes (0 while a plane is one chunk: the pointer may then be NULL), 8-byte aligned, every byte of
 * it written before it is read.  Supported: hw a multiple of 4, 2 <= K <= 256.  Everything unsupported returns C2W_ERR_UNSUPPORTED and
 * writes nothing. */
int c2w_wind_supported(int hw, int K); /* 1 or 0 */
long long c2w_wind_table_bytes(int K);
int c2w_wind_table(const double* xs, const double* ps, int K, void* table_host);
long long c2w_wind_scratch_bytes(long long planes, int hw);
int c2w_wind_power(const float* fields, int F, int u_index, int v_index, const void* table, int K, float hub_factor, double* sums,
                   float* derived, double* scratch, unsigned long long scratch_bytes, long long planes, int hw, void* stream);
/* Energy score and variogram score of an ensemble: the two multivariate scores, which see the dependence between the cells of a field
 * that the per-cell CRPS cannot (Gneiting & Raftery 2007; Scheuerer & Hamill 2015 -- both as recalled: README, statement 10).
 *
 * Definitions.  One (t, f) plane of hw = H W cells has the rows r_0 = y (the truth) and r_1 .. r_M = x_m, fp32 read as exact numbers;
 * planes = T F, x is [M][planes][hw], y is [planes][hw], dense.
 *   Energy score.  D2[plane][p] = sum_c (r_i[c] - r_j[c])^2 for every pair i < j, p row-major over i < j
 *   (p = i (2 (M + 1) - i - 1) / 2 + j - i - 1), P = M (M + 1) / 2 -- the kernel's product, double.  From it, the caller's in float64
 *   (climate2weather_amd.multivariate): D = sqrt(D2), A = (1 / M) sum_m D(0, m)^beta, B = sum_{1 <= m < m'} D(m, m')^beta,
 *   ES = A - B / M^2, fair: A - B / (M (M - 1)) (NaN for M = 1), beta in (0, 2), default 1; over all variables jointly
 *   D2_joint = sum_f D2[t][f] / scale_f^2.
 *   Variogram score of order p.  The offsets o = (di, dj) with max(|di|, |dj|) <= R in the half plane di > 0, or di == 0 and dj > 0,
 *   row-major: (0, 1) .. (0, R), then di = 1 .. R each with dj = -R .. R; O = ((2 R + 1)^2 - 1) / 2.  For every cell pair (c, c + o) with
 *   both cells inside the field g_y = |y_c - y_{c+o}|^p and g_x = (1 / M) sum_m |x_{m,c} - x_{m,c+o}|^p, and
 *   V[plane][o][0..2] = the sums over the pairs of ((g_y - g_x)^2, g_y, g_x) -- the kernel's product, double.  The weights are the
 *   caller's: VS = sum_o w_o V[..][o][0]; V[..][1] and V[..][2] over the pair count (H - di) (W - |dj|) are the empirical variograms
 *   of truth and ensemble by lag.  The kernel takes p as order2 = 2 p in {1, 2, 4}.
 * Non-finite values: a NaN or an infinity in a row makes every D2 entry of that row in its plane NaN, and the three sums of every
 * (plane, o) one of whose pairs touches its cell NaN; no other entry is touched.  The kernels see it on the result -- every term is
 * >= 0 and a difference with a non-finite end is not finite -- so a term that overflows fp32 (a difference beyond 1.8e19) ends as NaN
 * as well.
 * escore_pairs_kernel: a workgroup of 256 owns 256 cells of one plane and copies them, all M + 1 rows, from HBM to LDS once, 16 bytes a
 * load; a thread owns a 4 x 4 tile of row pairs and every S-th group of 4 cells (S a function of M) and keeps 16 double sums:
 * d = a - b in fp32, d * d in fp32, not fused, added to the double in cell order.  The S threads of a tile fold through LDS in thread
 * order; fold_parts_kernel (csrc/ordered_sum_launch.h) adds the chunks of a plane in index order.  (M + 1) 1040 bytes of LDS, at least 32 KiB: 67 600 at M = 64.
 * vario_terms_kernel: a workgroup of 256 owns an 8 x 32 tile of one plane and copies it with its halo (R columns either side, R rows
 * below) of all M + 1 rows to LDS; a thread owns a cell and walks the offsets four at a time, the member loop innermost: every term
 * fp32 (p = 0.5 the correctly rounded square root, p = 1 the absolute value, p = 2 a product), g_x the fp32 chain of the M terms in
 * member order times the fp32 1 / M, ((double)g_y - (double)g_x)^2 and the two variograms summed in double by the fixed-order sum of
 * csrc/ordered_sum.h (sixteen threads at a time, then the sixteen group totals); fold_parts_kernel adds the tiles in index order.  At most 78 336
 * bytes of LDS (R = 8, M = 16).  At most two launches each on the caller's stream, no atomics, no host read-back, the same bits for a
 * plane wherever it lies in the launch.  Error against float64 (tests/fp64_escore_ref.py): a D2 entry within 3 * 2^-24 of itself;
 * V[..][0] within (2 M + 8) 2^-24 sum (g_y + g_x)^2 over its pairs, V[..][1] within 3 * 2^-24 and V[..][2] within (M + 4) 2^-24 of
 * themselves.  scratch: c2w_*_scratch_bytes bytes (0 while a plane is one chunk or one tile: the pointer may then be NULL), 8-byte
 * aligned, every byte of it written before it is read.  Supported: pairs hw a multiple of 4, 1 <= M <= 64 (x, y 16-byte aligned);
 * variogram H and W multiples of 8, 1 <= R <= 8, 1 <= M <= 16, order2 in {1, 2, 4}.  Everything unsupported returns
 * C2W_ERR_UNSUPPORTED and writes nothing. */
int c2w_escore_supported(int hw, int M); /* 1 or 0 */
long long c2w_escore_scratch_bytes(long long planes, int hw, int M);
int c2w_escore_pairs(const float* x, const float* y, double* d2, double* scratch, unsigned long long scratch_bytes, int M, long long planes,
                     int hw, void* stream);
int c2w_vario_supported(int H, int W, int R, int M, int order2); /* 1 or 0 */
long long c2w_vario_scratch_bytes(long long planes, int H, int W, int R);
int c2w_vario_terms(const float* x, const float* y, double* V, double* scratch, unsigned long long scratch_bytes, int M, long long planes,
                    int H, int W, int R, int order2, void* stream);
/* Temporal increments of an ensemble: what a field does from one hour to a later one, which no score above sees -- each of them judges
 * one (t, f) plane at a time.  The definitions are elementary and verified by known answers (README, statement 11).
 *
 * Definitions.  x is [n_rep][T][F][hw], y is [T][F][hw] or NULL, both dense fp32 read as exact numbers.  The rows are r_0 = y when a
 * truth is given, then r_1 .. r_n = x (as c2w_escore_pairs has them); D = n_rep + 1 with a truth, n_rep without.  For row d, anchor
 * time t, variable f and lag tau = 1 .. L with t + tau < T, over the hw cells c of the plane
 *   dx_c = r_d[t + tau][f][c] - r_d[t][f][c],  dy_c the same increment of the truth
 *   S[d][t][f][tau - 1][0] = sum_c |dx_c|            (A1)
 *   S[d][t][f][tau - 1][1] = sum_c dx_c^2            (A2)
 *   S[d][t][f][tau - 1][2] = sum_c (dx_c - dy_c)^2   (E2)
 * S is double, [D][T][F][L][3], every entry written.  The truth's own row has E2 = +0.0; without a truth column 2 is +0.0; an entry
 * with t + tau >= T is +0.0 in all three columns: there is no pair, and the host knows the count.  From S, the caller's in float64
 * (climate2weather_amd.temporal): the structure functions S_p(tau) = sum_t A_p / ((T - tau) hw), the variability ratios
 * sqrt(S_2^m / S_2^y) and S_1^m / S_1^y, the tendency RMSE sqrt(sum_t E2 / ((T - tau) hw)) and the means by phase of an observation
 * period.
 * Non-finite values: a NaN or an infinity in plane (d, t, f) makes exactly these entries NaN, written explicitly: (d, t, f, tau) for
 * every tau that has a pair, (d, t - tau, f, tau) for every tau <= t, and, when the plane is the truth's, column 2 of the same entries
 * of every row (of the truth's own too); no other entry is touched.  The kernel sees it on the result -- every term is >= 0 and an
 * increment with a non-finite end is not finite, so a sum is non-finite exactly then and is written as NaN; a dx^2 that overflows fp32
 * (an increment beyond 1.8e19) ends as NaN as well.
 * tincr_terms_kernel: a workgroup of 256 owns one (d, t, f) anchor plane, or one chunk of 4096 cells of it (a function of hw alone).
 * The lags go in passes of 4; in a pass a thread loads 4 adjacent cells of the anchor plane, of the pass's four later planes and, with
 * a truth, of the truth's five, 16 bytes a load (a lag past L or past the end of the series reads plane T - 1 again and forms no term).
 * dx = b - a, |dx| and dx * dx, e = dx - dy and e * e are fp32, no multiply fused with an add; every fp32 term is added straight into
 * its double accumulator, cells in ascending order: no fp32 chain is kept.  The 12 sums of a pass fold by the fixed-order sum of
 * csrc/ordered_sum.h (sixteen threads at a time, then the sixteen group totals), and when a plane has several chunks
 * fold_parts_kernel adds them in index order: at most two launches on the caller's stream, no atomics, no host read-back, the same
 * bits for an entry wherever its plane lies in the launch.  A plane is read up to L + 1 times as an anchor and as a later plane; the
 * re-reads are left to the caches.  Error against float64 (tests/fp64_temporal_ref.py): A1 within 2 * 2^-24 of itself, A2 within
 * 3 * 2^-24 of itself, E2 within 6 * 2^-24 sum_c (|dx_c| + |dy_c|)^2 -- the error of E2 scales with the increments, not with their
 * difference -- each plus one fp32 denormal per cell.  scratch: c2w_tincr_scratch_bytes(rows, T, F, hw, L) bytes, rows = D (0 while a
 * plane is one chunk: the pointer may then be NULL), 8-byte aligned, every byte of it written before it is read.  Supported: hw a
 * multiple of 4, 1 <= L <= 24 (x, y 16-byte aligned).  Everything unsupported returns C2W_ERR_UNSUPPORTED and writes nothing. */
int c2w_tincr_supported(int hw, int L); /* 1 or 0 */
long long c2w_tincr_scratch_bytes(long long rows, int T, int F, int hw, int L);
int c2w_tincr_terms(const float* x, const float* y, double* S, double* scratch, unsigned long long scratch_bytes, int n_rep, int T, int F,
                    int hw, int L, void* stream);
/* Empirical quantile mapping per cell (climate2weather_amd.biascorrect): the step that turns a coarse climate-model series into the
 * bias-corrected series the sampler is conditioned on.  x: [n_rep][T][F][hw] fp32.  A SERIES is the values of one variable at one cell
 * over the times of one group (a calendar month, say; G = 1: no grouping).  The groups are given as a list: tidx[Tu] (int, device) holds
 * the times that have a group, sorted by group, and goff[G + 1] (int, device) where each group's part begins; group g is
 * tidx[goff[g] .. goff[g + 1]), goff[0] = 0, goff[G] = Tu <= T, and max_len is the longest group.  The kernels clamp every index they
 * read from the two lists, so a wrong list gives wrong numbers and never an access outside the arrays.
 * Nodes.  levels[K] (double, device), p_0 < .. < p_{K-1} in [0, 1].  q[rep][g][f][c][k] is the quantile at p_k of series
 * (rep, g, f, c) by the definition of c2w_quantiles above -- numpy.nanquantile(series.astype(float64), p_k), method "linear" with
 * numpy's _lerp: the two order statistics are exact fp32, the interpolation is float64 (csrc/quantile_core.h: rank_of, lerp_of, and
 * the monotone key the values are sorted by).  skipna != 0 leaves NaNs out; skipna == 0 makes the K nodes of a series with a NaN NaN.
 * A series without a valid value, an empty group included, is K NaNs.  n_valid[rep][g][f][c] (long long) = the non-NaN values.
 * c2w_qmap_nodes serves the cells [c0, c1) of every (rep, f) and writes only their entries; the caller walks the cell blocks so that
 * scratch -- c2w_qmap_scratch_bytes(n_rep F, c1 - c0, Tu) bytes, the series one after the other, fp32 -- stays bounded.  Two
 * launches: qmap_gather_kernel moves a tile of 64 list positions x 64 cells through LDS (a wave reads 256 contiguous bytes of a
 * plane and writes 256 contiguous bytes of a series); qmap_sort_kernel, a workgroup per series, loads the keys into LDS (a NaN and the
 * padding to the next power of two become the key no number has and sort to the top), runs a bitonic network, finds the count by
 * bisection and has thread k interpolate level k.
 * Mapping.  xq / yq [G][F][hw][K] (double): the nodes of the model's and of the reference's historical series.  out (the shape of x;
 * may BE x) gets, for every time t that has a group g, with the tables of (g, f, c), all in float64:
 *     j = the last node with xq[j] <= x
 *     no such node (x < xq[0]):  y = x + (yq[0] - xq[0])
 *     j == K - 1:                y = x + (yq[K-1] - xq[K-1])            (additive constant tails; x == xq[K-1] and +inf included)
 *     otherwise:                 v = yq[j] + (x - xq[j]) * ((yq[j+1] - yq[j]) / (xq[j+1] - xq[j])),  y = v > yq[j+1] ? yq[j+1] : v
 * no multiply fused with an add, y rounded once to fp32.  The interval is never degenerate (j is the LAST node <= x), and the clamp
 * makes the map non-decreasing across node boundaries.  A NaN x or a NaN table row gives NaN; a time without a group is not written.
 * qmap_apply_kernel: a workgroup of 512 per (g, f, block of C adjacent cells, slab of the group's (rep, time) rows), C in {64 .. 4}
 * chosen from K so that both tables of its cells fit 72 KiB of LDS; it stages them once, then walks its rows with 16-byte loads, four
 * in flight, bisects the four values of a load in LDS side by side and stores to the position it loaded from: each input read once,
 * each output written once.
 * Both: no atomics, no host read-back, everything on the caller's stream, the same bits wherever a series lies in the launch.
 * Supported: hw a multiple of 4, 2 <= K <= 128, max_len <= 16384 (x, out 16-byte aligned).  Everything unsupported returns
 * C2W_ERR_UNSUPPORTED and writes nothing. */
int c2w_qmap_supported(int hw, int K, int max_len); /* 1 or 0 */
long long c2w_qmap_scratch_bytes(long long rows, int cells, int Tu);
int c2w_qmap_nodes(const float* x, const int* tidx, const int* goff, const double* levels, double* q, long long* n_valid, float* scratch,
                   unsigned long long scratch_bytes, long long n_rep, int T, int F, int hw, int Tu, int G, int K, int max_len, int skipna,
                   int c0, int c1, void* stream);
int c2w_qmap_apply(const float* x, float* out, const double* xq, const double* yq, const int* tidx, const int* goff, long long n_rep, int T,
                   int F, int hw, int Tu, int G, int K, int max_len, void* stream);
/* Event verification of an ensemble (climate2weather_amd.events): was the event forecast?  Every score above is an average over the
 * whole distribution; these ask about a threshold.  The Brier score, its decomposition and the ROC are elementary and verified by
 * identities; the fair correction and the FSS of Roberts & Lean (2008) are recalled; the zero-padded box filter is verified against
 * scipy.ndimage.uniform_filter(mode="constant") (README, statement 13).
 *
 * The event.  x is [M][T][F][hw], y is [T][F][hw], dense fp32 read as exact numbers; thr[F][K] fp32 and dir[F][K] int: entry (f, k)
 * is the event x >= thr (dir != 0, "above") or x <= thr (dir == 0, "below"), IEEE comparisons: infinities compare as numbers, a NaN is
 * no event in its own row.  Both kernels produce INTEGER tables (long long), added with 64-bit integer adds to an output the call
 * zeroes first: the result does not depend on any order, and it equals the definition bit for bit.
 *
 * c2w_event_counts.  counts[t][f][k][o][j], [T][F][K][2][M + 1]: the cells of plane (t, f) whose truth indicator is o and in which
 * exactly j of the M members have the event.  invalid[t][f]: the cells with a NaN among their M + 1 values; they are in no bin, so
 * sum_{o, j} counts[t][f][k] + invalid[t][f] = hw for every k.  event_counts_kernel: a workgroup of 256 owns one plane or one chunk of
 * 4096 cells of it; a thread loads 4 adjacent cells of the truth (16 bytes), keeps them and streams the members over them, its four
 * member counts per threshold in the bytes of one register.  The bins live in LDS.  The common bin (0, 0) -- no event, no member -- is
 * never added in LDS: the threads count their valid cells in a register and bin (0, 0) = valid cells - the other bins.  One 64-bit
 * add per non-zero bin goes to the output.  Supported: hw a multiple of 4, 1 <= M <= 64, 1 <= K <= 8 (x, y 16-byte aligned).
 *
 * c2w_fss_sums.  The rows are d = 0 the truth, d = 1 .. M the members and d = M + 1 the ensemble, whose cell value is the member
 * count 0 .. M.  For radius r = radii[s] (a HOST array of S ints), n_d(c) = the sum of row d's cell values over the (2r + 1)^2 window
 * centred on cell c of the H x W plane, cells outside the domain counting 0.  sums[t][f][k][s][d][0..1] = (sum_c n_d(c)^2,
 * sum_c n_d(c) n_0(c)), [T][F][K][S][M + 2][2]; row 0 holds (OO, OO).  fss_sums_kernel: a workgroup of 256 owns (plane, threshold, tile
 * of at most 64 x 64 cells) -- the thresholds run over the grid, the planes are re-read from the caches -- and stages the tile plus a
 * halo of the largest radius, clipped to the domain (at most 96 x 96), as indicators in LDS, where a scan along the rows and one along
 * the columns make the row's summed-area table (16-bit entries); every radius reads it with four LDS reads per cell.  The truth's
 * table stays resident while the members go by; the member counts accumulate as bytes and get a 32-bit table at the end.  Products
 * and sums are 64-bit.  75440 bytes of LDS, two workgroups a CU (csrc/events_core.h has the budget).  Supported: W a multiple of 4, H, W >= 4,
 * H W <= 2^20, 1 <= M <= 64, 1 <= K <= 8, 1 <= S <= 8 radii in 0 .. 16, and (M (2r + 1)^2)^2 H W < 2^62.
 * Both: no host read-back, everything on the caller's stream.  Everything unsupported returns C2W_ERR_UNSUPPORTED and writes nothing. */
int c2w_event_counts_supported(int hw, int M, int K); /* 1 or 0 */
int c2w_event_counts(const float* x, const float* y, const float* thr, const int* dir, long long* counts, long long* invalid, int M, int T,
                     int F, int hw, int K, void* stream);
int c2w_fss_supported(int H, int W, int M, int K, const int* radii, int S); /* 1 or 0 */
int c2w_fss_sums(const float* x, const float* y, const float* thr, const int* dir, long long* sums, const int* radii, int M, int T, int F,
                 int H, int W, int K, int S, void* stream);
/* Event spells of an ensemble (climate2weather_amd.spells): how long does an event last?  The scores above judge one (t, f) plane at a
 * time or the difference between two times; a calm of 30 hours, a frost of five nights and a gale of two hours can share all of them.
 * The definitions are elementary and verified by known answers; nothing is taken from a package (README, statement 14).
 *
 * The event is that of c2w_event_counts: x is [M][T][F][hw], y is [T][F][hw] or NULL, dense fp32 read as exact numbers; thr[F][K] fp32
 * and dir[F][K] int, x >= thr (dir != 0) or x <= thr (dir == 0), IEEE comparisons: infinities compare as numbers, a NaN is no event.
 * Rows: d = 0 is the truth if y is given, then the M members; D = M + 1, or M without a truth.  A SERIES is the indicator e[t] of one
 * (d, f, k, cell) over all the times seen so far, block after block.  A NaN ends a spell like any non-event; NaN cell-hours are counted
 * per (d, f) in invalid.  A SPELL is a maximal run of consecutive 1s of a series, its length L the hours in it.
 *
 * c2w_spell_update takes one block of T >= 0 times whose first plane is the absolute hour t0 >= 0 (T = 0 does nothing).
 *   state[4][D][F][K][hw] int: (open, longest, count, hours) of every series -- open the length of the run open at the last time seen
 *     (0 if none), longest and count over the spells that have ENDED, hours all event hours.  Read at the start, written at the end.
 *   hist[D][F][K][Lmax] long long, Lmax = max_duration: += the spells that ended in this block with L = b + 1; the last bin holds
 *     L >= Lmax.  A spell carried in through state.open has its whole length.
 *   onsets[D][F][K][period] long long (NULL at period = 0): += the spells whose first hour t has (t0 + t) mod period = phi.  A run
 *     that begins at a series' very first time is an onset there; a run continued from the previous block is none.
 *   invalid[D][F] long long: += the NaN cell-hours.
 * hist, onsets and invalid are ACCUMULATORS: the caller zeroes them once and the call adds.  The call never closes a run at the block's
 * end: a run that touches the last time seen is in state.open alone, and the caller closes it on a copy when it wants the tables
 * (hist + the bins of min(open, Lmax), count + (open > 0), max(longest, open)) -- censored spells are counted, not dropped.
 * spell_update_kernel: a workgroup of 256 owns (row, variable, chunk of 1024 cells); a thread owns 4 adjacent cells, keeps their
 * counters of up to 4 thresholds in 64 registers and walks the T planes in order with 16-byte loads, 8 in flight; an event that starts a
 * run is one LDS add, a run that ends another, nothing else touches LDS (4484 bytes); one 64-bit integer add per non-zero bin goes to the
 * accumulators, so no bit depends on any order.  K > 4 is two launches over disjoint entries.  Time is not split over workgroups.  No
 * scratch, no host read-back, everything on the caller's stream.  Supported: hw a multiple of 4, 1 <= K <= 8, 1 <= max_duration <= 256,
 * 0 <= period <= 24, M >= 1 (x, y, state 16-byte aligned); everything else returns C2W_ERR_UNSUPPORTED and writes nothing.  T beyond
 * 2^20 in one call is C2W_ERR_BAD_SHAPE (the LDS bins are 32-bit); the caller keeps the total time under 2^31. */
int c2w_spell_supported(int hw, int K, int max_duration, int period); /* 1 or 0 */
int c2w_spell_update(const float* x, const float* y, const float* thr, const int* dir, int* state, long long* hist, long long* onsets,
                     long long* invalid, int M, int T, int F, int hw, int K, int max_duration, int period, long long t0, void* stream);
/* Event objects of an ensemble (climate2weather_amd.objects): how many events are there, how big are they and where?  The tables above
 * take a plane as a bag of cells (c2w_event_counts), a box of cells (c2w_fss_sums) or a series per cell (c2w_spell_update); none knows
 * which event cells belong together.  The definitions are elementary and verified by known answers; the centroid displacement is the
 * binary-mass form of the L1 of Wernli's SAL, recalled (README, statement 15).
 *
 * The event and the rows are those of c2w_spell_update: x is [M][T][F][H W], y is [T][F][H W] or NULL, thr[F][K] fp32 and dir[F][K]
 * int, x >= thr (dir != 0) or x <= thr (dir == 0), IEEE comparisons, a NaN is no event; d = 0 is the truth if y is given, then the M
 * members; D = M + 1, or M without a truth.  An OBJECT is a maximal connected set of event cells of one (d, t, f, k) plane of H x W
 * cells; connectivity 4 joins edge neighbours, 8 edge and corner neighbours; nothing wraps around.  Its LABEL is the smallest linear
 * index i W + j of its cells: it depends on nothing but the plane.
 *   plane[D][T][F][K][6] long long: the number of objects, the event cells, the largest area, the objects that touch the domain's
 *     border (they are cut by it: censored), sum i and sum j over the event cells.  Written, not added to.
 *   area_hist[D][F][K][B] long long, B = floor(log2(H W)) + 1: += the objects of all T planes with area in [2^b, 2^(b + 1)).  An
 *     ACCUMULATOR: the caller zeroes it once and the call adds; planes are independent in time, so a year may arrive in blocks.
 *   objects[D][T][F][K][max_objects][8] int (NULL at max_objects = 0): the first max_objects objects of the plane in label order as
 *     (label, area, sum_i, sum_j, i_min, i_max, j_min, j_max); the unused slots are WRITTEN as label -1 and the rest 0.  Objects past
 *     the cap are not listed but are in every other table: plane[..][0] - max_objects says how many are missing.
 *   invalid[D][T][F] long long: the NaN cells.  Written, not added to.
 * object_tables_kernel: a workgroup of 512 owns one (d, t, f, k) plane -- the thresholds run over the grid, the plane is re-read from
 * the caches.  The indicator is staged once with 16-byte loads as a bit mask and labelled entirely in LDS: 16-bit labels, the runs
 * along a row take the index of their first cell, the runs of adjacent rows (and diagonals at connectivity 8) are united by a
 * label-equivalence union-find that links the larger root to the smaller with a compare-and-swap, then one flattening pass; the
 * minimum labels make the result independent of any order.  A run adds its length once to its root's area; the roots are ranked by a
 * scan in index order, which is the label order of the list.  No global atomics but the one 64-bit add per non-zero area bin, no
 * scratch memory, no host read-back, everything on the caller's stream; every data-dependent loop has a trip bound derived from H W.
 * 80128 bytes of LDS, two workgroups a CU (csrc/objects_maps.h has the budget).  Supported: W a multiple of 4, H W <= 16384,
 * 1 <= K <= 8, connectivity 4 or 8, 0 <= max_objects <= 256, M >= 1 (x, y 16-byte aligned); everything else returns
 * C2W_ERR_UNSUPPORTED and writes nothing.  T = 0 does nothing. */
int c2w_objects_supported(int H, int W, int K, int connectivity, int max_objects); /* 1 or 0 */
int c2w_object_tables(const float* x, const float* y, const float* thr, const int* dir, long long* plane, long long* area_hist, int* objects,
                      long long* invalid, int M, int T, int F, int H, int W, int K, int connectivity, int max_objects, void* stream);
/* Extremes of an ensemble (climate2weather_amd.extremes): what does the tail do?  Every score above averages over the whole
 * distribution or needs a threshold chosen in advance; none sees the largest gust of a day or the 20-block return level.  The sample
 * L-moments are those of scipy.stats.lmoment(standardize=False); the GEV fit by L-moments is recalled from Hosking & Wallis and lives
 * in extremes.py as float64 tensor algebra (README, statement 16).
 *
 * Rows: d = 0 is the truth if y is given, then the M members; D = M + 1, or M without a truth.  x is [M][T][F][hw], y is [T][F][hw]
 * or NULL, dense fp32.  A SERIES is one (d, f, cell) over time; dir[F] int is 1 for maxima and 0 for minima of variable f; block b holds
 * the absolute hours [b block, (b + 1) block).  The EXTREME of a block is taken in the total order of the key of c2w_quantiles on the
 * fp32 bits: -0.0 < +0.0, the infinities are ordinary values, NaN hours are skipped and counted per (d, f) in invalid; a block whose
 * hours are all NaN has the extreme NaN, stored as the one pattern 0x7FC00000.
 *
 * c2w_block_extremes_update takes T >= 0 consecutive hours whose first plane is the absolute hour t0 >= 0 (T = 0 does nothing).
 *   open[D][F][hw] unsigned: the running key of the open block, read at the start and written at the end.  The key of a value is
 *     key ^ (dir ? 0 : ~0), so that both directions are an unsigned maximum; 0 is "no value yet" and the caller's initial value.
 *   table[D][F][B][hw] float, B = max_blocks: the extreme of every block whose LAST hour lies in this call is stored at index
 *     t / block, with plain 16-byte stores, exactly once.  Nothing else of table is touched.
 *   invalid[D][F] long long: += the NaN cell-hours; an ACCUMULATOR the caller zeroes once.
 * block_extremes_kernel: a workgroup of 256 owns (row, variable, chunk of 1024 cells); a thread owns 4 adjacent cells and walks the T
 * planes in order with 16-byte loads, 8 in flight, two integer compares a value; 4 bytes of LDS for the NaN count, one 64-bit integer
 * add per workgroup, no scratch, no host read-back, everything on the caller's stream.  Integer maxima commute: the table equals the
 * definition bit for bit for every cut of the time axis into calls.  Time is not split over workgroups.  Supported: hw a multiple of
 * 4, 1 <= block <= 2^20, 1 <= max_blocks <= 4096, M >= 1 (x, y, open, table 16-byte aligned); everything else returns
 * C2W_ERR_UNSUPPORTED and writes nothing.  T beyond 2^20, or a block that would end at or beyond index max_blocks, is
 * C2W_ERR_BAD_SHAPE.
 *
 * c2w_lmoments: table[R][n][hw] float (R = D F rows of n block extremes) -> lmom[R][4][hw] double, the sample L-moments l1 .. l4 of
 * each cell's n' <= n non-NaN extremes x_(0) <= .. <= x_(n' - 1), and n_valid[R][hw] int = n'.  With p = x_(n' / 2) the pivot and
 * e_j = x_(j) - p:  S_r = sum_j N_r(j) e_j in ascending j with N_0 = 1, N_1 = j, N_2 = j (j - 1), N_3 = j (j - 1)(j - 2);
 * b_r = S_r / (n' (n' - 1) .. (n' - r)), one division by an exact integer;  l1 = p + b_0, l2 = 2 b_1 - b_0, l3 = (6 b_2 - 6 b_1) + b_0,
 * l4 = ((20 b_3 - 30 b_2) + 12 b_1) - b_0; all in double on exactly converted fp32 values, no multiply fused with an add; l_r is NaN
 * where n' < r.  csrc/extremes_maps.h derives the error bound c_r(n') 2^-53 sum_j |e_j| (+ 2^-53 |l1| at r = 1).
 * lmoments_kernel: a thread holds the K x V extremes of V adjacent cells in registers (K = n rounded up to 8 / 16 / 32 / 64, V = 4, 4,
 * 2, 1), sorts them with the static Batcher network of c2w_crps_terms -- pads and NaNs are +inf and sort to the top -- and forms the
 * four moments; plain 8-byte stores, no LDS, no atomics, no scratch: the bits are the same at every position of the launch.
 * Supported: hw a multiple of 4, 1 <= n <= 64 (table 16-byte aligned); else C2W_ERR_UNSUPPORTED, nothing written.  R = 0 does nothing. */
int c2w_block_extremes_supported(int hw, int block, int max_blocks); /* 1 or 0 */
int c2w_block_extremes_update(const float* x, const float* y, const int* dir, unsigned* open, float* table, long long* invalid, int M, int T,
                              int F, int hw, int block, int max_blocks, long long t0, void* stream);
int c2w_lmoments_supported(int hw, int n); /* 1 or 0 */
int c2w_lmoments(const float* table, double* lmom, int* n_valid, long long R, int n, int hw, void* stream);
/* Co-moments of an ensemble (climate2weather_amd.dependence): do the variables still belong together, and does each member co-vary in
 * time with the truth?  Every score above judges a variable on its own.  Pearson correlation and the Taylor-diagram identity are the
 * textbook definitions (README, statement 17); they live in dependence.py as float64 tensor algebra on the tables below.
 *
 * Rows: d = 0 is the truth if y is given, then the M members; D = M + 1, or M without a truth.  x is [M][T][F][hw], y is [T][F][hw]
 * or NULL, dense fp32.  Hour t is VALID for (d, cell) iff all F values of row d at the cell and, with a truth, all F truth values at
 * the cell have an exponent field that is not all ones (infinities are invalid, not values).  An invalid hour adds nothing to
 * (d, cell) and is counted in invalid[d].
 *
 * c2w_comoments_update takes T >= 0 consecutive hours (T = 0 does nothing) and reads and writes the state, which the caller zeroed
 * when it made it:
 *   n[D][hw] int: the valid hours so far; 0 is "no pivot yet".
 *   pivot[D][F][hw], truth_pivot[D][F][hw] float: the row's and the truth's values at the first valid hour of (d, cell), never
 *     changed afterwards.  truth_pivot is not touched (and may be NULL) without a truth.
 *   sums[D][NS][hw] double: with e_f = (double)x_f - (double)P_f and eT_f = (double)y_f - (double)PT_f, per valid hour in hour order,
 *     each a plain s = s + term, no multiply fused with an add:  S[f] += e_f (F entries);  C[f,g] += e_f e_g for f <= g (F (F + 1) / 2
 *     entries in the order (0,0), (0,1) .. (0,F-1), (1,1) ..);  with a truth also ST[f] += eT_f, QT[f] += eT_f eT_f, X[f] += e_f eT_f
 *     (F entries each).  NS = 4 F + F (F + 1) / 2 with a truth, F + F (F + 1) / 2 without.  Row 0 has eT = e.
 *   invalid[D] long long: += the invalid cell-hours; an ACCUMULATOR the caller zeroes once.
 * comoments_update_kernel<F, TRUTH>: a workgroup of 256 owns (row, chunk of 256 V cells), V = 4 for F = 1, 2 for F = 2, 1 above; a
 * thread keeps the state of its V adjacent cells in registers, walks the T planes in order, 4 hours loaded in a straight line, and
 * stores the state where it loaded it; 4 bytes of LDS for the invalid count, one 64-bit integer add per workgroup, no atomics on
 * floats, no scratch, no host read-back, everything on the caller's stream.  One thread adds a series' terms in hour order, so the
 * tables are the same bit for bit at every position of a launch and for every cut of the hours into calls; csrc/comoments_maps.h
 * derives the error bound against exact arithmetic, (n + 1) 2^-53 sum |e| for S and ST, (n + 2) 2^-53 sum |e e| for the products.
 * Time is not split over workgroups.  Supported: hw a multiple of 4, 1 <= F <= 8, M >= 1 (x, y, n, pivot, truth_pivot, sums 16-byte
 * aligned); everything else returns C2W_ERR_UNSUPPORTED and writes nothing.  T beyond 2^20 is C2W_ERR_BAD_SHAPE: the host walks a
 * longer update in parts. */
int c2w_comoments_supported(int hw, int F); /* 1 or 0 */
int c2w_comoments_update(const float* x, const float* y, int* n, float* pivot, float* truth_pivot, double* sums, long long* invalid, int M, int T,
                         int F, int hw, void* stream);
/* Block moments at the observation grid (climate2weather_amd.scalesplit): averaged back to the coarse grid, does a member still
 * reproduce what it was conditioned on, and how much variability does it add below that grid?  For blocks of s x s cells with block
 * means m, sum (x - y)^2 = s^2 (m_x - m_y)^2 + sum ((x - m_x) - (y - m_y))^2 (README, statement 18); the scores live in scalesplit.py
 * as float64 tensor algebra on the tables below.
 *
 * Rows: d = 0 is the truth if y is given, then the M members; D = M + 1, or M without a truth.  x is [M][T][F][H][W], y is
 * [T][F][H][W] or NULL, dense fp32; h = H / s, w = W / s.  For each block of each (d, t, f) plane, cells x[r][c], r, c in 0 .. s-1:
 *   pivot[D][T][F][h][w] float: x[0][0], the fp32 value kept as its bits.
 *   n[D][T][F][h][w] int: the cells whose exponent field is not all ones (infinities are invalid, not values).
 *   sums[D][T][F][NS][h][w] double, NS = 3 with a truth and 2 without: with e = (double)x - (double)pivot and, from the truth's block
 *     and the truth's pivot, eT: the column sums A_c = sum_r e, Q_c = sum_r e e, X_c = sum_r e eT, each sequential from +0.0 in row
 *     order, then S1 = sum_c A_c, S2 = sum_c Q_c, X = sum_c X_c, each sequential from +0.0 in column order; every product rounded on
 *     its own, no multiply fused with an add.  A block with n < s^2 holds the canonical NaN 0x7ff8000000000000 in S1 and S2; X is that
 *     NaN if the block or the truth's block is invalid.  Row 0 carries the truth against itself (X == S2).
 * block_moments_kernel<S, TRUTH>: an item is (plane, block row, quad of 4 adjacent columns), the items of a row's planes numbered
 * flat; a workgroup of 256 takes 256 consecutive items, a thread walks its item's S rows with 16-byte loads, 8 rows in flight, and
 * keeps the 4 x NS column sums in registers; 26 KiB of LDS, one barrier, and the first thread of each block adds the S columns in
 * order and stores with plain stores.  No atomics, no scratch, no host read-back, everything on the caller's stream.  The order
 * fixes the bits: they are the same at every position of a launch; csrc/blockmoments_maps.h derives the error bound against exact
 * arithmetic, 2 s 2^-53 sum |e| for S1 and (2 s + 2) 2^-53 sum |e e| for S2 and X.  Supported: s in {4, 8, 16, 32}, H and W
 * multiples of s, M >= 1, F >= 1, the items of a row within an int and the grid within a launch (x, y 16-byte aligned); everything
 * else returns C2W_ERR_UNSUPPORTED and writes nothing.  T = 0 does nothing. */
int c2w_block_moments_supported(int H, int W, int s); /* 1 or 0 */
int c2w_block_moments(const float* x, const float* y, int* n, float* pivot, double* sums, int M, int T, int F, int H, int W, int s,
                      void* stream);
/* The network's output convolution (model/nn.py:194: 3x3, stride 1, zero padding) restricted to what the sampler's fold keeps
 * (src/thor/score.py:76-88: of a window's w * F output channels only the centre frame's F, all of them only for the first / last
 * window of a trajectory): rows r0 .. r0 + nr - 1 (nr <= 16) of the [wrows][9][Cin] weight matrix `w` over the NHWC rows `x`
 * ([B][H][W][Cin], 16-bit), bias added, rounded through the compute type like the full convolution's output, stored as fp32 planes:
 *     out[b * ostride + c * H * W + pix],  c < nr
 * -- with out = eps + (i0 + k) * F * H * W, ostride = F * H * W, r0 = k * F, nr = F the centre frames of windows i0 .. i0 + B - 1
 * land where fold() puts them, and no pass over the 128-channel output rows remains.  c2w_conv_center_supported: bf16 / fp16,
 * H % 8 == 0, W % 16 == 0, Cin in {64, 128}. */
int c2w_conv_center_supported(int H, int W, int Cin, int nr, int dtype);
int c2w_conv_center(const void* x, const void* w, const float* bias, float* out, int B, int H, int W, int Cin, int wrows, int r0, int nr,
                    long long ostride, int dtype, void* stream);
/* One-row fp32 Linear: y[r] = act(bias[r] + W[r][0..K) . x), W rows `ldk` floats apart; act = C2W_ACT_NONE / SILU / RELU.  The time
 * embedding MLP and the modulation projections (model/score.py:56-57,62-67; model/nn.py:149) when t is one value for the whole batch
 * (every network call of the sampler). */
int c2w_gemv_f32(const float* x, const float* W, const float* bias, float* y, int rows, int K, int ldk, int act, void* stream);
/* training_loop.py:385 (`loss.detach().item()` after optimizer.step()): the fp32 device scalar `src` is copied into host_slot[0]
 * (its bits) and host_slot[1] = seq is stored after it, release at system scope.  host_slot: two ints of pinned, device-visible host
 * memory; the host polls host_slot[1] for `seq` instead of synchronising the stream the value was produced on. */
int c2w_publish_scalar(const float* src, int* host_slot, int seq, void* stream);
/* model/score.py:14-34 */
int c2w_timestep_embedding(const float* t, float* out, int n, int dim, float max_period, void* stream);
/* src/thor/pipelines.py:13-20: musig[i] = {mu(t_i), sigma(t_i)} */
int c2w_mu_sigma(const float* t, float* musig, int n, float eta, void* stream);
int c2w_cast_f32(const float* in, void* out, long long n, int dtype, void* stream);
/* w[r][tap][k] (fp32, k-stride ldk) -> out[k][tap'][r] (dtype, r-stride ldr), taps reversed when flip: the operand of the
 * input-gradient convolution (dgrad = the same implicit GEMM over dy with these weights). */
int c2w_weight_transpose(const float* w, void* out, int R, int NT, int K, int ldk, int ldr, int flip, int dtype,
                         void* stream);
/* the same for nconv weight matrices in one launch: desc (device memory) holds 8 int64 per matrix
 * {w_off, out_off, R, NT, K, ldk, ldr, flip}, offsets in elements into flat / out */
int c2w_weight_transpose_batched(const float* flat, void* out, const long long* desc, int nconv, int dtype, void* stream);
/* Stage-major copies of 16-bit 3x3 conv weights for the 16x16-tile kernel (C2W_CONV_WPACKED), n matrices in one launch:
 * desc[j] = {src_off, dst_off, rows, cin} (offsets in ELEMENTS into src / dst; src matrix [rows][9][cin], cin a multiple of 32):
 *   dst[((tap * (cin / 32) + h) * rows_pad + r) * 32 + ((q ^ swz(r)) * 8) + e] = src[r][tap][h * 32 + q * 8 + e],  rows_pad = rows
 *   rounded up to 128, zero for r >= rows, swz(r) = (4 - ((r >> 2) & 3)) & 3 (the kernel's LDS swizzle, baked in).
 * The kernel then fetches the 128 rows x 64 B of a (tap, 32-channel half) as ONE contiguous 8 KiB block instead of 128 row pieces
 * 9 * cin * 2 bytes apart: 4.7 % of the dominant launch (profiles/r03_experiments.md section 11).  Size of a packed matrix:
 * 9 * cin * rows_pad elements. */
int c2w_pack_conv_weights_batched(const void* src, void* dst, const long long* desc, int n, int dtype, void* stream);
/* 1 when c2w_conv_forward takes args with C2W_CONV_WPACKED set (the launch goes to the 16x16-tile halo-patch kernel), else 0. */
int c2w_conv_wpacked_supported(const C2wConvArgs* args, int dtype);
/* fused torch.optim.AdamW step (train.py:176-181) + EMA (src/thor/ema.py:23-27) + bf16 shadow refresh over a flat
 * parameter buffer; ema / shadow_bf16 may be NULL; g is multiplied by grad_scale first. */
int c2w_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, void* shadow_bf16, long long n, float lr,
                  float beta1, float beta2, float eps, float weight_decay, int step, float ema_rate, float grad_scale,
                  void* stream);

/* The same step with a 16-bit weight shadow of either format (shadow_dtype = C2W_DTYPE_BF16 / C2W_DTYPE_F16) and, when
 * scaler_state != NULL, under the dynamic loss scale: g is divided by scaler_state[0]; if scaler_state[2] (found_inf) is
 * set the step changes nothing but the EMA; the Adam bias corrections use scaler_state[3] + 1 (steps actually taken)
 * instead of `step`. */
int c2w_adamw_ema_scaled(float* p, const float* g, float* m, float* v, float* ema, void* shadow, int shadow_dtype,
                         long long n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                         float ema_rate, float grad_scale, const float* scaler_state, void* stream);

/* Dynamic loss scale for fp16 training, resident on the device: torch.cuda.amp.GradScaler's rule, which Fabric's
 * precision="16-mixed" (train.py:98) wraps around fabric.backward / optimizer.step (training_loop.py:378,383).
 * state: 4 floats in device memory {scale, growth tracker, found_inf, optimizer steps taken}.  One step =
 *   loss gradient x state[0] (c2w_mse_loss_grad_scaled) -> backward -> [all-reduce] -> c2w_grad_scaler_check (found_inf = any
 *   non-finite gradient; identical on every rank after the all-reduce) -> c2w_adamw_ema_scaled -> c2w_grad_scaler_update
 *   (overflow: scale *= backoff, tracker = 0; else steps += 1, tracker += 1, and scale *= growth every growth_interval
 *   clean steps).  No host synchronisation anywhere; the host may read the state whenever it likes. */
int c2w_grad_scaler_init(float* state, float init_scale, void* stream);
int c2w_grad_scaler_check(const float* g, long long n, float* state, void* stream);
int c2w_grad_scaler_update(float* state, float growth, float backoff, int growth_interval, void* stream);

/* p_ema = rate * p_ema + (1 - rate) * p over a flat buffer (src/thor/ema.py:23-27) */
int c2w_ema_update(float* ema, const float* p, long long n, float rate, void* stream);

/* QKVAttention, one head (model/nn.py:62-85).  qkv: [B][T][3C] (q|k|v), o: [B][T][C], lse: [B][T] fp32 (may be NULL
 * for inference).  backward recomputes probabilities from lse; delta_ws is a [B][T] fp32 scratch. */
int c2w_attention_forward(const void* qkv, void* o, float* lse, int B, int T, int C, int dtype, void* stream);
int c2w_attention_backward(const void* qkv, const void* o, const void* d_o, const float* lse, float* delta_ws, void* dqkv,
                           int B, int T, int C, int dtype, void* stream);

/* ---- device-resident sampler (replaces the CPU-resident state + per-batch PCIe round trips of
 * src/thor/score.py:156-185 and the elementwise updates of src/thor/pipelines.py:41-91) ---- */
/* unfold, src/thor/score.py:68-74: windows i0..i0+nw-1 of x[L][F][HW] (fp32) -> NHWC rows [nw*HW][ldc], channel = tau*F + c */
int c2w_window_gather(const float* x, void* y, int nw, int F, int HW, int k, int i0, int ldc, int dtype, void* stream);
/* fold, src/thor/score.py:76-88: centre frame of every window (+ leading k of window 0, trailing k of the last) -> eps[L][F][HW] */
int c2w_window_scatter(const void* y, float* eps, int nw, int F, int HW, int k, int i0, int nwin_total, int ldc,
                       int dtype, void* stream);
/* predictor, src/thor/pipelines.py:41-46: x = a*x + b*eps with a = mu'/mu, b = sigma' - mu' sigma/mu; non-finite -> *nan_flag |= 1 */
int c2w_sampler_predict(float* x, const float* eps, int* nan_flag, long long n, float a, float b, void* stream);
/* out[0] += sum v^2 */
int c2w_sumsq(const float* v, float* out, long long n, void* stream);
/* corrector, src/thor/pipelines.py:81-88: delta = tau/(sumsq[0]/n); x -= (delta eps + sqrt(2 delta) z) sigma_next */
int c2w_sampler_correct(float* x, const float* eps, const float* z, const float* sumsq, int* nan_flag, long long n,
                        float tau, float sigma_next, void* stream);
/* likelihood guidance for A = AvgPool2d(s_step) o x[::t_step] (exp/downscaling.py:129-132) with exact_grad=False
 * (src/thor/score.py:24-57): eps -= sigma/mu * A^T((y - A((x - sigma eps)/mu)) / (std_c^2 + gamma (sigma/mu)^2)), in place */
int c2w_guidance(const float* x, float* eps, const float* yobs, const float* stdv, int nobs, int F, int H, int W,
                 int s_step, int t_step, float mu, float sigma, float gamma, void* stream);
/* the same with one gamma per variable, gammav[F] in device memory: what exp/downscaling.py:228-233 hands condition_on for a
 * list-valued `likelihood_gamma` (a (1, C, 1, 1) tensor that src/thor/score.py:55 broadcasts against err) */
int c2w_guidance_per_variable(const float* x, float* eps, const float* yobs, const float* stdv, const float* gammav, int nobs,
                              int F, int H, int W, int s_step, int t_step, float mu, float sigma, void* stream);
/* ---- exact guidance (src/thor/score.py:24-35 with exact_grad=True) streamed over the windows whose kept frames are observed.  A batch of
 * n such windows is two device lists: first[j] = index of the window's first frame in the flattened [members * L] frame array (m * L + i),
 * kind[j] = bit 0: its trajectory's first window, bit 1: its last. ---- */
/* c2w_guidance / c2w_guidance_per_variable (gammav_or_null: one gamma per variable, else the scalar `gamma`) with eps only READ:
 * delta[nobs][F][H][W] = the term those add to eps on the observed frames (eps[o * t_step] + delta[o] reproduces them bit for bit) */
int c2w_guidance_delta(const float* x, const float* eps, const float* yobs, const float* stdv, const float* gammav_or_null, float gamma,
                       float* delta, int nobs, int F, int H, int W, int s_step, int t_step, float mu, float sigma, void* stream);
/* c2w_window_gather for a list: y[j*HW + p][tau*F + f] = x[first[j] + tau][f][p], channels >= (2k+1) F zero */
int c2w_window_gather_list(const float* x, void* y, const int* first, int n, int F, int HW, int k, int ldc, int dtype, void* stream);
/* adjoint of fold: dy[j*HW + p][tau*F + f] = delta[first[j] / L][frame / t_step][f][p] where slot tau of window j is kept (tau == k; tau < k
 * with kind bit 0; tau > k with kind bit 1) and frame = first[j] % L + tau is observed (frame % t_step == 0, frame / t_step < nobs); every
 * other element of the row, padding included, is zero.  delta: [members][nobs][F][HW] fp32; rows in the compute type */
int c2w_window_cotangent_list(const float* delta, void* dy, const int* first, const int* kind, int n, int L, int F, int HW, int k,
                              int t_step, int nobs, int ldc, int dtype, void* stream);
/* adjoint of the gather: out[l][f][p] += scale * sum_j dx[j][(l - first[j]) F + f][p] over the j with first[j] <= l <= first[j] + 2k, added in
 * ascending j by the one thread that owns the element (no atomics: bit-identical launch to launch), for the frames l0 <= l < l0 + nl;
 * frames no window of the list contains are left untouched.  dx: [n][(2k+1) F][HW] fp32 */
int c2w_window_grad_fold_list(const float* dx, float* out, const int* first, int n, int l0, int nl, int F, int HW, int k, float scale,
                              void* stream);
/* the measurement operator itself: y[o][c][ph][pw] = mean of the s x s cell of x[o*t_step][c] (exp/downscaling.py:129-132) */
int c2w_pool_stride(const float* x, float* y, int nobs, int F, int H, int W, int s_step, int t_step, void* stream);
/* per-variable affine map over (planes = L*F) planes of HW values: y = x * scale[c] + shift[c], c = plane % F -- the quantile
 * normalisation / de-normalisation of data/pipeline.py:183-244 either side of the sampler (x == y allowed) */
int c2w_affine_channels(const float* x, float* y, const float* scale, const float* shift, long long planes, int F, int HW,
                        void* stream);

/* library identity: returns the gfx target string the kernels were compiled for ("gfx950") */
/* Run-time knobs (dispatch overrides for tests and opt-in modes: C2W_FORCE_GATHER, C2W_CONV_T3, C2W_CONV_S2_PATCH, C2W_TS2_PAIRS,
 * C2W_WGRAD_ATOMICS, C2W_ATTN_VALU, C2W_NO_LOSS_FUSION, C2W_NO_HALF8, C2W_HALF8_DB; csrc/knobs.h) are
 * read from the environment once, when the library is loaded; this re-reads them. */
void c2w_knobs_reload(void);

const char* c2w_target(void);
/* provenance: hex sha256 over the sources (csrc/, include/c2w_hip.h, compile flags) this library was built from; the Python loader
 * refuses a library whose digest differs from the source tree next to it (climate2weather_amd/build.py) */
const char* c2w_sources_sha256(void);

#ifdef __cplusplus
}
#endif
#endif /* C2W_HIP_H */
