// Run-time knobs of libc2w_hip.so -- ALL of them: each is either set by a test that runs both sides of a dispatch on one shape or selects
// an opt-in whose trade-off is open (DESIGN.md section 10 lists them with the test that exercises the non-default value, and the retired
// ones with the measurement that settled them).  None changes a result beyond the kernels' own rounding.  The environment is read ONCE,
// at the first launch; c2w_knobs_reload() (exported) re-reads it -- a test that flips a knob inside one process calls it afterwards.
#pragma once

struct C2wKnobs {
    bool force_gather;    // C2W_FORCE_GATHER=1   every conv / weight gradient on the general gather kernels (no halo-patch kernels)
    int conv_t3;          // C2W_CONV_T3          -1 (default): 16x16-tile conv kernel from 512 workgroups; 0: never; 16: wherever the image is tiled
    int conv_s2_patch;    // C2W_CONV_S2_PATCH    0 (default): stride-2 FORWARD on the gather kernel; 1: on the parity-plane halo-patch kernel where it pays (>= 4 K chunks or <= 2048 workgroups); 2: wherever the geometry allows
    bool ts2_pairs;       // C2W_TS2_PAIRS=0      stride-2 input gradient with one class per workgroup (round 4) instead of two (round 6; 16-bit)
    bool wgrad_atomics;   // C2W_WGRAD_ATOMICS=1  split-K partial sums by fp32 atomics even when a workspace is handed over
    bool attn_valu;       // C2W_ATTN_VALU=1      attention on the fp32 VALU kernels instead of the matrix-core ones
    bool loss_fusion;     // C2W_NO_LOSS_FUSION=1 c2w_conv_loss_supported answers 0 (callers run the output conv and c2w_mse_loss_grad_noise)
    bool half8;           // C2W_NO_HALF8=1       every 8x16-tile launch on the 4-wave kernel (rounds 1-5)
    bool half8_db;        // C2W_HALF8_DB=0       eight-wave launches of at most 256 workgroups with ONE patch buffer (an exposed patch load per K chunk)
};

const C2wKnobs& c2w_knobs();
extern "C" void c2w_knobs_reload(void);
