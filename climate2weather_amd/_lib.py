"""ctypes binding of libc2w_hip.so (the C ABI declared in include/c2w_hip.h).

The product path has no CPU fallback: if the library is missing or a call fails this module raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int, c_int32, c_longlong, c_ulonglong, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("C2W_LIB") or os.path.join(HERE, "libc2w_hip.so")  # C2W_LIB: diagnostic builds only

DTYPE_F32, DTYPE_BF16, DTYPE_F16 = 0, 1, 2
CONV_1X1, CONV_S1, CONV_S2, CONV_UP, CONV_TS2 = 0, 1, 2, 3, 4
ACT_NONE, ACT_SILU, ACT_SILU_PAIR, ACT_RELU, ACT_RELU_PAIR = 0, 1, 2, 3, 4
MUL_PLAIN, MUL_DSILU = 0, 1
CONV_POOL2, CONV_WPACKED, CONV_NO_Y, CONV_DETERMINISTIC = 1, 2, 4, 8  # ConvArgs.flags (bit set)
KERNEL_GATHER, KERNEL_PATCH_8X16, KERNEL_PATCH_16X16, KERNEL_PATCH_PAIR, KERNEL_PATCH_TS2, KERNEL_PATCH_S2 = 0, 1, 2, 3, 4, 5  # c2w_conv_dispatch


class C2wError(RuntimeError):
    pass


class ConvArgs(Structure):
    _fields_ = [
        ("x", c_void_p), ("w", c_void_p), ("bias", c_void_p), ("res", c_void_p), ("mul", c_void_p), ("y", c_void_p), ("y2", c_void_p),
        ("B", c_int32), ("Hin", c_int32), ("Win", c_int32), ("Cin", c_int32),
        ("Hout", c_int32), ("Wout", c_int32), ("Cout", c_int32), ("ldy", c_int32),
        ("wrows", c_int32), ("mode", c_int32), ("act", c_int32), ("mulmode", c_int32),
        ("ln_x", c_void_p), ("ln_m", c_void_p), ("ln_dm", c_void_p), ("ln_ldm", c_int32), ("ln_unbiased", c_int32),
        ("ln_eps", c_float), ("flags", c_int32), ("lnf_y", c_void_p), ("lnf_m", c_void_p), ("kvalid", c_int32),
        ("lnf_rstd", c_void_p), ("ln_rstd", c_void_p),
        ("lnf_mean", c_void_p), ("res_rstd", c_void_p), ("res_mean", c_void_p), ("res_m", c_void_p),
        ("loss_sum", c_void_p), ("loss_scaler", c_void_p), ("loss_eps", c_void_p), ("loss_gscale", c_float), ("loss_C", c_int32),
        ("loss_lde", c_int32), ("splitk_ws", c_void_p), ("splitk_ws_bytes", c_ulonglong), ("splitk", c_int32),
        ("det_ws", c_void_p), ("det_ws_bytes", c_ulonglong),
    ]


class WgradItem(Structure):  # C2wWgradItem
    _fields_ = [("x", c_void_p), ("dy", c_void_p), ("dw", c_void_p), ("dbias", c_void_p)]


# name -> argtypes (every function returns int status except c2w_target)
_PROTOS = {
    "c2w_conv_forward": [POINTER(ConvArgs), c_int, c_int, c_void_p],
    "c2w_conv_lnbwd_supported": [POINTER(ConvArgs), c_int],
    "c2w_conv_lnfwd_supported": [POINTER(ConvArgs), c_int],
    "c2w_conv_loss_supported": [POINTER(ConvArgs), c_int],
    "c2w_conv_splitk_plan": [POINTER(ConvArgs), c_int, POINTER(c_ulonglong)],
    "c2w_conv_lnfwd_chain_supported": [POINTER(ConvArgs), c_int],
    "c2w_conv_det_scratch_bytes": [POINTER(ConvArgs), c_int],
    "c2w_conv_patch_supported": [POINTER(ConvArgs), c_int],
    "c2w_conv_pool2_supported": [POINTER(ConvArgs), c_int],
    "c2w_conv_dispatch": [POINTER(ConvArgs), c_int],
    "c2w_conv_wgrad_dispatch": [POINTER(ConvArgs), c_int],
    "c2w_upsample2": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_conv_wgrad": [POINTER(ConvArgs), c_void_p, c_void_p, c_void_p, c_ulonglong, c_int, c_void_p],
    "c2w_conv_wgrad_workspace_bytes": [POINTER(ConvArgs), c_int],
    "c2w_conv_wgrad_grouped_supported": [POINTER(ConvArgs), c_int, c_int],
    "c2w_conv_wgrad_grouped_workspace_bytes": [POINTER(ConvArgs), c_int, c_int],
    "c2w_conv_wgrad_grouped": [POINTER(ConvArgs), POINTER(WgradItem), c_int, c_void_p, c_ulonglong, c_int, c_void_p],
    "c2w_ln_forward": [c_void_p, c_void_p, c_void_p, c_longlong, c_int, c_int, c_int, c_float, c_int, c_int, c_void_p],
    "c2w_ln_backward": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_longlong, c_int, c_int, c_int, c_float, c_int,
                        c_int, c_void_p],
    "c2w_ln_backward_det": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_longlong, c_int, c_int, c_int, c_float, c_int,
                            c_void_p, c_ulonglong, c_int, c_void_p],
    "c2w_ln_backward_det_scratch_bytes": [c_longlong, c_int, c_int, c_int],
    "c2w_colsum": [c_void_p, c_void_p, c_longlong, c_int, c_int, c_int, c_void_p],
    "c2w_colsum_det": [c_void_p, c_void_p, c_longlong, c_int, c_int, c_void_p, c_ulonglong, c_int, c_void_p],
    "c2w_colsum_det_scratch_bytes": [c_longlong, c_int],
    "c2w_silu": [c_void_p, c_void_p, c_longlong, c_int, c_void_p],
    "c2w_silu_backward": [c_void_p, c_void_p, c_void_p, c_longlong, c_int, c_void_p],
    "c2w_sumpool2": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_nchw_to_nhwc": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_nhwc_to_nchw": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_mse_loss_grad": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_int, c_void_p],
    "c2w_mse_loss_grad_scaled": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_int, c_void_p],
    "c2w_philox_normal": [c_void_p, c_longlong, c_ulonglong, c_void_p],
    "c2w_nchw_to_nhwc_noise_rows": [c_void_p, c_void_p, c_ulonglong, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_nchw_to_nhwc_noise": [c_void_p, c_ulonglong, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_windows_to_nhwc_noise": [c_void_p, c_void_p, c_ulonglong, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_mse_loss_grad_noise": [c_void_p, c_ulonglong, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_int, c_void_p],
    "c2w_sq_err": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_sq_err_noise": [c_void_p, c_ulonglong, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_loss_det_scratch_bytes": [],
    "c2w_mse_loss_grad_det": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_ulonglong, c_int,
                              c_void_p],
    "c2w_mse_loss_grad_noise_det": [c_void_p, c_ulonglong, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_ulonglong,
                                    c_int, c_void_p],
    "c2w_sq_err_det": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_ulonglong, c_int, c_void_p],
    "c2w_sq_err_noise_det": [c_void_p, c_ulonglong, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_ulonglong, c_int, c_void_p],
    "c2w_sq_err_levels_scratch_bytes": [c_int, c_int, c_int],
    "c2w_sq_err_levels": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_ulonglong,
                          c_int, c_void_p],
    "c2w_sq_err_levels_noise": [c_void_p, c_ulonglong, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                c_ulonglong, c_int, c_void_p],
    "c2w_rapsd_supported": [c_int, c_int],
    "c2w_rapsd": [c_void_p, c_void_p, c_longlong, c_int, c_int, c_void_p],
    "c2w_ssim_supported": [c_int, c_int, c_int],
    "c2w_ssim": [c_void_p, c_void_p, c_void_p, c_void_p, c_longlong, c_longlong, c_int, c_int, c_int, c_void_p],
    "c2w_swd_supported": [c_int, c_int, c_int],
    "c2w_swd_project": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_longlong, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_swd_project_pair": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_longlong, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_swd_distance": [c_void_p, c_void_p, c_void_p, c_longlong, c_int, c_int, c_int, c_void_p],
    "c2w_kde_supported": [c_int, c_int],
    "c2w_kde_scratch_bytes": [c_longlong, c_longlong, c_int],
    "c2w_kde_eval": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_ulonglong, c_void_p, c_longlong, c_int, c_int, c_int, c_int,
                     c_void_p],
    "c2w_kde_partial": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_ulonglong, c_longlong, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_kde_fold": [c_void_p, c_void_p, c_void_p, c_longlong, c_longlong, c_int, c_void_p],
    "c2w_pit_supported": [c_int, c_int],
    "c2w_pit_counts": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_quantile_supported": [c_int, c_int],
    "c2w_quantile_scratch_bytes": [c_longlong, c_int],
    "c2w_quantiles": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_ulonglong, c_void_p, c_void_p, c_void_p, c_longlong, c_int, c_int, c_int,
                      c_void_p],
    "c2w_crps_supported": [c_int, c_int],
    "c2w_crps_scratch_bytes": [c_int, c_int, c_int],
    "c2w_crps_terms": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_ulonglong, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_wind_supported": [c_int, c_int],
    "c2w_wind_table_bytes": [c_int],
    "c2w_wind_table": [c_void_p, c_void_p, c_int, c_void_p],
    "c2w_wind_scratch_bytes": [c_longlong, c_int],
    "c2w_wind_power": [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p, c_ulonglong, c_longlong, c_int, c_void_p],
    "c2w_escore_supported": [c_int, c_int],
    "c2w_escore_scratch_bytes": [c_longlong, c_int, c_int],
    "c2w_escore_pairs": [c_void_p, c_void_p, c_void_p, c_void_p, c_ulonglong, c_int, c_longlong, c_int, c_void_p],
    "c2w_vario_supported": [c_int, c_int, c_int, c_int, c_int],
    "c2w_vario_scratch_bytes": [c_longlong, c_int, c_int, c_int],
    "c2w_vario_terms": [c_void_p, c_void_p, c_void_p, c_void_p, c_ulonglong, c_int, c_longlong, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_tincr_supported": [c_int, c_int],
    "c2w_tincr_scratch_bytes": [c_longlong, c_int, c_int, c_int, c_int],
    "c2w_tincr_terms": [c_void_p, c_void_p, c_void_p, c_void_p, c_ulonglong, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_qmap_supported": [c_int, c_int, c_int],
    "c2w_qmap_scratch_bytes": [c_longlong, c_int, c_int],
    "c2w_qmap_nodes": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_ulonglong, c_longlong, c_int, c_int, c_int, c_int,
                       c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_qmap_apply": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_longlong, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                       c_void_p],
    "c2w_event_counts_supported": [c_int, c_int, c_int],
    "c2w_event_counts": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_fss_supported": [c_int, c_int, c_int, c_int, c_void_p, c_int],
    "c2w_fss_sums": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_spell_supported": [c_int, c_int, c_int, c_int],
    "c2w_spell_update": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                         c_int, c_longlong, c_void_p],
    "c2w_objects_supported": [c_int, c_int, c_int, c_int, c_int],
    "c2w_object_tables": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                          c_int, c_int, c_void_p],
    "c2w_block_extremes_supported": [c_int, c_int, c_int],
    "c2w_block_extremes_update": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_longlong,
                                  c_void_p],
    "c2w_lmoments_supported": [c_int, c_int],
    "c2w_lmoments": [c_void_p, c_void_p, c_void_p, c_longlong, c_int, c_int, c_void_p],
    "c2w_comoments_supported": [c_int, c_int],
    "c2w_comoments_update": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_block_moments_supported": [c_int, c_int, c_int],
    "c2w_block_moments": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_timestep_embedding": [c_void_p, c_void_p, c_int, c_int, c_float, c_void_p],
    "c2w_mu_sigma": [c_void_p, c_void_p, c_int, c_float, c_void_p],
    "c2w_publish_scalar": [c_void_p, c_void_p, c_int, c_void_p],
    "c2w_gemv_f32": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_conv_center_supported": [c_int, c_int, c_int, c_int, c_int],
    "c2w_conv_center": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_longlong, c_int, c_void_p],
    "c2w_cast_f32": [c_void_p, c_void_p, c_longlong, c_int, c_void_p],
    "c2w_weight_transpose": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_weight_transpose_batched": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "c2w_pack_conv_weights_batched": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p],
    "c2w_conv_wpacked_supported": [POINTER(ConvArgs), c_int],
    "c2w_adamw_ema": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_longlong, c_float, c_float, c_float, c_float,
                      c_float, c_int, c_float, c_float, c_void_p],
    "c2w_adamw_ema_scaled": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_longlong, c_float, c_float, c_float,
                             c_float, c_float, c_int, c_float, c_float, c_void_p, c_void_p],
    "c2w_grad_scaler_init": [c_void_p, c_float, c_void_p],
    "c2w_grad_scaler_check": [c_void_p, c_longlong, c_void_p, c_void_p],
    "c2w_grad_scaler_update": [c_void_p, c_float, c_float, c_int, c_void_p],
    "c2w_ema_update": [c_void_p, c_void_p, c_longlong, c_float, c_void_p],
    "c2w_attention_forward": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_attention_backward": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_window_gather": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_window_scatter": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_sampler_predict": [c_void_p, c_void_p, c_void_p, c_longlong, c_float, c_float, c_void_p],
    "c2w_sumsq": [c_void_p, c_void_p, c_longlong, c_void_p],
    "c2w_sampler_correct": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_longlong, c_float, c_float, c_void_p],
    "c2w_guidance": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_float,
                     c_void_p],
    "c2w_guidance_per_variable": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float,
                                  c_void_p],
    "c2w_guidance_delta": [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                           c_float, c_void_p],
    "c2w_window_gather_list": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_window_cotangent_list": [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_window_grad_fold_list": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p],
    "c2w_pool_stride": [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p],
    "c2w_affine_channels": [c_void_p, c_void_p, c_void_p, c_void_p, c_longlong, c_int, c_int, c_void_p],
}

_lib = None


def exported_symbols():
    """Names include/c2w_hip.h declares (used by the CPU test that the library exports all of them)."""
    return list(_PROTOS) + ["c2w_target", "c2w_sources_sha256", "c2w_knobs_reload"]


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise C2wError(f"{LIB_PATH} is missing: run `python -m climate2weather_amd.build` (hipcc, gfx950). "
                       "There is no CPU fallback for the product path.")
    if not os.environ.get("C2W_LIB") and os.environ.get("C2W_ALLOW_STALE_LIB", "") in ("", "0"):
        from . import build as _build  # content hash of csrc/ + include/ against the digest linked into the library
        if os.path.isdir(_build.CSRC) and _build._stale():
            raise C2wError(f"{LIB_PATH} was not built from the sources on disk (the digest compiled into it, c2w_sources_sha256 = "
                           f"{_build.embedded_digest()}, differs from sha256(csrc/, include/) = {_build.sources_digest()[:16]}...): run "
                           "`python -m climate2weather_amd.build`.  Refusing to run kernels that do not match the source tree.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in _PROTOS.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.argtypes = argtypes
        fn.restype = c_longlong if name.endswith("_bytes") else c_int
    lib.c2w_knobs_reload.restype = None
    lib.c2w_knobs_reload.argtypes = []
    for name in ("c2w_target", "c2w_sources_sha256"):
        getattr(lib, name).restype = c_char_p
        getattr(lib, name).argtypes = []
    _lib = lib
    return lib


def check(status: int, what: str) -> None:
    if status != 0:
        kind = {-1: "bad argument", -2: "bad shape", -3: "unsupported"}.get(status, f"hipError_t {status}")
        raise C2wError(f"{what} failed: {kind}")
