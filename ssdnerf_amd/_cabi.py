"""ctypes binding of libssdnerf_hip.so (the C ABI declared in include/ssdnerf_hip.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; the library receives raw
device pointers.  There is NO fallback: if the shared library is missing or fails to load, importing
any operator raises immediately (the product path never routes through the CPU oracle).
"""
from __future__ import annotations

import ctypes  # re-exported as C.ctypes for the drop-in modules
import os
from typing import Optional

import torch

# SSDNERF_HIP_LIB: another build of the SAME library (e.g. one compiled with experimental -D flags into .variants/) for A/B runs
_LIB_PATH = os.environ.get("SSDNERF_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libssdnerf_hip.so")
_lib: Optional[ctypes.CDLL] = None

ABI_VERSION = 3
F32, F16 = 0, 1
BF16 = 2        # (the prior-loss entries and the scene cache; ``dtype_code`` serves the fp32 / fp16 operators)

EXPORTS = [
    "ssdnerf_last_error", "ssdnerf_abi_version", "ssdnerf_near_far_from_aabb", "ssdnerf_sph_from_ray", "ssdnerf_morton3D",
    "ssdnerf_morton3D_invert", "ssdnerf_packbits", "ssdnerf_march_rays_train_workspace", "ssdnerf_march_rays_train",
    "ssdnerf_march_rays_train_batch_workspace", "ssdnerf_march_rays_train_batch_count", "ssdnerf_march_rays_train_batch_write",
    "ssdnerf_composite_rays_train_forward", "ssdnerf_composite_rays_train_backward", "ssdnerf_march_rays", "ssdnerf_composite_rays",
    "ssdnerf_sh_encode_forward", "ssdnerf_sh_encode_backward", "ssdnerf_triplane_pack", "ssdnerf_point_decode", "ssdnerf_point_decode_backward_workspace",
    "ssdnerf_point_decode_backward", "ssdnerf_point_decode_backward_layout",
    "ssdnerf_point_decode_backward_params_workspace", "ssdnerf_point_decode_backward_params",
    "ssdnerf_render_rays_fused", "ssdnerf_render_rays_fused_batch", "ssdnerf_render_queue_workspace", "ssdnerf_render_first_hit",
    "ssdnerf_render_shade_queue", "ssdnerf_render_shade_queue_mfma", "ssdnerf_render_first_hit_cams", "ssdnerf_render_shade_queue_mfma_cams", "ssdnerf_density_grid_update", "ssdnerf_packbits_dev_thresh", "ssdnerf_ddim_step_v",
    "ssdnerf_group_norm_workspace", "ssdnerf_group_norm_backward_workspace", "ssdnerf_group_norm_nhwc", "ssdnerf_group_norm_nhwc_runs", "ssdnerf_group_norm_nhwc_backward", "ssdnerf_group_norm_nhwc_backward_cat", "ssdnerf_bias_residual_nhwc",
    "ssdnerf_conv2d_nhwc_bf16_supported", "ssdnerf_conv2d_nhwc_bf16_plan", "ssdnerf_conv2d_nhwc_bf16", "ssdnerf_conv2d_nhwc_f32x2", "ssdnerf_conv2d_nhwc_f32x2_plan", "ssdnerf_attention_qkv_bf16", "ssdnerf_attention_qkv_f32", "ssdnerf_attention_qkv_f32_lse", "ssdnerf_attention_qkv_f32_backward", "ssdnerf_cam_rays", "ssdnerf_quantize_u8",
    "ssdnerf_marching_cubes_count", "ssdnerf_marching_cubes_emit", "ssdnerf_conv2d_nhwc_f32x2_presplit_supported", "ssdnerf_conv2d_nhwc_f32x2_presplit", "ssdnerf_split_f32_nhwc",
    "ssdnerf_image_metrics", "ssdnerf_tv_loss_forward", "ssdnerf_tv_loss_backward", "ssdnerf_mesh_vertex_attributes",
    "ssdnerf_lpips_input", "ssdnerf_relu_pool_nhwc", "ssdnerf_lpips_layer_workspace", "ssdnerf_lpips_layer",
    "ssdnerf_feature_moments_accumulate", "ssdnerf_kid_subset_sums_workspace", "ssdnerf_kid_subset_sums",
    "ssdnerf_adam_max_tensors", "ssdnerf_adam_step_multi",
    "ssdnerf_gather_views_u8", "ssdnerf_sample_rays_u8", "ssdnerf_perm_indices", "ssdnerf_sample_rays_perm_u8",
    "ssdnerf_ema_chunk", "ssdnerf_ema_plan_build", "ssdnerf_ema_update_multi",
    "ssdnerf_cache_max_scenes", "ssdnerf_cache_load_multi", "ssdnerf_cache_store_multi",
    "ssdnerf_dpmpp_step_v", "ssdnerf_dpmpp_block_cap",
    "ssdnerf_png_filter_rows", "ssdnerf_code_plane_rgb",
    "ssdnerf_philox_normal_fill", "ssdnerf_sde_step_v", "ssdnerf_sde_block_cap",
    "ssdnerf_prior_q_sample", "ssdnerf_prior_loss_v", "ssdnerf_prior_loss_v_backward", "ssdnerf_prior_block_cap", "ssdnerf_prior_blocks_per_sample",
    "ssdnerf_prior_loss_partials",
]


class AdamTensor(ctypes.Structure):
    """``ssdnerf_adam_tensor`` (include/ssdnerf_hip.h): one row of the table ``ssdnerf_adam_step_multi`` steps in a launch"""
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("numel", ctypes.c_uint64), ("step_size", ctypes.c_float), ("bc2_sqrt", ctypes.c_float), ("weight_decay", ctypes.c_float),
                ("reserved", ctypes.c_uint32)]


class EmaRow(ctypes.Structure):
    """``ssdnerf_ema_row`` (include/ssdnerf_hip.h): one (source, EMA) tensor pair of the plan ``ssdnerf_ema_update_multi`` launches over"""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("numel", ctypes.c_uint64), ("trainable", ctypes.c_uint32),
                ("first_block", ctypes.c_uint32)]


class CacheStore(ctypes.Structure):
    """``ssdnerf_cache_store`` (include/ssdnerf_hip.h): the five device arrays of the scene cache, their sizes and dtype codes (0 fp32, 1 fp16, 2 bf16)"""
    _fields_ = [("code", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p), ("density_grid", ctypes.c_void_p),
                ("density_bitfield", ctypes.c_void_p), ("slots", ctypes.c_uint64), ("numel", ctypes.c_uint64), ("grid_bytes", ctypes.c_uint64),
                ("bits_bytes", ctypes.c_uint64), ("code_dtype", ctypes.c_int32), ("moment_dtype", ctypes.c_int32)]


class CacheRow(ctypes.Structure):
    """``ssdnerf_cache_row`` (include/ssdnerf_hip.h): one (slot, batch row, has_state) entry of ``ssdnerf_cache_load_multi`` / ``_store_multi``"""
    _fields_ = [("slot", ctypes.c_uint32), ("row", ctypes.c_uint32), ("has_state", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


def lib_path() -> str:
    return _LIB_PATH


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(
                f"libssdnerf_hip.so not found at {_LIB_PATH}: build it with `python -m ssdnerf_amd.build` "
                "(there is no CPU fallback for the product path)")
        l = ctypes.CDLL(_LIB_PATH)
        l.ssdnerf_last_error.restype = ctypes.c_char_p
        l.ssdnerf_abi_version.restype = ctypes.c_int
        l.ssdnerf_march_rays_train_workspace.restype = ctypes.c_size_t
        l.ssdnerf_march_rays_train_workspace.argtypes = [ctypes.c_uint32]
        l.ssdnerf_render_queue_workspace.restype = ctypes.c_size_t
        l.ssdnerf_render_queue_workspace.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
        l.ssdnerf_march_rays_train_batch_workspace.restype = ctypes.c_size_t
        l.ssdnerf_march_rays_train_batch_workspace.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        l.ssdnerf_triplane_pack.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_uint32] * 4 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        l.ssdnerf_point_decode.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 3 + [ctypes.c_uint32, ctypes.c_float] + \
                                          [ctypes.c_void_p] * 3
        l.ssdnerf_point_decode_backward.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_uint32] * 3 + [ctypes.c_void_p] * 4 + [ctypes.c_uint32, ctypes.c_float] + \
                                                   [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_void_p]
        l.ssdnerf_point_decode_backward_workspace.restype = ctypes.c_size_t
        l.ssdnerf_point_decode_backward_workspace.argtypes = [ctypes.c_uint32] * 4
        l.ssdnerf_point_decode_backward_layout.restype = None
        l.ssdnerf_point_decode_backward_layout.argtypes = [ctypes.c_uint32] * 4 + [ctypes.POINTER(ctypes.c_uint64)]
        l.ssdnerf_point_decode_backward_params_workspace.restype = ctypes.c_size_t
        l.ssdnerf_point_decode_backward_params_workspace.argtypes = [ctypes.c_uint32] * 3
        l.ssdnerf_point_decode_backward_params.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_uint32] * 3 + [ctypes.c_void_p] * 4 + \
                                                          [ctypes.c_uint32, ctypes.c_float] + [ctypes.c_void_p] * 3 + [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        l.ssdnerf_group_norm_workspace.restype = ctypes.c_size_t
        l.ssdnerf_group_norm_workspace.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        l.ssdnerf_group_norm_backward_workspace.restype = ctypes.c_size_t
        l.ssdnerf_group_norm_backward_workspace.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        l.ssdnerf_image_metrics.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p]
        l.ssdnerf_tv_loss_forward.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p,
                                              ctypes.c_void_p]
        l.ssdnerf_tv_loss_backward.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float,
                                               ctypes.c_void_p, ctypes.c_void_p]
        l.ssdnerf_mesh_vertex_attributes.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                                     ctypes.c_uint32, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.c_float] + [ctypes.c_void_p] * 7
        l.ssdnerf_lpips_input.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        l.ssdnerf_relu_pool_nhwc.argtypes = [ctypes.c_void_p] + [ctypes.c_uint32] * 4 + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        l.ssdnerf_lpips_layer_workspace.restype = ctypes.c_size_t
        l.ssdnerf_lpips_layer_workspace.argtypes = [ctypes.c_uint32]
        l.ssdnerf_lpips_layer.argtypes = [ctypes.c_void_p] + [ctypes.c_uint32] * 4 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                          ctypes.c_void_p]
        l.ssdnerf_feature_moments_accumulate.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        l.ssdnerf_kid_subset_sums_workspace.restype = ctypes.c_size_t
        l.ssdnerf_kid_subset_sums_workspace.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
        l.ssdnerf_kid_subset_sums.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_uint32] * 3 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        l.ssdnerf_adam_max_tensors.restype = ctypes.c_uint32
        l.ssdnerf_adam_max_tensors.argtypes = []
        l.ssdnerf_adam_step_multi.argtypes = [ctypes.POINTER(AdamTensor), ctypes.c_uint32, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
        l.ssdnerf_gather_views_u8.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        l.ssdnerf_sample_rays_u8.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 3 + \
                                            [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 4
        l.ssdnerf_perm_indices.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64,
                                           ctypes.c_uint32, ctypes.c_void_p]
        l.ssdnerf_sample_rays_perm_u8.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 3 + \
                                                 [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32] + \
                                                 [ctypes.c_void_p] * 4
        l.ssdnerf_ema_chunk.restype = ctypes.c_uint32
        l.ssdnerf_ema_chunk.argtypes = []
        l.ssdnerf_ema_plan_build.argtypes = [ctypes.POINTER(EmaRow), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
        l.ssdnerf_ema_update_multi.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float, ctypes.c_float, ctypes.c_void_p]
        l.ssdnerf_cache_max_scenes.restype = ctypes.c_uint32
        l.ssdnerf_cache_max_scenes.argtypes = []
        for fn in (l.ssdnerf_cache_load_multi, l.ssdnerf_cache_store_multi):
            fn.argtypes = [ctypes.POINTER(CacheStore), ctypes.POINTER(CacheRow), ctypes.c_uint32] + [ctypes.c_void_p] * 6
        l.ssdnerf_dpmpp_block_cap.restype = ctypes.c_uint32
        l.ssdnerf_dpmpp_block_cap.argtypes = []
        l.ssdnerf_dpmpp_step_v.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint64] + [ctypes.c_float] * 7 + [ctypes.c_void_p] * 3
        l.ssdnerf_sde_block_cap.restype = ctypes.c_uint32
        l.ssdnerf_sde_block_cap.argtypes = []
        l.ssdnerf_philox_normal_fill.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p]
        l.ssdnerf_sde_step_v.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint64, ctypes.c_int] + [ctypes.c_float] * 8 + \
                                        [ctypes.c_uint64, ctypes.c_uint32] + [ctypes.c_void_p] * 3
        l.ssdnerf_prior_block_cap.restype = l.ssdnerf_prior_blocks_per_sample.restype = ctypes.c_uint32
        l.ssdnerf_prior_block_cap.argtypes = []
        l.ssdnerf_prior_blocks_per_sample.argtypes = [ctypes.c_uint64]
        l.ssdnerf_prior_loss_partials.restype = ctypes.c_uint64
        l.ssdnerf_prior_loss_partials.argtypes = [ctypes.c_uint32, ctypes.c_uint64]
        l.ssdnerf_prior_q_sample.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32] + [ctypes.c_void_p] * 2
        l.ssdnerf_prior_loss_v.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3 + \
                                          [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32] + [ctypes.c_void_p] * 4
        l.ssdnerf_prior_loss_v_backward.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4 + \
                                                   [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32] + [ctypes.c_void_p] * 3
        l.ssdnerf_png_filter_rows.argtypes =[ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_uint32] * 3 + [ctypes.c_void_p] * 2
        l.ssdnerf_code_plane_rgb.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_uint32] * 4 + [ctypes.c_float] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 2
        if l.ssdnerf_abi_version() != ABI_VERSION:
            raise RuntimeError(f"libssdnerf_hip.so ABI {l.ssdnerf_abi_version()} != expected {ABI_VERSION}: rebuild")
        _lib = l
    return _lib


_SYNC_CHECK = os.environ.get("SSDNERF_SYNC_CHECK", "0") == "1"      # debugging aid: synchronise after every library call and name it first


def check(status: int, what: str) -> None:
    if status != 0:
        raise RuntimeError(f"{what} failed ({status}): {lib().ssdnerf_last_error().decode()}")
    if _SYNC_CHECK and not torch.cuda.is_current_stream_capturing():
        import sys
        print(f"[ssdnerf sync-check] {what}", file=sys.stderr, flush=True)
        torch.cuda.synchronize()


def ptr(t: Optional[torch.Tensor]) -> ctypes.c_void_p:
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def u32(v) -> ctypes.c_uint32:
    return ctypes.c_uint32(int(v))


def f32(v) -> ctypes.c_float:
    return ctypes.c_float(float(v))


def dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float16:
        return F16
    raise RuntimeError(f"unsupported dtype {t.dtype} (fp32 / fp16 only)")


def require_cuda(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("ssdnerf_amd operators need tensors on the GPU (cuda:N == HIP device N)")
