"""ctypes binding of libgut_hip.so (C ABI in include/gut_hip.h).

The product path has NO CPU fallback: if the HIP library is missing or fails to load this module
raises, and every Tracer call fails loudly.  (The CPU oracle under oracle/ is test infrastructure and
is never imported from here.)
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GUT_HIP_LIB", os.path.join(HERE, "libgut_hip.so"))  # override: dev experiments only

GUT_ABI_VERSION = 6   # include/gut_hip.h: bumped on every struct / array-length / signature change
GUT_NUM_KERNEL_TIMERS = 11
BWD_RAW_PARAMETER_GRADS = 1
BWD_COMPACT_RADIANCE_GRADS = 2
BWD_SKIP_EPILOGUE = 4
OPT_LAZY_TILE_ORDER = 1
ADAM_CLEAR_CONSUMED_GRADS = 1
GRADIENT_RECORD_FLOATS = 16
OPT_SORTED_REFERENCE_BACKWARD = 2
OPT_EARLY_EXTRA_PERCENT = 3
OPT_FORWARD_TILE_ORDER = 4
OPT_KERNEL_TIMING_SET = 5
OPT_DEBUG_REPLACE_SCRATCH = 100
KERNEL_TIMER_NAMES = ("project", "scan", "expand", "sort", "ranges", "render", "render_bwd", "project_bwd", "optimizer",
                      "optimizer_early", "optimizer_early_2")

SHUTTER_GLOBAL = 4
CAMERA_PINHOLE, CAMERA_FISHEYE = 0, 1

BUF = dict(tiles_count=0, tiles_offset=1, proj_pos=2, conic_opacity=3, extent=4, depth=5, feat=6,
           unsorted_keys=7, unsorted_ids=8, sorted_keys=9, sorted_ids=10, tile_ranges=11, grad_scratch=12,
           tile_traversed_fwd=13, tile_traversed_bwd=14, ordered_ids=15, packed_rows=16)


class GutCamera(C.Structure):
    _fields_ = [
        ("model", C.c_int32), ("shutter", C.c_int32),
        ("principal_point", C.c_float * 2), ("focal_length", C.c_float * 2),
        ("radial_coeffs", C.c_float * 6), ("tangential_coeffs", C.c_float * 2), ("thin_prism_coeffs", C.c_float * 4),
        ("max_angle", C.c_float), ("pose_start", C.c_float * 7), ("pose_end", C.c_float * 7),
        ("timestamp_start_us", C.c_int64), ("timestamp_end_us", C.c_int64),
    ]


class GutConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("enable_kernel_timings", C.c_int32), ("particle_radiance_sph_degree", C.c_int32),
        ("particle_kernel_degree", C.c_int32), ("k_buffer_size", C.c_int32), ("global_z_order", C.c_int32),
        ("n_rolling_shutter_iterations", C.c_int32), ("ut_require_all_sigma_points", C.c_int32),
        ("rect_bounding", C.c_int32), ("tight_opacity_bounding", C.c_int32), ("tile_based_culling", C.c_int32),
        ("enable_hitcounts", C.c_int32),
        ("particle_kernel_min_response", C.c_float), ("particle_kernel_min_alpha", C.c_float),
        ("particle_kernel_max_alpha", C.c_float), ("min_transmittance", C.c_float),
        ("ut_alpha", C.c_float), ("ut_beta", C.c_float), ("ut_kappa", C.c_float), ("ut_in_image_margin_factor", C.c_float),
    ]


class GutStats(C.Structure):
    _fields_ = [
        ("num_particles", C.c_uint64), ("num_visible", C.c_uint64), ("num_intersections", C.c_uint64),
        ("num_tiles", C.c_uint64), ("num_pixels", C.c_uint64), ("traversed_fwd", C.c_uint64),
        ("traversed_bwd", C.c_uint64), ("sort_end_bit", C.c_uint32), ("binning_overflows", C.c_uint32),
        ("side_stream_rows", C.c_uint64), ("side_stream_rows_first_launch", C.c_uint64),
    ]


class GutLazyMoments(C.Structure):
    _fields_ = [("d_wave_step", C.c_void_p), ("d_pow_beta1", C.c_void_p), ("d_pow_beta2", C.c_void_p), ("table_len", C.c_uint32),
                ("d_overrun", C.c_void_p)]


class GutRegularisation(C.Structure):
    """The MCMC regularisers (gut_hip.h): density_coeff = lambda_opacity / N, scale_coeff = lambda_scale / (3 N), d_partials
    [ceil(N / 64), 2] floats for the loss value or None."""
    _fields_ = [("density_coeff", C.c_float), ("scale_coeff", C.c_float), ("d_partials", C.c_void_p)]


class GutPhotometricLoss(C.Structure):
    """The fused loss by descriptor (gut_hip.h, gut_photometric_loss_run): device pointers, None = that operand is absent."""
    _fields_ = [("d_rgba", C.c_void_p), ("d_gt_rgb", C.c_void_p), ("d_mask", C.c_void_p), ("d_background", C.c_void_p),
                ("d_exposure12", C.c_void_p), ("d_workspace", C.c_void_p), ("d_loss3", C.c_void_p), ("d_rgba_grad", C.c_void_p),
                ("d_exposure_grad12", C.c_void_p), ("background", C.c_float), ("lambda_l1", C.c_float), ("lambda_ssim", C.c_float)]


class GutContribution(C.Structure):
    """One Gaussian's contribution record (gut_hip.h, gut_trace_contribution): 16 bytes, accumulated into."""
    _fields_ = [("weight_sum_q32", C.c_uint64), ("max_weight_bits", C.c_uint32), ("pixels", C.c_uint32)]


SURFACE_LEVEL, SURFACE_MAX_WEIGHT = 0, 1   # gut_hip.h, GUT_SURFACE_*

TSDF_MAX_VIEWS = 8   # gut_hip.h, GUT_TSDF_MAX_VIEWS


class GutTsdfGrid(C.Structure):
    """The TSDF volume (gut_hip.h): the box and the caller's state tensors, None = no colours."""
    _fields_ = [("origin", C.c_float * 3), ("voxel", C.c_float), ("dims", C.c_int32 * 3), ("truncation", C.c_float),
                ("d_acc", C.c_void_p), ("d_cnt", C.c_void_p), ("d_rgb_sum", C.c_void_p), ("d_rgb_cnt", C.c_void_p)]


class GutTsdfView(C.Structure):
    """One view of gut_tsdf_integrate: the camera (host), the planes (device; rgba and ray origin may be None)."""
    _fields_ = [("camera", C.POINTER(GutCamera)), ("width", C.c_int32), ("height", C.c_int32), ("d_distance", C.c_void_p),
                ("d_rgba", C.c_void_p), ("d_ray_origin", C.c_void_p)]


kEnvSlots = 128                    # gut_hip.h, GUT_ENVIRONMENT_SLOTS: texels a 16x16 pixel tile of the adjoint sums in LDS
ENVIRONMENT_MAX_RESOLUTION = 8192  # gut_hip.h, GUT_ENVIRONMENT_MAX_RESOLUTION
ENVIRONMENT_TILE = 16


class GutEnvironmentView(C.Structure):
    """One view of the cube-map background (gut_hip.h): the ray table (device), the camera-to-world rotation by value."""
    _fields_ = [("d_ray_direction", C.c_void_p), ("rotation", C.c_float * 9), ("height", C.c_int32), ("width", C.c_int32)]


class GutEnvironmentCotangent(C.Structure):
    """The adjoint's cotangent: the plane [H,W,3], or the fused loss's pair rgba / rgba_grad [H,W,4]; None = that form is absent."""
    _fields_ = [("d_plane_grad", C.c_void_p), ("d_rgba", C.c_void_p), ("d_rgba_grad", C.c_void_p)]


BILATERAL_MAX_DIM = 256   # gut_hip.h, GUT_BILATERAL_MAX_DIM
BILATERAL_TABLE = 1024    # gut_hip.h, GUT_BILATERAL_TABLE: 64-bit sums a 16x16 pixel tile of the adjoint holds in LDS
BILATERAL_TILE = 16


class GutBilateralGrid(C.Structure):
    """One view's bilateral grid (gut_hip.h): d_grid [12, levels, rows, columns] float32 on the device."""
    _fields_ = [("d_grid", C.c_void_p), ("levels", C.c_int32), ("rows", C.c_int32), ("columns", C.c_int32)]


EXPORTS = ("gut_default_config", "gut_create", "gut_destroy", "gut_trace", "gut_trace_bwd", "gut_collect_times",
           "gut_get_stats", "gut_debug_buffer", "gut_debug_copy", "gut_kernel_times", "gut_kernel_times_mean", "gut_last_error", "gut_abi_version",
           "gut_ssim_workspace_bytes", "gut_ssim_forward", "gut_ssim_backward",
           "gut_photometric_workspace_bytes", "gut_photometric_loss", "gut_optimize_after_bwd", "gut_set_option",
           "gut_trace_bwd_ex", "gut_optimize_rows_without_gradient", "gut_compact_gradient_rows", "gut_scatter_gradient_records",
           "gut_sh_adam_step_ex", "gut_mark_walked_waves", "gut_adam_unwalked_waves", "gut_activate_pack", "gut_adam_step", "gut_sh_adam_step", "gut_mcmc_relocation",
           "gut_optimize_finish_without_gradient", "gut_scatter_gradient_records_dev", "gut_adam_unwalked_waves_ex", "gut_sync_moments", "gut_trace_fields", "gut_trace_bwd_fields", "gut_selective_adam",
           "gut_trace_model_fields", "gut_trace_bwd_model_fields", "gut_position_gradient_statistics",
           "gut_set_position_gradient_statistics", "gut_mcmc_perturb", "gut_trace_raw_model_fields", "gut_set_regularisation",
           "gut_sh_adam_step_regularised", "gut_adam_unwalked_waves_regularised", "gut_sync_moments_ex", "gut_regularisation_gradient",
           "gut_regularisation_loss", "gut_image_metrics_workspace_bytes", "gut_image_metrics", "gut_photometric_loss_masked",
           "gut_photometric_loss_background", "gut_set_pose_gradient", "gut_pose_adam_step",
           "gut_photometric_exposure_workspace_bytes", "gut_photometric_loss_exposure", "gut_exposure_adam_step",
           "gut_image_metrics_cc_workspace_bytes", "gut_image_metrics_cc", "gut_photometric_loss_run", "gut_trace_bwd_pose",
           "gut_trace_contribution", "gut_trace_contribution_weighted", "gut_pixel_error", "gut_trace_attributes",
           "gut_trace_attributes_bwd", "gut_trace_surface", "gut_tsdf_integrate", "gut_surface_nets_count", "gut_surface_nets_emit",
           "gut_environment_sample", "gut_environment_workspace_bytes", "gut_environment_backward", "gut_environment_rotation",
           "gut_bilateral_workspace_bytes", "gut_bilateral_slice", "gut_bilateral_backward", "gut_bilateral_backward_image",
           "gut_bilateral_adam_step")

_lib = None


def load():
    """Load libgut_hip.so (raises RuntimeError with build instructions if it is absent)."""
    global _lib
    if _lib is not None:
        return _lib
    # (GUT_HIP_LIBRARY: a developer's diagnostic build of the same sources, e.g. tools/clock_probe.py's stamped library)
    path = os.environ.get("GUT_HIP_LIBRARY") or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the 3DGUT HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (needs hipcc). There is no CPU fallback in the product path.")
    lib = C.CDLL(path)
    vp, u32, i32, f_p = C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p
    lib.gut_last_error.restype = C.c_char_p
    lib.gut_abi_version.restype = C.c_int
    lib.gut_default_config.argtypes = [C.POINTER(GutConfig)]
    lib.gut_default_config.restype = None
    lib.gut_create.argtypes = [C.POINTER(GutConfig), C.c_int, C.POINTER(vp)]
    lib.gut_destroy.argtypes = [vp]
    lib.gut_destroy.restype = None
    lib.gut_trace.argtypes = [vp, vp, u32, i32, u32, f_p, f_p, i32, i32, f_p, f_p, C.POINTER(GutCamera), f_p, f_p, f_p, f_p]
    lib.gut_trace_bwd.argtypes = [vp, vp, u32, i32, u32, f_p, f_p, i32, i32, f_p, f_p, C.POINTER(GutCamera),
                                  f_p, f_p, f_p, f_p, f_p, f_p]
    lib.gut_trace_fields.argtypes = [vp, vp, u32, i32, u32, f_p, f_p, f_p, f_p, f_p, i32, i32, f_p, f_p, C.POINTER(GutCamera), f_p, f_p, f_p, f_p]
    lib.gut_trace_bwd_fields.argtypes = [vp, vp, u32, i32, u32, f_p, i32, i32, f_p, f_p, C.POINTER(GutCamera), f_p, f_p, f_p, f_p,
                                         f_p, f_p, f_p, f_p, f_p]
    lib.gut_trace_model_fields.argtypes = [vp, vp, u32, i32, u32, f_p, f_p, f_p, f_p, f_p, f_p, i32, i32, f_p, f_p, C.POINTER(GutCamera),
                                           f_p, f_p, f_p, f_p]
    lib.gut_trace_raw_model_fields.argtypes = lib.gut_trace_model_fields.argtypes
    lib.gut_trace_bwd_model_fields.argtypes = [vp, vp, u32, i32, u32, i32, i32, f_p, f_p, C.POINTER(GutCamera), f_p, f_p, f_p, f_p,
                                               f_p, f_p, f_p, f_p, f_p, f_p]
    lib.gut_position_gradient_statistics.argtypes = [vp, u32, f_p, u32, f_p, u32, f_p, f_p, vp]
    lib.gut_set_position_gradient_statistics.argtypes = [vp, f_p, vp]
    lib.gut_set_pose_gradient.argtypes = [vp, f_p]
    lib.gut_pose_adam_step.argtypes = [vp, f_p, f_p, f_p, vp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, f_p]
    lib.gut_trace_bwd_pose.argtypes = [vp, vp, u32, i32, u32, f_p, i32, i32, f_p, f_p, C.POINTER(GutCamera), f_p, f_p, f_p, f_p]
    lib.gut_trace_contribution.argtypes = [vp, vp, u32, i32, u32, f_p, i32, i32, f_p, f_p, C.POINTER(GutCamera), vp]
    lib.gut_trace_contribution_weighted.argtypes = [vp, vp, u32, i32, u32, f_p, i32, i32, f_p, f_p, C.POINTER(GutCamera), f_p, vp, vp]
    lib.gut_trace_attributes.argtypes = [vp, vp, u32, i32, u32, f_p, i32, i32, f_p, f_p, C.POINTER(GutCamera), i32, f_p, f_p]
    lib.gut_trace_attributes_bwd.argtypes = lib.gut_trace_attributes.argtypes
    lib.gut_trace_surface.argtypes = [vp, vp, u32, i32, u32, f_p, i32, i32, f_p, f_p, C.POINTER(GutCamera), i32, C.c_float, f_p, vp, f_p]
    lib.gut_tsdf_integrate.argtypes = [vp, C.POINTER(GutTsdfGrid), i32, C.POINTER(GutTsdfView)]
    lib.gut_surface_nets_count.argtypes = [vp, C.POINTER(GutTsdfGrid), u32, vp, vp]
    lib.gut_surface_nets_emit.argtypes = [vp, C.POINTER(GutTsdfGrid), u32, vp, vp, vp, vp, vp, vp, vp]
    env_p = C.POINTER(GutEnvironmentView)
    lib.gut_environment_sample.argtypes = [vp, env_p, vp, i32, vp]
    lib.gut_environment_workspace_bytes.argtypes = [i32]
    lib.gut_environment_workspace_bytes.restype = C.c_size_t
    lib.gut_environment_backward.argtypes = [vp, env_p, C.POINTER(GutEnvironmentCotangent), i32, vp, vp]
    lib.gut_environment_rotation.argtypes = [C.POINTER(GutCamera), C.POINTER(C.c_float)]
    bil_p = C.POINTER(GutBilateralGrid)
    lib.gut_bilateral_workspace_bytes.argtypes = [i32, i32, i32]
    lib.gut_bilateral_workspace_bytes.restype = C.c_size_t
    lib.gut_bilateral_slice.argtypes = [vp, i32, i32, vp, vp, C.c_float, bil_p, vp]
    lib.gut_bilateral_backward.argtypes = [vp, i32, i32, vp, vp, C.c_float, bil_p, vp, C.c_float, vp, vp, vp]
    lib.gut_bilateral_backward_image.argtypes = [vp, i32, i32, vp, vp, C.c_float, bil_p, vp, vp]
    lib.gut_bilateral_adam_step.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float]
    lib.gut_pixel_error.argtypes = [vp, i32, i32, vp, vp, vp, vp, C.c_float, vp, vp]
    lib.gut_mcmc_perturb.argtypes = [vp, u32, f_p, f_p, C.c_float, C.c_uint64, C.c_uint64, f_p]
    lib.gut_collect_times.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.gut_get_stats.argtypes = [vp, C.POINTER(GutStats)]
    lib.gut_debug_buffer.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(C.c_size_t)]
    lib.gut_debug_copy.argtypes = [vp, i32, vp, C.c_size_t]
    lib.gut_kernel_times.argtypes = [vp, C.POINTER(C.c_float)]
    lib.gut_kernel_times_mean.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
    i64 = C.c_int64
    lib.gut_ssim_workspace_bytes.argtypes = [i32, i32, i32]
    lib.gut_ssim_workspace_bytes.restype = C.c_size_t
    lib.gut_ssim_forward.argtypes = [vp, i32, i32, i32, i64, i64, i64, vp, vp, vp, vp]
    lib.gut_ssim_backward.argtypes = [vp, i32, i32, i32, i64, i64, i64, vp, vp, vp, vp, vp]
    lib.gut_photometric_workspace_bytes.argtypes = [i32, i32]
    lib.gut_photometric_workspace_bytes.restype = C.c_size_t
    lib.gut_photometric_loss.argtypes = [vp, i32, i32, vp, vp, C.c_float, C.c_float, C.c_float, vp, vp, vp]
    lib.gut_photometric_loss_masked.argtypes = [vp, i32, i32, vp, vp, vp, C.c_float, C.c_float, C.c_float, vp, vp, vp]
    lib.gut_photometric_loss_background.argtypes = [vp, i32, i32, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp, vp]
    lib.gut_photometric_exposure_workspace_bytes.argtypes = [i32, i32]
    lib.gut_photometric_exposure_workspace_bytes.restype = C.c_size_t
    lib.gut_photometric_loss_exposure.argtypes = [vp, i32, i32, vp, vp, vp, vp, C.c_float, vp, C.c_float, C.c_float, vp, vp, vp, vp]
    lib.gut_photometric_loss_run.argtypes = [vp, i32, i32, C.POINTER(GutPhotometricLoss)]
    lib.gut_exposure_adam_step.argtypes = [vp, vp, vp, vp, vp, vp, C.c_float, C.c_float, C.c_float, C.c_float]
    lib.gut_image_metrics_workspace_bytes.argtypes = [i32, i32]
    lib.gut_image_metrics_workspace_bytes.restype = C.c_size_t
    lib.gut_image_metrics.argtypes = [vp, i32, i32, vp, vp, C.c_float, vp, vp]
    lib.gut_image_metrics_cc_workspace_bytes.argtypes = [i32, i32]
    lib.gut_image_metrics_cc_workspace_bytes.restype = C.c_size_t
    lib.gut_image_metrics_cc.argtypes = [vp, i32, i32, vp, vp, C.c_float, C.c_float, vp, vp, vp]
    lib.gut_image_metrics_cc.restype = C.c_int
    lib.gut_trace_bwd_ex.argtypes = [vp, vp, u32, i32, u32, f_p, f_p, i32, i32, f_p, f_p, C.POINTER(GutCamera),
                                     f_p, f_p, f_p, f_p, f_p, f_p, u32]
    lib.gut_activate_pack.argtypes = [vp, u32, vp, vp]
    lib.gut_adam_step.argtypes = [vp, C.c_uint64, u32, vp, vp, vp, vp, C.POINTER(C.c_float), C.c_float, C.c_float,
                                  C.c_float, u32, vp]
    fptr = C.POINTER(C.c_float)
    lazy_p = C.POINTER(GutLazyMoments)
    lib.gut_optimize_after_bwd.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, fptr, fptr, C.c_float, C.c_float, C.c_float, u32,
                                           vp, vp, lazy_p]
    lib.gut_optimize_rows_without_gradient.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, fptr, fptr, C.c_float, C.c_float, C.c_float,
                                                       u32, vp, lazy_p]
    lib.gut_sync_moments.argtypes = [vp, u32, vp, vp, vp, vp, lazy_p, u32]
    lib.gut_optimize_finish_without_gradient.argtypes = [vp, vp]
    lib.gut_selective_adam.argtypes = [vp, C.c_uint64, u32, vp, vp, vp, vp, vp, C.c_float, C.c_float, C.c_float, C.c_float]
    lib.gut_set_option.argtypes = [vp, i32, i32]
    lib.gut_mcmc_relocation.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp, vp]
    lib.gut_sh_adam_step.argtypes = [vp, u32, i32, u32, vp, vp, vp, C.c_float, vp, vp, vp, vp, vp, vp, fptr, fptr,
                                     C.c_float, C.c_float, C.c_float, u32, vp, vp, u32]
    lib.gut_sh_adam_step_ex.argtypes = lib.gut_sh_adam_step.argtypes + [u32, vp, lazy_p]
    lib.gut_mark_walked_waves.argtypes = [vp, vp, vp]
    lib.gut_adam_unwalked_waves.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, fptr, fptr, C.c_float, C.c_float, C.c_float, u32, vp]
    lib.gut_adam_unwalked_waves_ex.argtypes = lib.gut_adam_unwalked_waves.argtypes + [lazy_p]
    reg_p = C.POINTER(GutRegularisation)
    lib.gut_set_regularisation.argtypes = [vp, reg_p]
    lib.gut_sh_adam_step_regularised.argtypes = lib.gut_sh_adam_step_ex.argtypes + [reg_p]
    lib.gut_adam_unwalked_waves_regularised.argtypes = lib.gut_adam_unwalked_waves_ex.argtypes + [reg_p]
    lib.gut_sync_moments_ex.argtypes = lib.gut_sync_moments.argtypes + [reg_p]
    lib.gut_regularisation_gradient.argtypes = [vp, u32, vp, vp, reg_p]
    lib.gut_regularisation_loss.argtypes = [vp, u32, vp, C.c_float, C.c_float, vp, vp, vp]
    lib.gut_compact_gradient_rows.argtypes = [vp, vp, vp, vp, u32, vp]
    lib.gut_scatter_gradient_records.argtypes = [vp, vp, u32, u32, vp, vp]
    lib.gut_scatter_gradient_records_dev.argtypes = [vp, vp, vp, u32, u32, vp, vp]
    if lib.gut_abi_version() != GUT_ABI_VERSION:
        raise RuntimeError("libgut_hip.so ABI version mismatch; rebuild")
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().gut_last_error()
        raise RuntimeError(f"[3dgut] {what}: {msg.decode() if msg else 'unknown error'}")
