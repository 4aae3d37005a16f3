/*
 * gut_hip.h — C ABI of libgut_hip.so, the MI355X-native replacement of the reference's pybind
 * module `lib3dgut_cc` (threedgut_tracer/bindings.cpp:79-113, include/3dgut/splatRaster.h:47-89).
 *
 * Conventions
 *   - every pointer named d_* is a DEVICE pointer owned by the caller (torch tensors in the Python
 *     shim); the library never retains them past the call.  Scratch (per-Gaussian projection
 *     buffers, tile keys, sort temporaries) is owned by the handle and is grow-only.
 *   - `stream` is a hipStream_t passed as void*; all work of a call is enqueued on it.  The reference blocks in the middle
 *     of its forward on a 4-byte device->host read-back of the intersection count (src/gutRenderer.cu:313-321); here only
 *     the FIRST trace() on a handle does: afterwards the binning buffers are sized from the previous frames' counts, the
 *     whole forward is queued, and the host reads the count back behind it (a frame that needed more is binned and
 *     composited a second time; GutStats.binning_overflows counts those).
 *   - return value 0 = success; anything else is an error and gut_last_error() describes it
 *     (the reference logs and drops its Status codes, splatRaster.cpp:225-237; pybind turns C++
 *     exceptions into RuntimeError — the Python shim raises RuntimeError on non-zero).
 *   - one handle <-> one in-flight view: trace_bwd() must follow the trace() it differentiates, on
 *     the same stream (gutRenderer.cu:413-417).  A handle may be used from different host threads
 *     (autograd worker) but not concurrently.
 */
#ifndef GUT_HIP_H
#define GUT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped on every change of a struct layout, an array length or an entry point's signature (2: GutStats grew to 80 bytes and
 * GUT_NUM_KERNEL_TIMERS to 11 in round 2; 3: GutLazyMoments in the gut_optimize_* / gut_sh_adam_step_ex signatures, gut_sync_moments,
 * gut_optimize_finish_without_gradient, gut_scatter_gradient_records_dev, gut_trace_fields / gut_trace_bwd_fields;
 * 4: gut_trace_model_fields / gut_trace_bwd_model_fields, gut_position_gradient_statistics, gut_set_position_gradient_statistics,
 * gut_mcmc_perturb; 5: behaviour, not layout — GUT_OPT_SORTED_REFERENCE_BACKWARD defaults to 1, the reference's own form of the
 * sorted variant's backward; the UT sigma-point spread is rounded from double like the reference's build script does;
 * GutLazyMoments.d_overrun; gut_trace_raw_model_fields; GUT_OPT_FORWARD_TILE_ORDER).  Added under 5 without a bump, nothing that was
 * accepted changed meaning: gut_create takes every value of GutConfig the reference has a kernel for (kernel degree, SH storage degree,
 * rolling-shutter iterations, hit counts), gut_optimize_after_bwd takes a NULL camera position, GUT_OPT_KERNEL_TIMING_SET, and the
 * unsorted backward clamps alpha with the reference's literal 0.99 whatever particle_kernel_max_alpha is; 6: GutRegularisation,
 * gut_set_regularisation, gut_sh_adam_step_regularised, gut_adam_unwalked_waves_regularised, gut_sync_moments_ex,
 * gut_regularisation_gradient, gut_regularisation_loss.  Added under 6 without a bump, nothing that was accepted changed meaning:
 * gut_photometric_loss_masked and gut_photometric_loss_background, new entry points next to gut_photometric_loss, which is
 * untouched; gut_set_pose_gradient and gut_pose_adam_step, new entry points: while it is not set, every gut_trace_bwd* queues what it queued before;
 * gut_trace_bwd_pose, a new entry point: the backward for the pose gradient alone, every other backward launches what it launched;
 * gut_photometric_exposure_workspace_bytes, gut_photometric_loss_exposure and gut_exposure_adam_step, new entry points next to the
 * other forms of the fused loss, which launch what they launched before; gut_image_metrics_cc_workspace_bytes and gut_image_metrics_cc,
 * new entry points next to gut_image_metrics, which launches what it launched before; GutPhotometricLoss and gut_photometric_loss_run,
 * the descriptor form of the fused loss: the four positional forms keep their signatures and call it; GutContribution and
 * gut_trace_contribution, a new entry point: every other call queues what it queued before; gut_trace_contribution_weighted and
 * gut_pixel_error, new entry points: gut_trace_contribution and every other call queue what they queued before; added under 6
 * without a bump: gut_trace_attributes, a new entry point: every other call queues what it queued before; gut_trace_attributes_bwd,
 * likewise; gut_trace_surface, likewise; gut_tsdf_integrate, gut_surface_nets_count and gut_surface_nets_emit, handle-free new entry
 * points; gut_bilateral_workspace_bytes, gut_bilateral_slice, gut_bilateral_backward, gut_bilateral_backward_image and gut_bilateral_adam_step with
 * GutBilateralGrid, handle-free new entry points: every other call, gut_exposure_adam_step included, queues what it queued before). */
#define GUT_ABI_VERSION 6

typedef struct gut_context* gut_handle;

/* sensors/cameraModels.h:34-47 */
enum { GUT_SHUTTER_ROLLING_TOP_TO_BOTTOM = 0, GUT_SHUTTER_ROLLING_LEFT_TO_RIGHT = 1,
       GUT_SHUTTER_ROLLING_BOTTOM_TO_TOP = 2, GUT_SHUTTER_ROLLING_RIGHT_TO_LEFT = 3, GUT_SHUTTER_GLOBAL = 4 };
enum { GUT_CAMERA_OPENCV_PINHOLE = 0, GUT_CAMERA_OPENCV_FISHEYE = 1 };

/* Replaces threedgut::CameraModelParameters + TSensorState (sensors/cameraModels.h:22-58,
 * sensors/sensors.h:33-42) as built by fromOpenCV{Pinhole,Fisheye}CameraModelParameters
 * (bindings.cpp:34-77) and toSensorState (splatRaster.cpp:92-100). */
typedef struct GutCamera {
    int32_t model;              /* GUT_CAMERA_* */
    int32_t shutter;            /* GUT_SHUTTER_* */
    float principal_point[2];
    float focal_length[2];
    float radial_coeffs[6];     /* pinhole: k1..k6 ; fisheye: k1..k4 in [0..3] */
    float tangential_coeffs[2]; /* pinhole only */
    float thin_prism_coeffs[4]; /* pinhole only */
    float max_angle;            /* fisheye only */
    float pose_start[7];        /* world->sensor translation (3) + quaternion (x,y,z,w) */
    float pose_end[7];
    int64_t timestamp_start_us;
    int64_t timestamp_end_us;
} GutCamera;

/* The reference bakes conf.render.* into the kernels as -D defines (setup_3dgut.py:47-70) and its
 * SplatRaster constructor reads only render.enable_kernel_timings (splatRaster.cpp:158-159).  Here
 * the same settings arrive as a struct and reach the kernels as run-time values: every key of
 * render/3dgut.yaml may differ from its default (ut_require_all_sigma_points = true is rejected, as the
 * reference's static_assert does).  Values the reference has no kernel for are rejected by gut_create
 * with a clear message.  The fused optimiser entry points and the model-field traces exist for
 * particle_radiance_sph_degree = 3 only. */
typedef struct GutConfig {
    int32_t abi_version;                  /* GUT_ABI_VERSION */
    int32_t enable_kernel_timings;        /* render.enable_kernel_timings */
    int32_t particle_radiance_sph_degree; /* 3 -> 16 coefficients (default); 0..2: radiance rows and their gradient are [N, 3 (d+1)^2] */
    int32_t particle_kernel_degree;       /* 2 (quadratic, default); 0, 1, 3, 4, 5, 8: the reference's other generalised Gaussians */
    int32_t k_buffer_size;                /* 0 (unsorted) */
    int32_t global_z_order;               /* 1 */
    int32_t n_rolling_shutter_iterations; /* 5 by default; 0..64 */
    int32_t ut_require_all_sigma_points;  /* 0 */
    int32_t rect_bounding, tight_opacity_bounding, tile_based_culling; /* 1,1,1 */
    int32_t enable_hitcounts;             /* 1; 0: the hit-count output is all zeros, as in the reference */
    float particle_kernel_min_response;   /* 0.0113 */
    float particle_kernel_min_alpha;      /* 1/255 */
    float particle_kernel_max_alpha;      /* 0.99 */
    float min_transmittance;              /* 1e-4 */
    float ut_alpha, ut_beta, ut_kappa;    /* 1, 2, 0 */
    float ut_in_image_margin_factor;      /* 0.1 */
} GutConfig;

/* scene/traversal statistics of the most recent trace()/trace_bwd() pair: the quantities the
 * algorithmic-bytes model of SURVEY.md §8d is written in. */
typedef struct GutStats {
    uint64_t num_particles;      /* N */
    uint64_t num_visible;        /* V : Gaussians with tilesCount > 0 */
    uint64_t num_intersections;  /* M */
    uint64_t num_tiles;          /* T */
    uint64_t num_pixels;         /* P */
    uint64_t traversed_fwd;      /* E_f : sum over tiles of list entries fetched before the tile terminated */
    uint64_t traversed_bwd;      /* E_b */
    uint32_t sort_end_bit;       /* 32 + bit_width(T) */
    uint32_t binning_overflows;  /* forwards of this handle whose binning was redone because the frame had more intersections than
                                    the capacity assumed from earlier frames (the forward is queued before the count is known) */
    uint64_t side_stream_rows;   /* Gaussians whose optimiser step the last gut_optimize_rows_without_gradient took (both of its
                                    launches, whole 64-row waves); 0 when the last step did not use it */
    uint64_t side_stream_rows_first_launch; /* ... of which in its first launch (under the forward compositor) */
} GutStats;

/* intermediate buffers exposed to the parity tests (device pointers into handle scratch, valid until
 * the next trace() on the handle) */
enum {
    GUT_BUF_TILES_COUNT = 0,   /* u32 [N]        gutRenderer.cu:166 */
    GUT_BUF_TILES_OFFSET = 1,  /* u32 [N]        inclusive scan */
    GUT_BUF_PROJ_POSITION = 2, /* f32 [N,2] */
    GUT_BUF_CONIC_OPACITY = 3, /* f32 [N,4] */
    GUT_BUF_PROJ_EXTENT = 4,   /* f32 [N,2] */
    GUT_BUF_GLOBAL_DEPTH = 5,  /* f32 [N] */
    GUT_BUF_FEATURES = 6,      /* f32 [N,3] precomputed view-dependent RGB (unclamped) */
    GUT_BUF_UNSORTED_KEYS = 7, /* u64 [M] */
    GUT_BUF_UNSORTED_IDS = 8,  /* u32 [M] */
    GUT_BUF_SORTED_KEYS = 9,   /* u64 [M]  (SORTED_*: the reference's fully sorted lists; built on request, see ORDERED_IDS) */
    GUT_BUF_SORTED_IDS = 10,   /* u32 [M] */
    GUT_BUF_TILE_RANGES = 11,  /* u32 [T,2] */
    GUT_BUF_GRAD_SCRATCH = 12, /* f32 [N,16] per-Gaussian gradient rows of the last trace_bwd (also while the library holds them to be all zero) */
    GUT_BUF_TILE_TRAVERSED_FWD = 13, /* u32 [T] list entries each tile walked before all its rays terminated */
    GUT_BUF_TILE_TRAVERSED_BWD = 14, /* u32 [T] same, last trace_bwd */
    GUT_BUF_ORDERED_IDS = 15,  /* u32 [M] what the compositors actually walked: per tile, the ids in final order for the chunks the
                                  forward staged (0xFFFFFFFF beyond); equals SORTED_IDS on those positions */
    GUT_BUF_PACKED_ROWS = 16   /* f32 [N,12] the rows the last gut_trace_fields / _model_fields / _raw_model_fields forward packed (and, for
                                  the raw entry point, activated: |quat| in the pad column) — what the kernels actually read */
};

/* fills *cfg with the reference defaults (configs/render/3dgut.yaml + 3dgrt.yaml) */
void gut_default_config(GutConfig* cfg);

/* SplatRaster(json) — splatRaster.cpp:153-169 */
int gut_create(const GutConfig* cfg, int device_index, gut_handle* out);
/* ~SplatRaster */
void gut_destroy(gut_handle h);

/* SplatRaster::trace — splatRaster.cpp:174-245.
 *   d_particle_density  f32 [N,12]  (pos3, density, quat wxyz, scale3, pad)   tracer.py:176-178
 *   d_particle_radiance f32 [N,48]  (16 SH coefficients x RGB; [N, 3 (d+1)^2] on a handle with particle_radiance_sph_degree = d < 3)
 *   d_ray_origin/d_ray_direction f32 [H,W,3] camera-space rays
 * outputs (fully written by the call, no pre-initialisation needed):
 *   d_ray_radiance_density f32 [H,W,4], d_ray_hit_distance f32 [H,W,1] (1e6 for rays that miss the
 *   scene AABB), d_ray_hit_count f32 [H,W,1], d_particle_visibility f32 [N,1] (1.0/0.0)          */
int gut_trace(gut_handle h, void* stream, uint32_t frame_number, int32_t num_active_features /* SH degree 0..3 */,
              uint32_t num_particles, const float* d_particle_density, const float* d_particle_radiance,
              int32_t width, int32_t height, const float* d_ray_origin, const float* d_ray_direction,
              const GutCamera* camera,
              float* d_ray_radiance_density, float* d_ray_hit_distance, float* d_ray_hit_count,
              float* d_particle_visibility);

/* SplatRaster::traceBwd — splatRaster.cpp:247-332.  d_ray_hit_distance_grad may be NULL (treated as zeros; selects
 * the kernel variant without hit-distance gradient terms).  Gradient outputs are fully overwritten:
 *   d_particle_density_grad f32 [N,12], d_particle_radiance_grad f32 [N,48]                       */
int gut_trace_bwd(gut_handle h, void* stream, uint32_t frame_number, int32_t num_active_features,
                  uint32_t num_particles, const float* d_particle_density, const float* d_particle_radiance,
                  int32_t width, int32_t height, const float* d_ray_origin, const float* d_ray_direction,
                  const GutCamera* camera,
                  const float* d_ray_radiance_density, const float* d_ray_radiance_density_grad,
                  const float* d_ray_hit_distance, const float* d_ray_hit_distance_grad,
                  float* d_particle_density_grad, float* d_particle_radiance_grad);

/* Same as gut_trace_bwd with option flags.  GUT_BWD_RAW_PARAMETER_GRADS: d_particle_density must be rows produced by
 * gut_activate_pack (|quat| in the pad column); the [N,12] output is then the gradient w.r.t. the RAW parameters
 * (density logit, un-normalised quaternion, log-scale), i.e. chained through sigmoid / normalise / exp
 * (threedgrut/model/model.py:74-93), ready for gut_adam_step. */
#define GUT_BWD_RAW_PARAMETER_GRADS 1u
/* GUT_BWD_COMPACT_RADIANCE_GRADS (implies raw parameter gradients): d_particle_radiance_grad receives only [N,3] =
 * dL/dRGB masked by (precomputed RGB > 0) instead of the [N,48] SH gradient; the SH gradient of the view is
 * Y_k(dir) (x) that row and is rebuilt by gut_sh_adam_step (also across several views: compact data-parallel exchange). */
#define GUT_BWD_COMPACT_RADIANCE_GRADS 2u
/* GUT_BWD_SKIP_EPILOGUE: stop after the compositing backward; the per-Gaussian gradient rows stay in the handle and the two
 * output pointers may be NULL.  Follow with gut_optimize_after_bwd on the same stream (single-view training step: the
 * epilogue, the SH-gradient rebuild and Adam then run as ONE pass over the Gaussians). */
#define GUT_BWD_SKIP_EPILOGUE 4u
int gut_trace_bwd_ex(gut_handle h, void* stream, uint32_t frame_number, int32_t num_active_features,
                     uint32_t num_particles, const float* d_particle_density, const float* d_particle_radiance,
                     int32_t width, int32_t height, const float* d_ray_origin, const float* d_ray_direction,
                     const GutCamera* camera,
                     const float* d_ray_radiance_density, const float* d_ray_radiance_density_grad,
                     const float* d_ray_hit_distance, const float* d_ray_hit_distance_grad,
                     float* d_particle_density_grad, float* d_particle_radiance_grad, uint32_t flags);

/* gut_trace / gut_trace_bwd with the particle parameters as the FOUR activated tensors the reference's Tracer.render hands to
 * _Autograd.apply (positions [N,3], density [N,1], rotation [N,4] wxyz, scale [N,3]; threedgut_tracer/tracer.py:317-327) instead
 * of the [N,12] concatenation _Autograd.forward builds with torch.cat (:176-178), and with the density gradient returned as the
 * four tensors _Autograd.backward hands back (:268-286) instead of one [N,12] tensor it splits and copies.  The rows are packed
 * into handle scratch by one coalesced kernel and kept for the backward; results are those of gut_trace / gut_trace_bwd on the
 * concatenated rows, bit for bit.  d_rotation / d_rotation_grad must be 16-byte aligned (torch allocations are). */
int gut_trace_fields(gut_handle h, void* stream, uint32_t frame_number, int32_t num_active_features, uint32_t num_particles,
                     const float* d_positions, const float* d_density, const float* d_rotation, const float* d_scale,
                     const float* d_particle_radiance, int32_t width, int32_t height, const float* d_ray_origin,
                     const float* d_ray_direction, const GutCamera* camera, float* d_ray_radiance_density,
                     float* d_ray_hit_distance, float* d_ray_hit_count, float* d_particle_visibility);
int gut_trace_bwd_fields(gut_handle h, void* stream, uint32_t frame_number, int32_t num_active_features, uint32_t num_particles,
                         const float* d_particle_radiance, int32_t width, int32_t height, const float* d_ray_origin,
                         const float* d_ray_direction, const GutCamera* camera, const float* d_ray_radiance_density,
                         const float* d_ray_radiance_density_grad, const float* d_ray_hit_distance,
                         const float* d_ray_hit_distance_grad, float* d_positions_grad, float* d_density_grad, float* d_rotation_grad,
                         float* d_scale_grad, float* d_particle_radiance_grad);

/* gut_trace_fields / gut_trace_bwd_fields with the SH coefficients handed over as the model's TWO feature tensors as well
 * (features_albedo [N,3] = the degree-0 triple, features_specular [N,45]; threedgrut/model/model.py:68-75), instead of the [N,48]
 * tensor `get_features()` builds with torch.cat for every render (threedgut_tracer/tracer.py:322) — a 2.3 GB copy at 6 M
 * Gaussians, plus the split and two copies autograd makes of its gradient.  The projection reads each wave's [64,45] block
 * directly (rows of culled Gaussians are not fetched); the backward writes the two gradient tensors in full (zeros for Gaussians
 * without tiles), coalesced.  Results are those of gut_trace_fields on the concatenation, bit for bit.  d_rotation,
 * d_features_specular and their gradients must be 16-byte aligned.  The backward follows a gut_trace_model_fields (or
 * gut_trace_fields) forward on the same handle and stream. */
int gut_trace_model_fields(gut_handle h, void* stream, uint32_t frame_number, int32_t num_active_features, uint32_t num_particles,
                           const float* d_positions, const float* d_density, const float* d_rotation, const float* d_scale,
                           const float* d_features_albedo, const float* d_features_specular, int32_t width, int32_t height,
                           const float* d_ray_origin, const float* d_ray_direction, const GutCamera* camera,
                           float* d_ray_radiance_density, float* d_ray_hit_distance, float* d_ray_hit_count,
                           float* d_particle_visibility);
/* gut_trace_model_fields on the model's PRE-ACTIVATION tensors — what MixtureOfGaussians keeps as nn.Parameters (density logit,
 * un-normalised quaternion, log-scale; threedgrut/model/model.py:74-93 with configs/base_gs.yaml:54-55: sigmoid / exp, rotation
 * always normalize): the three activations and the row packing run as one kernel, and the gut_trace_bwd_model_fields that follows
 * on this handle returns the gradients w.r.t. those raw tensors (chained through sigmoid' / normalize' / exp').  For a trainer that
 * keeps the reference's model and optimiser this removes the model's activation kernels, their backward kernels and the
 * AccumulateGrad copies from every step (6.2 -> 5.2 ms per step on the 6 M stand-in).  The caller (3dgrut_amd/tracer.py: Tracer.render)
 * uses it only for a model whose three activation callables ARE torch.sigmoid / torch.nn.functional.normalize / torch.exp. */
int gut_trace_raw_model_fields(gut_handle h, void* stream, uint32_t frame_number, int32_t num_active_features, uint32_t num_particles,
                               const float* d_positions, const float* d_density_logit, const float* d_rotation_raw, const float* d_log_scale,
                               const float* d_features_albedo, const float* d_features_specular, int32_t width, int32_t height,
                               const float* d_ray_origin, const float* d_ray_direction, const GutCamera* camera,
                               float* d_ray_radiance_density, float* d_ray_hit_distance, float* d_ray_hit_count,
                               float* d_particle_visibility);
int gut_trace_bwd_model_fields(gut_handle h, void* stream, uint32_t frame_number, int32_t num_active_features, uint32_t num_particles,
                               int32_t width, int32_t height, const float* d_ray_origin, const float* d_ray_direction,
                               const GutCamera* camera, const float* d_ray_radiance_density, const float* d_ray_radiance_density_grad,
                               const float* d_ray_hit_distance, const float* d_ray_hit_distance_grad, float* d_positions_grad,
                               float* d_density_grad, float* d_rotation_grad, float* d_scale_grad, float* d_features_albedo_grad,
                               float* d_features_specular_grad);

/* SplatRaster::collectTimes — splatRaster.cpp:334-364: mean ms per tag over the timers recorded
 * since the last call; -1 for a tag with no samples. */
int gut_collect_times(gut_handle h, float* forward_render_ms, float* backward_render_ms);

/* statistics + debug views (parity tests, roofline accounting).  gut_get_stats synchronises the
 * stream of the last call. */
int gut_get_stats(gut_handle h, GutStats* out);
int gut_debug_buffer(gut_handle h, int32_t which, void** d_ptr, size_t* bytes);
/* copies a debug buffer into caller-owned DEVICE memory of at least `bytes` bytes (stream-ordered, then synchronised) */
int gut_debug_copy(gut_handle h, int32_t which, void* d_dst, size_t bytes);

/* Runtime options of a handle (take effect at the next gut_trace).
 * GUT_OPT_LAZY_TILE_ORDER (default 1; unsorted variant only): group the (tile | depth) keys by tile only (2 of the 5 radix
 * passes) and let the forward compositor put each tile's entries in depth order 512 at a time, as far as the tile is
 * actually walked (whole-tile termination leaves most of every list untouched: 86 % on the bench frame).  Images, traversal
 * depths and gradients are identical to the fully sorted path; GUT_BUF_ORDERED_IDS shows what was walked, GUT_BUF_SORTED_*
 * still return the reference's full lists (built on request).  0 restores the full radix sort. */
#define GUT_OPT_LAZY_TILE_ORDER 1
/* GUT_OPT_SORTED_REFERENCE_BACKWARD (default 1 since ABI 5; sorted variant k_buffer_size > 0 only): compute the colour term of
 * d(alpha) in the backward exactly as the reference does — un-doing the back-to-front colour recurrence from the final colour
 * with the UNclamped precomputed colour (gutKBufferRenderer.cuh:127-131, shRadiativeParticles.slang:179-207) although the
 * forward composited max(colour, 0) (:159-161).  0 = the exact derivative of the forward (clamped colour in both passes).  The
 * two are identical wherever no composited colour channel is negative; where one is, the reference's gradient is not the
 * derivative of its own forward — the library follows the reference by default and offers the corrected form as the option. */
#define GUT_OPT_SORTED_REFERENCE_BACKWARD 2
/* GUT_OPT_EARLY_EXTRA_PERCENT (default 100, 0..100; unsorted variant): share of the 256-row blocks in which the second launch of
 * gut_optimize_rows_without_gradient (queued when the backward compositor starts) also takes the 64-row waves that HAVE tiles
 * but hold no Gaussian the forward compositor walked.  The backward compositor is bounded by the forward's per-tile depth, so
 * such waves cannot receive a gradient; their zero-gradient Adam step is the same arithmetic wherever it runs.  0 = only waves
 * without tiles take the side stream. */
#define GUT_OPT_EARLY_EXTRA_PERCENT 3
/* GUT_OPT_DEBUG_REPLACE_SCRATCH (developer probe, not a tuning knob): value = index of one of the handle's scratch buffers
 * (0 tiles_count, 1 tiles_offset, 2 proj_pos, 3 conic_opacity, 4 extent, 5 depth, 6 feat, 7 gradient rows, 8 scan temp, 9 / 10
 * unsorted / grouped keys, 11 / 12 unsorted / grouped ids, 13 sort temp, 14 ordered ids, 15 tile ranges, 16 / 17 traversal
 * depths, 18 / 19 tile launch order / ordered prefix): the buffer moves to a fresh device allocation, contents kept (synchronises
 * the device).  tools/scratch_placement.py uses it to find out whose physical placement the compositing kernels' two speeds
 *  belong to. */
/* GUT_OPT_FORWARD_TILE_ORDER (default -1; unsorted variant): launch order of the forward compositor's tiles.  1 = longest lists
 * first (a one-workgroup counting sort of the list lengths in front of it), 0 = image order, -1 = decided by the library from the
 * share of their lists the last frames walked (longest first above 25 %: then the length of a list says how long its tile will
 * run; read back with the intersection count, no extra synchronisation).  Results do not depend on it. */
#define GUT_OPT_FORWARD_TILE_ORDER 4
/* GUT_OPT_KERNEL_TIMING_SET (default 0; only with enable_kernel_timings): which kernel boundaries of the following frames are
 * bracketed by events.  0 = all of them; 2 = none (as with enable_kernel_timings = 0, switchable at run time: bench.py times its
 * steps this way and collects the per-kernel times in a second pass — the two dozen event records per train step cost 5 - 7 % of
 * a 2.4 ms step on MI355X); 1 = only the optimiser launches on the library's side stream (measured: SLOWER than either, the side
 * stream's second launch loses its head start over the backward compositor to the timing event's barrier packet and takes 1.7
 * instead of 1.1 ms — kept for experiments).  Timers of
 * boundaries that were not bracketed read -1. */
#define GUT_OPT_KERNEL_TIMING_SET 5
#define GUT_OPT_DEBUG_REPLACE_SCRATCH 100
int gut_set_option(gut_handle h, int32_t option, int32_t value);

/* per-kernel hipEvent timings of the last trace / trace_bwd (ms), for bench.py's roofline block.
 * Order: project, scan, expand, sort, ranges, render, render_bwd, project_bwd, optimizer (gut_optimize_after_bwd; -1 when
 * that call was not used), optimizer_early (gut_optimize_rows_without_gradient on its side stream, start of its first to end of
 * its second launch, idle gap included; -1 when not used), optimizer_early_2 (its second launch alone).  While a pose gradient
 * is set (gut_set_pose_gradient) project_bwd also holds its two launches (with GUT_BWD_SKIP_EPILOGUE: nothing else); render_bwd stays
 * the backward compositor alone.  Requires enable_kernel_timings; synchronises. */
#define GUT_NUM_KERNEL_TIMERS 11
int gut_kernel_times(gut_handle h, float* ms8);
/* mean per-kernel time over the (at most 64 most recent) trace/trace_bwd calls since the previous call of this
 * function; *count = number of forward calls averaged.  Synchronises. */
int gut_kernel_times_mean(gut_handle h, float* ms8, int32_t* count);

/* ---- "next" row N1: fused SSIM, replaces the external CUDA package `fused_ssim`
 * (threedgrut/model/losses.py:17-33: fused_ssim(img1, img2, padding="valid")).  Mean SSIM of two images with an
 * 11x11 Gaussian window (sigma 1.5), valid padding.  Images are addressed with element strides (channel, row,
 * pixel) so NCHW and NHWC tensors are both consumed in place.  Workspace (derivative maps + partial sums) is
 * caller-owned device memory of gut_ssim_workspace_bytes(); backward consumes the workspace its forward filled.
 * Return 0 on success. */
size_t gut_ssim_workspace_bytes(int32_t channels, int32_t height, int32_t width);
int gut_ssim_forward(void* stream, int32_t channels, int32_t height, int32_t width, int64_t stride_c, int64_t stride_h,
                     int64_t stride_w, const float* d_img1, const float* d_img2, void* d_workspace, float* d_mean_ssim);
int gut_ssim_backward(void* stream, int32_t channels, int32_t height, int32_t width, int64_t stride_c, int64_t stride_h,
                      int64_t stride_w, const float* d_img1, const float* d_img2, const void* d_workspace,
                      const float* d_upstream, float* d_grad_img1);

/* Fused photometric loss of the reference's train step (trainer.py:425-449, configs/base_gs.yaml:111-119), forward AND
 * gradient in three launches, no autograd:  image = rgb + background * (1 - alpha)  (model/background.py:78-93,
 * background 0 = black, 1 = white);  loss = lambda_l1 * mean|image - gt| + lambda_ssim * (1 - SSIM(image, gt)).
 * d_rgba [H,W,4] is gut_trace's ray_radiance_density, d_gt_rgb [H,W,3]; d_loss3 receives {loss, L1, SSIM};
 * d_rgba_grad [H,W,4] receives d(loss)/d(rgba), ready to be passed to gut_trace_bwd. */
size_t gut_photometric_workspace_bytes(int32_t height, int32_t width);
int gut_photometric_loss(void* stream, int32_t height, int32_t width, const float* d_rgba, const float* d_gt_rgb, float background,
                         float lambda_l1, float lambda_ssim, void* d_workspace, float* d_loss3, float* d_rgba_grad);

/* The same loss of a MASKED view: the reference multiplies prediction and ground truth by the batch's mask before its losses
 * (trainer.py:397-404).  d_mask: float32 [H,W], multiplied as it is (the readers produce 0 / 1):
 *     image = (rgb + background * (1 - alpha)) * mask,  gt' = gt * mask,
 *     L1 = sum |image - gt'| / (3 H W),  SSIM = the valid-region mean over the two masked images, count 3 (H - 10)(W - 10)
 * (neither denominator shrinks with the mask); d_loss3 receives {loss, L1, SSIM} of the masked images.  d(loss)/d(rgb) =
 * mask * d(loss)/d(image) and d(loss)/d(alpha) = -background * sum_c d(loss)/d(rgb_c); a pixel whose mask is 0 gets 0 in all four
 * channels of d_rgba_grad, whatever its colours are.  d_mask == NULL is gut_photometric_loss: the same kernel instantiations, the
 * same bits (so is, in value, an all-ones mask: a product with 1.0f is exact).  Workspace, launch count (the masked forms are
 * compile-time variants of the same two kernels) and stream behaviour as gut_photometric_loss. */
int gut_photometric_loss_masked(void* stream, int32_t height, int32_t width, const float* d_rgba, const float* d_gt_rgb,
                                const float* d_mask, float background, float lambda_l1, float lambda_ssim, void* d_workspace,
                                float* d_loss3, float* d_rgba_grad);

/* The same loss over a background IMAGE: every pixel is composited over its own colour, as the reference's `random` background
 * does in training (model/background.py:83-89: torch.rand_like(rays_d), per pixel), and as a constant RGB colour or an environment
 * image need.  d_background: float32 [H,W,3], contiguous, interleaved like d_gt_rgb:
 *     image = (rgb + B[y,x,:] * (1 - alpha)) * mask,  gt' = gt * mask          (d_mask == NULL: no mask, the factor is absent)
 * d(loss)/d(rgb) = mask * d(loss)/d(image) and d(loss)/d(alpha) = -sum_c B_c * d(loss)/d(rgb_c); all four channels of every pixel
 * of d_rgba_grad are written, and a pixel whose mask is 0 gets 0 in all four.  A pixel outside the image reads neither plane.
 * Further compile-time variants of the same two kernels, which the constant-background entry points above do not launch: those
 * return the bits they returned before.  An all-zero plane gives the values of background 0; an all-ones plane those of
 * background 1 up to the rounding of the alpha sum.  Returns 1 for a null pointer other than d_mask (d_background included) or
 * height / width <= 10.  Workspace (gut_photometric_workspace_bytes), launch count and stream behaviour as gut_photometric_loss. */
int gut_photometric_loss_background(void* stream, int32_t height, int32_t width, const float* d_rgba, const float* d_gt_rgb,
                                    const float* d_mask, const float* d_background, float lambda_l1, float lambda_ssim,
                                    void* d_workspace, float* d_loss3, float* d_rgba_grad);

/* Evaluation metrics of one view (the reference's test-split scoring, threedgrut/render.py:137-285), forward only, no gradient:
 * d_out4 receives { MSE, PSNR, SSIM, L1 } of image = rgb + background * (1 - alpha) against d_gt_rgb, values unclamped.
 * PSNR = 10 log10(1 / MSE) (a data range of 1; +inf for MSE == 0), SSIM = the valid-region mean SSIM of gut_photometric_loss (equal to
 * the reflect-padded, border-cropped mean of torchmetrics' StructuralSimilarityIndexMeasure).  The same forward kernel as the loss
 * without the derivative maps; the per-workgroup partials are summed in double in a fixed order (identical inputs, identical bits).
 * d_out4 may point into a caller's [V,4] device tensor.  Returns 1 for a null pointer or height / width <= 10.  Workspace: caller-owned
 * device memory of gut_image_metrics_workspace_bytes(). */
size_t gut_image_metrics_workspace_bytes(int32_t height, int32_t width);
int gut_image_metrics(void* stream, int32_t height, int32_t width, const float* d_rgba, const float* d_gt_rgb, float background,
                      void* d_workspace, float* d_out4);

/* COLOUR-CORRECTED evaluation metrics of one view (new functionality): the metrics above of the image mapped through
 * the affine colour transform that fits it best to the photo, so that a held-out photo's own exposure and white balance are not
 * charged to the model.  With comp_k = rgb_k + background (1 - alpha) in fp32 and x = (comp_0, comp_1, comp_2, 1), over the
 * P = height * width pixels (no mask, nothing clamped), E = [A | b] (3x4) minimises
 *     sum_pixels |A comp + b - gt|^2  +  ridge * P * |[A | b] - [I | 0]|_F^2 :
 *     G = sum x x^T + ridge P I_4,   C = sum x gt^T + ridge P [I_3; 0],   E^T = G^-1 C.
 * ridge > 0 is part of the definition (1e-6 in the Python surface): G is positive definite for every finite input (a constant or grey
 * image, an all-black render), directions the data do not show stay at the identity, SSE(E) <= SSE(identity), and for gt = A* comp + b*
 * exactly the corrected MSE is at most ridge |[A* | b*] - [I | 0]|_F^2 / 3.
 * d_out4 receives { MSE, PSNR, SSIM, L1 } of image_c = fma(E[c][0], comp_0, fma(E[c][1], comp_1, fma(E[c][2], comp_2, E[c][3])))
 * against d_gt_rgb, counts and definitions as gut_image_metrics; d_exposure12 (may be NULL) receives the fitted E, row-major 3x4; both
 * may point into a caller's [V,4] / [V,12] device tensors.  Four launches on `stream`, nothing copied to the host, nothing
 * synchronised: the 22 moments (10 of G, 12 of C) accumulated in double from the first product, one row of 22 doubles per 1024
 * pixels, no atomics; one workgroup that sums the rows in a fixed order, adds the ridge, factors G by Cholesky and solves, in double;
 * the metrics forward on E [comp; 1], reading E from the workspace; the finish of gut_image_metrics.  Identical inputs, identical
 * bits.  Non-finite inputs give non-finite outputs.  d_rgba must be 16-byte and d_workspace 8-byte aligned (torch allocations are).
 * Returns 1 — on the host, before anything is queued — for a null pointer other than d_exposure12, height / width <= 10, a ridge that
 * is not finite or not > 0, or a misaligned workspace; 2 for a launch failure.  Workspace: gut_image_metrics_cc_workspace_bytes(). */
size_t gut_image_metrics_cc_workspace_bytes(int32_t height, int32_t width);
int gut_image_metrics_cc(void* stream, int32_t height, int32_t width, const float* d_rgba, const float* d_gt_rgb,
                         float background, float ridge, void* d_workspace, float* d_out4,
                         float* d_exposure12 /* receives the fitted E, row-major 3x4; may be NULL */);

/* ---- "next" row N2: parameter activation + fused Adam ----
 * gut_activate_pack: raw rows [N,12] (pos3, density logit, quat4, log-scale3, unused) -> activated rows
 *   (pos3, sigmoid, quat/|quat|, exp, |quat|) = the particle_density the tracer consumes (model.py:74-93 +
 *   tracer.py:176-178 in one pass).
 * gut_adam_step: in-place Adam on an [rows, cols] fp32 tensor, cols a multiple of 4 and <= 64, per-column learning
 *   rates (host array).  step >= 1: torch.optim.Adam bias correction; step == 0: none (the reference's SelectiveAdam,
 *   optimizers.cu:47-79).  d_visibility != NULL: rows with visibility == 0 are skipped entirely. */
int gut_activate_pack(void* stream, uint32_t num_particles, const float* d_raw12, float* d_act12);
int gut_adam_step(void* stream, uint64_t rows, uint32_t cols, float* d_param, const float* d_grad, float* d_exp_avg,
                  float* d_exp_avg_sq, const float* lr_per_col, float beta1, float beta2, float eps, uint32_t step,
                  const float* d_visibility);

/* ---- Lazy moment decay of the fused optimiser entry points (gut_optimize_*, gut_adam_unwalked_waves_ex, gut_sh_adam_step_ex) ----
 * Adam with a zero gradient still decays both moments of every parameter (torch.optim.Adam semantics), i.e. reads AND writes
 * 2 x 236 bytes per Gaussian per step for nothing but two multiplications by constants.  With a GutLazyMoments the zero-gradient
 * update of a 64-row wave that cannot receive a gradient in this step — no row of it has a tile, or the forward compositor walked
 * none of its Gaussians (the backward is bounded by the forward's per-tile depth) — READS the moments, brings them up to date in
 * registers, updates the parameters, and does NOT write the moments back: d_wave_step[w] (one uint32 per wave, caller-owned,
 * zero-initialised) holds the step up to which the stored moments of wave w are current, and the next kernel that reads them
 * multiplies by beta^(steps missed), taken from the caller's tables d_pow_beta1/2[k] = (float) beta^k, k < table_len
 * (d_pow[0] = 1).  Every wave that can receive a gradient is brought up to date, updated and written as before.  The rule
 * does not depend on which kernel walks a wave, so one-pass and two-pass steps stay bit-identical.  The result differs from
 * writing the moments every step only by the rounding of beta^k against k successive multiplications (~1e-7 relative).
 * gut_sync_moments brings every stored moment up to `step` (call it before moving rows between waves, reading the moments
 * from outside, or every table_len / 2 steps).  Not available with a visibility mask (SelectiveAdam does not decay at all). */
typedef struct GutLazyMoments {
    uint32_t* d_wave_step;       /* [ceil(N / 64)] */
    const float* d_pow_beta1;    /* [table_len] */
    const float* d_pow_beta2;    /* [table_len] */
    uint32_t table_len;
    uint32_t* d_overrun;         /* may be NULL; one word, caller-zeroed: set to 1 by any kernel that met a wave whose stored moments
                                    had missed table_len or more steps (its decay factor does not exist in the tables: the caller
                                    resumed with a wave_step that does not belong to its step counter, or never called
                                    gut_sync_moments).  The caller checks it where it synchronises anyway (ABI 5) */
} GutLazyMoments;
int gut_sync_moments(void* stream, uint32_t num_particles, float* d_raw_m, float* d_raw_v, float* d_sh_m, float* d_sh_v,
                     const GutLazyMoments* lazy, uint32_t step /* the last optimiser step applied */);

/* lib_optimizers_cc.selective_adam_update (threedgrut/optimizers/optimizers.cu:47-117, bound in optimizers/__init__.py:113-123):
 * the SelectiveAdam update of one [rows, cols] fp32 parameter of ANY width, rows whose visibility byte is 0 untouched, no bias
 * correction.  d_visibility: one byte per row (a torch.bool tensor).  3dgrut_amd/optimizers.py wraps it in the reference's
 * `SelectiveAdam(torch.optim.Adam)` class. */
int gut_selective_adam(void* stream, uint64_t rows, uint32_t cols, float* d_param, const float* d_grad, float* d_exp_avg,
                       float* d_exp_avg_sq, const uint8_t* d_visibility, float lr, float beta1, float beta2, float eps);

/* Fused "SH gradient + Adam" step of the native trainer.  For every Gaussian: Adam on the raw [N,12] row with
 * d_raw_grad12 (already summed over views), then the [N,48] SH row with the gradient
 *     sum_v Y_k(normalize(pos - camera_position[v])) * mrgb[v][i][c]   (k < (sh_degree+1)^2, else 0)
 * rebuilt on the fly from num_views compact rows (gut_trace_bwd_ex(..., GUT_BWD_COMPACT_RADIANCE_GRADS)); both
 * gradients are scaled by grad_scale (1/num_views for a mean over views).  pos is the pre-update position.
 * lr12/lr48: host arrays of per-column learning rates; step/visibility as in gut_adam_step.
 * d_act12_out (may be NULL): if given, every updated row's activation (what gut_activate_pack would compute from the new
 * raw row) is written there, so the next gut_trace needs no separate activation pass.
 * mrgb_view_stride: rows between consecutive views in d_mrgb (0 = num_particles).  All per-Gaussian pointers may be
 * offset to a row range [r0, r1) with num_particles = r1 - r0: that is how the data-parallel trainer pipelines the
 * optimiser over chunks of Gaussians behind the gradient exchange of the following chunk. */
int gut_sh_adam_step(void* stream, uint32_t num_particles, int32_t sh_degree, uint32_t num_views,
                     const float* d_camera_positions /* device [num_views,3] */, const float* d_mrgb /* [num_views,N,3] */,
                     const float* d_raw_grad12, float grad_scale,
                     float* d_raw12, float* d_raw_m, float* d_raw_v, float* d_sh48, float* d_sh_m, float* d_sh_v,
                     const float* lr12, const float* lr48, float beta1, float beta2, float eps, uint32_t step,
                     const float* d_visibility, float* d_act12_out, uint32_t mrgb_view_stride);

/* Epilogue of the last gut_trace_bwd_ex(..., GUT_BWD_SKIP_EPILOGUE) + gut_sh_adam_step for ONE view in a single kernel:
 * chains the handle's gradient rows to the raw parameters (sigmoid / normalise / exp recomputed from d_raw12, which must be
 * the rows the forward's gut_activate_pack input was made from), rebuilds the SH gradient from the masked dL/dRGB and
 * applies Adam to d_raw12 / d_sh48.  d_camera_position: device [3] sensor position of the view, or NULL = the sensor position of
 * the cached forward, which the library keeps on the device (the floats its projection evaluated the colours from).  Other arguments as in
 * gut_sh_adam_step.  Consumes the backward context. */
int gut_optimize_after_bwd(gut_handle h, void* stream, int32_t num_active_features, const float* d_camera_position,
                           float* d_raw12, float* d_raw_m, float* d_raw_v, float* d_sh48, float* d_sh_m, float* d_sh_v,
                           const float* lr12, const float* lr48, float beta1, float beta2, float eps, uint32_t step,
                           const float* d_visibility, float* d_act12_out, const GutLazyMoments* lazy /* may be NULL */);

/* Optional first half of that optimiser step, to be called BETWEEN gut_trace and gut_trace_bwd_ex(..., GUT_BWD_SKIP_EPILOGUE) on
 * the forward's stream.  Gaussians that cannot receive a gradient from this view get their Adam step (same arithmetic as
 * gut_optimize_after_bwd with an exactly-zero gradient: moments decay, parameters move on their momentum, activation rows
 * rewritten) on a side stream owned by the handle, as pure HBM streaming UNDER and beside the VALU-bound compositing kernels of
 * the same iteration.  They are taken by whole 64-row waves, in two launches of a persistent kernel with a small fixed footprint:
 *   1. right away, ordered behind the binning part of the forward only: waves in which no row has a tile
 *      (tiles_count == 0), in the first 60 % of the row blocks with lazy moments (a 32-register form of the kernel, which
 *      leaves the forward compositor all of its waves), in the first quarter otherwise;
 *   2. when gut_trace_bwd_ex queues the backward compositor: the remaining waves without tiles and — unsorted variant,
 *      GUT_OPT_EARLY_EXTRA_PERCENT — the waves that have tiles but hold no Gaussian among the list entries the forward
 *      compositor walked (the backward compositor is bounded by the forward's per-tile depth).
 * The following gut_optimize_after_bwd (mandatory; same pointers and hyper-parameters; d_visibility must be NULL) then walks only
 * the other waves and orders the caller's stream behind the side stream.  The parameters after the two calls are those of
 * gut_optimize_after_bwd alone; every row of a wave the side stream took is bit-identical to it.  The caller must not touch the
 * parameter tensors on other streams between the two calls. */
int gut_optimize_rows_without_gradient(gut_handle h, void* stream, float* d_raw12, float* d_raw_m, float* d_raw_v, float* d_sh48,
                                       float* d_sh_m, float* d_sh_v, const float* lr12, const float* lr48, float beta1,
                                       float beta2, float eps, uint32_t step, float* d_act12_out,
                                       const GutLazyMoments* lazy /* may be NULL; must match gut_optimize_after_bwd's */);

/* Ends an optimiser step that gut_optimize_rows_without_gradient began but gut_optimize_after_bwd cannot finish (the caller's
 * loss raised, the backward was rejected, ...): every wave the side stream does not own takes the same Adam step with an
 * exactly-zero gradient (whatever the backward compositor may already have accumulated for this view is discarded and the
 * gradient rows are left zero), the caller's stream is ordered behind the side stream, and the handle accepts gut_trace again.
 * Afterwards every row has taken exactly one step of iteration `step`, as if the view had given no gradient at all.  No-op
 * (returns 0) when no step is half applied. */
int gut_optimize_finish_without_gradient(gut_handle h, void* stream);

/* ---- Sparse gradient exchange of the data-parallel trainer (new functionality, the reference is single-GPU) ----
 * A view gives a gradient only to the Gaussians its rays hit.  Instead of dense [N,12] + [N,3] tensors per view, the ranks
 * exchange lists of 64-byte records, one per Gaussian with a non-zero gradient row:
 *     f32[16] = { d pos3, d density logit, d quat4 (un-normalised), d log-scale3, row id (uint32 bits), masked dL/dRGB 3, 0 }
 * (the gradient w.r.t. the RAW parameters, as GUT_BWD_RAW_PARAMETER_GRADS | GUT_BWD_COMPACT_RADIANCE_GRADS would write it).
 *
 * gut_compact_gradient_rows: epilogue of the last gut_trace_bwd_ex(..., GUT_BWD_SKIP_EPILOGUE).  d_particle_density: the
 *   activated rows the forward was given (gut_activate_pack layout).  d_records: [capacity,16] with capacity >= num_particles
 *   (so it cannot overflow); *d_count (device uint32) receives the number of records.  Record order is unspecified; every
 *   row id occurs at most once.  Consumes the backward context (the handle's gradient rows are left zero).
 * gut_scatter_gradient_records: adds `count` records of ONE view into the dense accumulator d_raw_grad12 [N,12] and stores
 *   their dL/dRGB into that view's slab d_mrgb_view [N,3].  Both must be zero wherever no record lands (allocate zeroed once;
 *   gut_sh_adam_step_ex(..., GUT_ADAM_CLEAR_CONSUMED_GRADS) zeroes what it consumed).  Scatter the views one call after the
 *   other in the same order on every rank: the sums are then formed in the same order everywhere and replicas stay
 *   bit-identical.
 * gut_sh_adam_step_ex: gut_sh_adam_step with flags; GUT_ADAM_CLEAR_CONSUMED_GRADS writes zeros over every non-zero row of
 *   d_raw_grad12 / d_mrgb it read. */
#define GUT_ADAM_CLEAR_CONSUMED_GRADS 1u
#define GUT_GRADIENT_RECORD_FLOATS 16
int gut_compact_gradient_rows(gut_handle h, void* stream, const float* d_particle_density, float* d_records, uint32_t capacity,
                              uint32_t* d_count);
int gut_scatter_gradient_records(void* stream, const float* d_records, uint32_t count, uint32_t num_particles, float* d_raw_grad12,
                                 float* d_mrgb_view);
/* the same with the number of valid records read ON THE DEVICE: min(*d_count, max_count) records are taken.  Lets the caller
 * queue the scatter before the host has seen the ranks' record counts (3dgrut_amd/dp.py: RecordExchange). */
int gut_scatter_gradient_records_dev(void* stream, const float* d_records, const uint32_t* d_count, uint32_t max_count,
                                     uint32_t num_particles, float* d_raw_grad12, float* d_mrgb_view);
int gut_sh_adam_step_ex(void* stream, uint32_t num_particles, int32_t sh_degree, uint32_t num_views,
                        const float* d_camera_positions, float* d_mrgb, float* d_raw_grad12, float grad_scale,
                        float* d_raw12, float* d_raw_m, float* d_raw_v, float* d_sh48, float* d_sh_m, float* d_sh_v,
                        const float* lr12, const float* lr48, float beta1, float beta2, float eps, uint32_t step,
                        const float* d_visibility, float* d_act12_out, uint32_t mrgb_view_stride, uint32_t flags,
                        const uint8_t* d_wave_flags /* may be NULL; else waves with flag 0 are left alone, see below */,
                        const GutLazyMoments* lazy /* may be NULL */);

/* Data-parallel form of the side-stream optimiser pass (single-view form: gut_optimize_rows_without_gradient).
 * gut_mark_walked_waves: after gut_trace, same stream: d_wave_flags [ceil(N/64)] bytes := 1 for every 64-row wave that holds a
 *   Gaussian among the list entries the forward compositor walked (sorted variant: every wave with a tile), else 0.  The
 *   backward compositor gives gradients to those Gaussians only.  MAX-all-reduce the flags over the ranks (94 KB at 6 M): a
 *   wave whose flag is still 0 receives no gradient from ANY view of the step.
 * gut_adam_unwalked_waves: zero-gradient Adam step (moments decay, parameters move on their momentum, activation rows
 *   rewritten) of every wave whose flag is 0, as a persistent kernel with a small fixed footprint: queue it on a side stream
 *   as soon as the reduced flags are there; it streams under the backward compositor, the gradient exchange and the call below.
 * gut_sh_adam_step_ex(..., d_wave_flags) then skips exactly those waves.  Rows of the skipped waves are bit-identical to what
 *   gut_sh_adam_step_ex without flags computes for them (their gradient is exactly zero). */
int gut_mark_walked_waves(gut_handle h, void* stream, uint8_t* d_wave_flags);
int gut_adam_unwalked_waves(void* stream, uint32_t num_particles, const uint8_t* d_wave_flags, float* d_raw12, float* d_raw_m,
                            float* d_raw_v, float* d_sh48, float* d_sh_m, float* d_sh_v, const float* lr12, const float* lr48,
                            float beta1, float beta2, float eps, uint32_t step, float* d_act12_out);
/* ... with lazy moment decay (NULL = as above) */
int gut_adam_unwalked_waves_ex(void* stream, uint32_t num_particles, const uint8_t* d_wave_flags, float* d_raw12, float* d_raw_m,
                               float* d_raw_v, float* d_sh48, float* d_sh_m, float* d_sh_v, const float* lr12, const float* lr48,
                               float beta1, float beta2, float eps, uint32_t step, float* d_act12_out, const GutLazyMoments* lazy);

/* ---- The MCMC recipe's opacity and scale regularisers (configs/base_mcmc.yaml:13-18, threedgrut/trainer.py:432-449) ----
 *     loss_opacity = lambda_opacity * mean |sigmoid(d)|  over N,   loss_scale = lambda_scale * mean |exp(s)|  over 3N
 * Their gradient w.r.t. a raw row (density logit d, column 3; log-scales s_k, columns 8..10) depends on that row alone:
 *     dL/dd = density_coeff * sigmoid(d) (1 - sigmoid(d)),   dL/ds_k = scale_coeff * exp(s_k)
 * with density_coeff = lambda_opacity / N and scale_coeff = lambda_scale / (3 N), evaluated on the parameters BEFORE the update.
 * Every optimiser kernel that updates a row adds it to the row's photometric gradient (after the 1/world scaling of the data-parallel
 * forms: it is counted once).  With a visibility mask (SelectiveAdam) rows with visibility 0 stay untouched, regulariser included.
 * With a regulariser no row is gradient-free in the [N,12] block, so its moments are stored every step for every row; the lazy
 * decay (GutLazyMoments) then governs the [N,48] block only, and gut_sync_moments_ex must be given the same setting.  Switching
 * between "no regulariser" and "a regulariser" needs a gut_sync_moments(_ex) under the OLD setting first.
 * d_partials (optional): [ceil(N / 64), 2] floats; the kernel that owns 64-row wave w writes (sum of sigmoid(d), sum of exp(s_k)) of
 * the wave's pre-update rows, all of them (SelectiveAdam's untouched rows included).  Row-range calls (chunks) offset it by r0 / 64.
 * A GutRegularisation with both coefficients 0 is the same as NULL: the unregularised kernels, bit for bit. */
typedef struct GutRegularisation {
    float density_coeff;   /* lambda_opacity / N */
    float scale_coeff;     /* lambda_scale / (3 N) */
    float* d_partials;     /* [ceil(N / 64), 2] or NULL */
} GutRegularisation;
/* handle paths (gut_optimize_rows_without_gradient + gut_optimize_after_bwd, or gut_optimize_finish_without_gradient): consumed by the
 * next optimiser step; NULL clears it */
int gut_set_regularisation(gut_handle h, const GutRegularisation* reg);
/* stateless data-parallel paths: gut_sh_adam_step_ex / gut_adam_unwalked_waves_ex with a regulariser (NULL = none) */
int gut_sh_adam_step_regularised(void* stream, uint32_t num_particles, int32_t sh_degree, uint32_t num_views,
                                 const float* d_camera_positions, float* d_mrgb, float* d_raw_grad12, float grad_scale,
                                 float* d_raw12, float* d_raw_m, float* d_raw_v, float* d_sh48, float* d_sh_m, float* d_sh_v,
                                 const float* lr12, const float* lr48, float beta1, float beta2, float eps, uint32_t step,
                                 const float* d_visibility, float* d_act12_out, uint32_t mrgb_view_stride, uint32_t flags,
                                 const uint8_t* d_wave_flags, const GutLazyMoments* lazy, const GutRegularisation* reg);
int gut_adam_unwalked_waves_regularised(void* stream, uint32_t num_particles, const uint8_t* d_wave_flags, float* d_raw12,
                                        float* d_raw_m, float* d_raw_v, float* d_sh48, float* d_sh_m, float* d_sh_v, const float* lr12,
                                        const float* lr48, float beta1, float beta2, float eps, uint32_t step, float* d_act12_out,
                                        const GutLazyMoments* lazy, const GutRegularisation* reg);
/* gut_sync_moments under a regulariser setting (non-NULL with a coefficient != 0: only the [N,48] moments are brought up to date) */
int gut_sync_moments_ex(void* stream, uint32_t num_particles, float* d_raw_m, float* d_raw_v, float* d_sh_m, float* d_sh_v,
                        const GutLazyMoments* lazy, uint32_t step, const GutRegularisation* reg);
/* the unfused optimiser (gut_adam_step on a materialised raw gradient): adds the regulariser's gradient into d_raw_grad12 [N,12]
 * (after any exchange) and writes the partials */
int gut_regularisation_gradient(void* stream, uint32_t num_particles, const float* d_raw12, float* d_raw_grad12,
                                const GutRegularisation* reg);
/* the loss values from the partials of the last step, reduced in a fixed order: *d_opacity_loss = lambda_opacity * mean sigmoid,
 * *d_scale_loss = lambda_scale * mean exp (device floats); d_loss (may be NULL): both are added onto that device float.  Order it
 * behind every stream that wrote partials. */
int gut_regularisation_loss(void* stream, uint32_t num_particles, const float* d_partials, float lambda_opacity, float lambda_scale,
                            float* d_opacity_loss, float* d_scale_loss, float* d_loss);

/* ---- "next" row N3: the densification statistics of GSStrategy.update_gradient_buffer (threedgrut/strategy/gs.py:
 * 106-115), which the reference's trainer runs between backward and optimiser in every iteration up to densify.end_iteration
 * (trainer.py:741-743): for every Gaussian whose position gradient of THIS view is non-zero,
 *     norm_accum[i] += | grad_i * |position_i - sensor_position| | / 2,      norm_denom[i] += 1.
 * gut_position_gradient_statistics is that as one kernel (grad / positions: rows of `*_stride` floats, first three columns used;
 * d_sensor_position: device float[3]).  gut_set_position_gradient_statistics folds it into the NEXT gut_optimize_after_bwd on the
 * handle (that kernel holds each row's gradient and pre-update position in registers anyway; the setting is consumed by that one
 * call, so the caller may reallocate its buffers between steps; NULL, NULL clears it): the step keeps its fused one- or two-pass
 * optimiser instead of materialising the [N,3] gradient for a hook (6.5 -> 2.6 ms per step at 6 M Gaussians). */
int gut_position_gradient_statistics(void* stream, uint32_t num_particles, const float* d_position_grad, uint32_t grad_stride,
                                     const float* d_positions, uint32_t position_stride, const float* d_sensor_position,
                                     float* d_norm_accum, int32_t* d_norm_denom);
int gut_set_position_gradient_statistics(gut_handle h, float* d_norm_accum, int32_t* d_norm_denom);

/* ---- Camera-pose gradient of a view (new functionality, the reference keeps its poses fixed) ----
 * The backward differentiates the per-ray 3-D evaluation only (the projection decides tile membership and is not differentiated, the SH
 * view direction carries no gradient), and that evaluation depends on the relative placement of ray and Gaussian alone.  Moving a
 * global-shutter camera rigidly therefore equals moving every Gaussian by the inverse motion with its colour held fixed, and the
 * gradient w.r.t. the camera is a reduction of the per-Gaussian gradient rows the backward compositor has written anyway.  With
 * g_mu / g_q a row's gradient w.r.t. its activated position / quaternion (wxyz), q that quaternion and c the sensor position:
 *     F = sum_i g_mu_i,     M = sum_i (mu_i - c) x g_mu_i + tau_i,     tau_i,k = 1/2 g_q_i . ((0, e_k) (x) q_i),  k = x, y, z
 * and for the world-axis twist  c' = c + rho,  R_c2w' = exp([phi]x) R_c2w  (rotation about the camera centre):
 *     dL/d rho = -F,   dL/d phi = -M.
 * gut_set_pose_gradient(h, d_out8): while d_out8 (device float[8], caller-owned, must stay valid) is set, EVERY gut_trace_bwd* on the
 * handle queues the reduction on its stream right behind the backward compositor and before any epilogue (the epilogues, the fused
 * optimiser and gut_compact_gradient_rows included, zero the rows as they read them) and leaves
 *     d_out8 = { F[3], M[3], number of rows summed (the Gaussians with a tile), 0 }.
 * The rows are only read.  c is the sensor position the forward's projection left on the device.  Two launches, fp32 accumulators,
 * partial sums combined in a fixed order, no atomics: the numbers are a pure function of the rows.  A view whose start and end poses
 * differ (a rolling shutter in motion) has no single rigid motion: gut_trace_bwd* then fails before it queues anything, and the handle
 * stays as it was.  With num_particles == 0 the eight floats are set to zero.  NULL (the default) switches it off: nothing is
 * launched and nothing else changes. */
int gut_set_pose_gradient(gut_handle h, float* d_out8);
/* Adam on the six pose coordinates of one view, from the eight floats above: gradient (-F, -M); d_m6 / d_v6 / d_count (one int32) are
 * that view's own moments and visit count, which is advanced by one and used for the bias correction; lr_translation applies to rho,
 * lr_rotation to phi.  d_delta6 receives the increment (d rho, d phi): c += d rho, R_c2w <- exp([d phi]x) R_c2w.  One launch. */
int gut_pose_adam_step(void* stream, const float* d_grad8, float* d_m6, float* d_v6, int32_t* d_count, float lr_translation,
                       float lr_rotation, float beta1, float beta2, float eps, float* d_delta6);
/* The backward for the pose gradient ALONE (pose alignment of held-out views with the Gaussians frozen).  Arguments as
 * gut_trace_bwd_ex without the gradient outputs and without flags; d_particle_density may be NULL after a *_fields forward (the rows
 * that forward packed).  Follows any forward on the same handle and stream, runs the backward compositor as every other backward
 * does (both variants) and then the CONSUMING form of the reduction above: the same arithmetic, grid and summation order, so d_out8
 * is the same pure function of the rows, and every gradient row with a tile is left as 64 zero bytes.  No epilogue runs and nothing
 * of size N is written besides the handle's own gradient rows.  Afterwards the rows are known to be zero (the next backward queues
 * no clear), NO backward context is pending (gut_optimize_after_bwd and gut_compact_gradient_rows refuse) and the next gut_trace
 * is accepted.  Refused before anything is queued, the handle left as it was: no pose output set, pose_start != pose_end,
 * gut_optimize_rows_without_gradient was called for this forward, arguments that differ from the cached forward.  With
 * num_particles == 0 the eight floats are set to zero.  Timers: the two launches count towards project_bwd. */
int gut_trace_bwd_pose(gut_handle h, void* stream, uint32_t frame_number, int32_t num_active_features, uint32_t num_particles,
                       const float* d_particle_density, int32_t width, int32_t height, const float* d_ray_origin,
                       const float* d_ray_direction, const GutCamera* camera, const float* d_ray_radiance_density,
                       const float* d_ray_radiance_density_grad, const float* d_ray_hit_distance,
                       const float* d_ray_hit_distance_grad /* may be NULL */);

/* ---- Per-Gaussian contribution scores (new functionality, the reference has none) ----
 * What each Gaussian contributed to the view of the cached forward, from the blending weights w = T * alpha the forward compositor
 * formed (T: the ray's transmittance in front of the Gaussian): per Gaussian, over every pixel in which the forward composited it,
 * the sum of w, the largest w and the number of such pixels (the pixels the hit-count plane counts).  One record of 16 bytes per
 * Gaussian, ACCUMULATED INTO: the caller zeroes the array once and calls this after the forward of every view it wants scored. */
typedef struct GutContribution {
    uint64_t weight_sum_q32;   /* sum over (view, tile) of round(tile_sum * 2^32): integer adds, so the total is independent of arrival order */
    uint32_t max_weight_bits;  /* float bits of the largest w seen; atomicMax on the bits (w >= 0, so the bits order like the values) */
    uint32_t pixels;           /* pixels, over all views, in which the Gaussian was composited (w > 0) */
} GutContribution;
/* Follows any forward on the same handle and stream (arguments as gut_trace_bwd_pose's view; d_particle_density may be NULL after a
 * *_fields forward: the rows that forward packed).  Two launches: the tile order by the forward's walked depth, then one walk of
 * what the forward walked — the same ordered-id lists, bounded by the forward's per-tile depth as the backward compositor bounds
 * them, the forward's tests by the forward's arithmetic, no colours read and no image written.  Per (tile, Gaussian) the 256 weights
 * are reduced in a fixed order (inside each wave, then the four waves in wave order); a Gaussian no pixel of the tile composited
 * issues nothing, the others one 64-bit integer add, one 32-bit integer max and one 32-bit integer add.  Identical inputs therefore
 * give identical bytes, from run to run and whatever the order in which views are accumulated; a Gaussian without a tile, or behind
 * every walked prefix, keeps its 16 bytes.  The forward context is NOT consumed: the gradient rows, the backward's traversal depths
 * and every forward output are left alone, and any backward (or another gut_trace_contribution) may follow.
 * Unsorted variant at the default kernel only.  Returns 1 on the host, before anything is queued and with the handle left as it was,
 * for: a null handle, camera or ray pointer; d_scores NULL or not 8-byte aligned with num_particles > 0; no forward on this stream;
 * arguments or a camera that differ from the cached forward; a handle created with k_buffer_size > 0 or particle_kernel_degree != 2;
 * gut_optimize_rows_without_gradient called for this forward.  num_particles == 0 or a forward without intersections: nothing is
 * queued, 0 is returned.  Not part of the kernel timers. */
int gut_trace_contribution(gut_handle h, void* stream, uint32_t frame_number, int32_t num_active_features, uint32_t num_particles,
                           const float* d_particle_density /* NULL: the rows the last *_fields forward packed */,
                           int32_t width, int32_t height, const float* d_ray_origin, const float* d_ray_direction,
                           const GutCamera* camera, GutContribution* d_scores /* [N], accumulated into */);

/* ---- Contribution scores weighted by a per-pixel plane (new functionality) ----
 * gut_trace_contribution_weighted is gut_trace_contribution — its scope, its walk, its refusals, nothing consumed — with a float
 * plane [H,W] of the view: every weight w is also multiplied by e = min(max(plane[pixel], 0), 1) (the clamp is part of the contract:
 * a NaN counts as 0, a value above 1 as 1) and the products are summed per Gaussian, by the reduction of the plain sum, into
 * d_weighted_q32 [N]: round(tile_sum * 2^32) per (tile, Gaussian), one 64-bit integer add, ACCUMULATED INTO like the records, so the
 * totals are independent of the order of tiles and views.  A plane of ones gives weight_sum_q32 bit for bit.  With the error plane of
 * gut_pixel_error it is the rendering error each Gaussian is responsible for; with a 0/1 mask, weighted / weight_sum is the share of
 * the Gaussian that lies inside the mask.  d_scores NULL: the weighted sums alone; otherwise the records are written in the same walk
 * and equal those of gut_trace_contribution.  Additionally refused: d_pixel_weight NULL; d_weighted_q32 NULL or not 8-byte aligned
 * with num_particles > 0. */
int gut_trace_contribution_weighted(gut_handle h, void* stream, uint32_t frame_number, int32_t num_active_features,
                                    uint32_t num_particles, const float* d_particle_density /* NULL: the packed rows */,
                                    int32_t width, int32_t height, const float* d_ray_origin, const float* d_ray_direction,
                                    const GutCamera* camera, const float* d_pixel_weight /* [H,W] */,
                                    GutContribution* d_scores /* [N] or NULL */, uint64_t* d_weighted_q32 /* [N], accumulated into */);
/* The per-pixel rendering error of a view, a float plane [H,W] in [0, 1] (operands as gut_photometric_loss_exposure's; d_mask,
 * d_background and d_exposure12 may each be NULL):
 *     comp_k = rgb_k + B_k (1 - alpha),   img_c = A[c] . comp + b_c with E = [A | b] read from device memory (comp_c without E),
 *     error  = min(max((|img_0 - gt_0| + |img_1 - gt_1| + |img_2 - gt_2|) / 3, 0), 1) * mask
 * One elementwise launch, no workspace, no synchronisation; every element of d_error is written.  Returns 1 on the host, before
 * anything is queued, for a null d_rgba, d_gt_rgb or d_error or a height or width below 1; 2 for a launch failure. */
int gut_pixel_error(void* stream, int32_t height, int32_t width, const float* d_rgba, const float* d_gt_rgb,
                    const float* d_mask, const float* d_background, float background, const float* d_exposure12, float* d_error);

/* ---- Rendering per-Gaussian attributes (new functionality, the reference has none) ----
 * gut_trace_attributes is the other direction of gut_trace_contribution_weighted: where that sums a per-pixel plane onto the
 * Gaussians, this blends per-Gaussian values into the pixels, out[k][pixel] = sum over the Gaussians the forward composited in the
 * pixel of w * d_attributes[i][k], with the forward's blending weights w = T * alpha.  Scope, walk and refusals are
 * gut_trace_contribution's: it follows any forward on the same handle and stream, walks what that forward walked by the forward's
 * arithmetic, consumes nothing (gradient rows, traversal depths and forward outputs are left alone) and may be followed by any
 * backward, contribution call or further attribute call.  The channels are rendered four at a time, one walk per group (1 + ceil(K/4)
 * launches with the tile order); a pixel's sum is formed in the order of its tile's list by one fused multiply-add per composited
 * Gaussian and channel, in the lane's registers: no atomics, identical inputs give identical bytes, a channel's plane does not depend
 * on the other channels, and negated attributes give the negated image.  A Gaussian's values are multiplied in only where it was
 * composited: a non-finite value reaches those pixels alone.  d_out is planar [K,H,W] (each plane is a plane for
 * gut_trace_contribution_weighted) and written in full, 0 where nothing was composited, so it needs no initialisation; with
 * num_particles == 0 or a forward without intersections it is zero-filled by one memset on the stream.  Rows of d_attributes are read
 * by 16-byte loads where num_channels is a multiple of four and the pointer is 16-byte aligned, by 4-byte loads otherwise: no
 * alignment beyond a float's is required.  Additionally refused, on the host before anything is queued: num_channels outside 1..64;
 * d_attributes NULL with num_particles > 0; d_out NULL or not 4-byte aligned.  Not part of the kernel timers. */
int gut_trace_attributes(gut_handle h, void* stream, uint32_t frame_number, int32_t num_active_features, uint32_t num_particles,
                         const float* d_particle_density /* NULL: the packed rows */, int32_t width, int32_t height,
                         const float* d_ray_origin, const float* d_ray_direction, const GutCamera* camera,
                         int32_t num_channels /* 1..64 */, const float* d_attributes /* [N, num_channels] row-major */,
                         float* d_out /* [num_channels, H, W], fully written */);

/* ---- The gradient of rendered attributes with respect to the attributes (new functionality) ----
 * gut_trace_attributes_bwd is the adjoint of gut_trace_attributes: for a cotangent d_out_grad [K,H,W] of the planes,
 *     d_attributes_grad[i][k] = sum over the pixels in which the forward composited Gaussian i of w * d_out_grad[k][pixel],
 * with the forward's blending weights w, signed and without a clamp (the exact adjoint, where gut_trace_contribution_weighted is the
 * adjoint for planes in [0, 1] only).  The geometry gets no gradient.  Scope, walk and refusals are gut_trace_contribution's; it
 * consumes nothing and may be followed by any backward, contribution or attribute call.  Four channels per walk.  A non-finite
 * cotangent value counts as 0.  The sums are formed in a fixed order per tile and added across tiles as 64-bit integers in units of
 * 2^-s_k, s_k a power-of-two exponent taken per channel from the plane's largest |value| (unit: at most 2^-39 of it): identical
 * inputs give identical bytes whatever the order in which tiles run, a channel does not depend on the other channels of the call,
 * a negated cotangent gives the negated gradient and a cotangent scaled by a power of two the scaled gradient.  Every element of
 * d_attributes_grad is written, 0 for rows nobody composited; with num_particles == 0 or a forward without intersections it is
 * zero-filled by one memset and nothing is walked.  Per group of four channels: two memsets (32 bytes per Gaussian of handle
 * scratch), a reduction of the planes, the walk and one pass over the rows.  Additionally refused, on the host before anything is
 * queued: num_channels outside 1..64; d_out_grad or d_attributes_grad NULL with num_particles > 0, or not 4-byte aligned. */
int gut_trace_attributes_bwd(gut_handle h, void* stream, uint32_t frame_number, int32_t num_active_features, uint32_t num_particles,
                             const float* d_particle_density /* NULL: the packed rows */, int32_t width, int32_t height,
                             const float* d_ray_origin, const float* d_ray_direction, const GutCamera* camera,
                             int32_t num_channels /* 1..64 */, const float* d_out_grad /* [num_channels, H, W] */,
                             float* d_attributes_grad /* [N, num_channels] row-major, fully written */);

/* ---- The surface of a view: a distance and an id per pixel (new functionality, the reference has none) ----
 * Every other form of the walk answers "how much"; gut_trace_surface answers "where".  Per pixel it chooses ONE of the Gaussians the
 * forward composited there and writes that Gaussian's hit distance along the ray (the hitT of the forward's distance plane, which
 * is the un-normalised mean sum w * hitT and lies between surfaces), its index and its blending weight w = T_before * alpha:
 *     GUT_SURFACE_LEVEL       the first, in the order of the tile's list, behind which the transmittance T is below `level`
 *                             (T counted after the Gaussian; level 0.5: the median distance).  Later Gaussians change nothing.
 *     GUT_SURFACE_MAX_WEIGHT  the one with the largest w; of equal weights the first in the order of the list.
 * A pixel in which nothing is chosen (nothing composited; in level mode, T never below the level) gets distance 0.0f, id
 * 0xFFFFFFFF and weight 0.0f.  Every element of the given planes is written, so they need no initialisation; d_id and d_weight may
 * be NULL and do not change d_distance.  The choice is made per pixel in the lane's registers while the walk passes: no reduction,
 * no atomics, identical inputs give identical bytes; the weight is the very w gut_trace_contribution takes the maximum of.  Scope,
 * walk and refusals are gut_trace_contribution's: it follows any forward on the same handle and stream, walks what that forward
 * walked by the forward's arithmetic, consumes nothing and may be followed by any backward or walk; unsorted variant at kernel
 * degree 2 only; refused after gut_optimize_rows_without_gradient.  One launch besides the tile order; with num_particles == 0 or a
 * forward without intersections the planes are filled with the no-hit values by memsets on the stream (0xFF bytes for d_id) and
 * nothing is walked.  Additionally refused, on the host before anything is queued: a mode that is neither of the two; in level mode
 * a level that is not finite or not inside (min_transmittance, 1) (the walk ends a ray below min_transmittance: a level there is
 * never crossed); d_distance NULL; a given plane not 4-byte aligned.  Render-only: nothing has a gradient.  Not part of the kernel
 * timers. */
enum { GUT_SURFACE_LEVEL = 0, GUT_SURFACE_MAX_WEIGHT = 1 };
int gut_trace_surface(gut_handle h, void* stream, uint32_t frame_number, int32_t num_active_features, uint32_t num_particles,
                      const float* d_particle_density /* NULL: the packed rows */, int32_t width, int32_t height,
                      const float* d_ray_origin, const float* d_ray_direction, const GutCamera* camera,
                      int32_t mode /* GUT_SURFACE_* */, float level /* GUT_SURFACE_LEVEL only */,
                      float* d_distance /* [H,W], fully written */, uint32_t* d_id /* [H,W] or NULL */, float* d_weight /* [H,W] or NULL */);

/* ---- Per-view exposure in the fused loss (new functionality, the reference has none) ----
 * gut_photometric_loss_exposure is the fused loss of gut_photometric_loss[_masked | _background] on the AFFINE image of a view:
 *     comp_k  = rgb_k + B_k (1 - alpha)                    B: `background` (d_background NULL) or the [H,W,3] plane d_background
 *     image_c = (sum_k A[c][k] comp_k + b_c) * mask        E = [A | b]: d_exposure12, a row-major 3x4 float array in DEVICE memory,
 *                                                          read by the kernels (no host copy, no synchronisation); identity [I | 0]
 * against gt * mask, counts as in the other forms.  With g_c = d loss / d image_c (mask factor included):
 *     d loss / d rgb_k = sum_c A[c][k] g_c,   d loss / d alpha = -sum_k B_k d loss / d rgb_k,
 *     d loss / d A[c][k] = sum_pixels g_c comp_k,   d loss / d b_c = sum_pixels g_c      -> d_exposure_grad12, laid out like E.
 * d_exposure_grad12 NULL: E is applied and nothing is reduced (one launch less).  The 12 sums are deterministic: a wave butterfly,
 * one row of partials per workgroup of 1024 pixels in the workspace, a final sum in double in a fixed order; no atomics.  Every
 * element of d_rgba_grad, d_loss3 and d_exposure_grad12 is written; a pixel whose mask is 0 gets four times 0.0f and adds nothing to
 * the sums.  The workspace is one of gut_photometric_exposure_workspace_bytes.  Launches: forward, backward, the per-pixel pass (for
 * every background, black included: the channels mix), the finish of the sums.  Returns 1 for a null pointer other than d_mask,
 * d_background and d_exposure_grad12 or an image of 10 pixels or less either way, 2 for a launch failure.
 * gut_exposure_adam_step: one Adam step on the 12 values of one view, in place: *d_count (the view's visit count) is advanced first
 * and gives the bias correction; d_m12 / d_v12 are the view's own moments; the betas are held in float32.  One launch. */
size_t gut_photometric_exposure_workspace_bytes(int32_t height, int32_t width);
int gut_photometric_loss_exposure(void* stream, int32_t height, int32_t width, const float* d_rgba, const float* d_gt_rgb,
                                  const float* d_mask        /* [H,W] or NULL */,
                                  const float* d_background  /* [H,W,3] or NULL: then `background` is the constant */,
                                  float background, const float* d_exposure12, float lambda_l1, float lambda_ssim,
                                  void* d_workspace, float* d_loss3, float* d_rgba_grad,
                                  float* d_exposure_grad12   /* NULL: E is applied, nothing is reduced */);
int gut_exposure_adam_step(void* stream, const float* d_grad12, float* d_exposure12, float* d_m12, float* d_v12,
                           int32_t* d_count, float lr, float beta1, float beta2, float eps);

/* ---- The fused loss by descriptor: the form new callers should use ----
 * One struct names everything the four positional forms above take; gut_photometric_loss_run is the function all four call, so
 * values, launches, workspace and stream behaviour are theirs.  An optional pointer that is NULL means "that operand is absent":
 *     d_mask NULL            no mask                                   (gut_photometric_loss_masked otherwise)
 *     d_background NULL      the constant `background`; non-NULL: the [H,W,3] plane, and `background` is not used
 *     d_exposure12 NULL      no exposure; non-NULL: d_workspace is one of gut_photometric_exposure_workspace_bytes (else
 *                            gut_photometric_workspace_bytes) and d_exposure_grad12 (may be NULL) receives d(loss)/dE
 * Returns 1 — on the host, nothing is launched — for a NULL descriptor, a NULL d_rgba, d_gt_rgb, d_workspace, d_loss3 or d_rgba_grad,
 * d_exposure_grad12 without d_exposure12, or height / width <= 10; 2 for a launch failure.  88 bytes: nine pointers, three floats. */
typedef struct GutPhotometricLoss {
    const float* d_rgba;          /* [H,W,4] */
    const float* d_gt_rgb;        /* [H,W,3] */
    const float* d_mask;          /* [H,W] or NULL */
    const float* d_background;    /* [H,W,3] or NULL */
    const float* d_exposure12;    /* E, row-major 3x4, or NULL */
    void* d_workspace;
    float* d_loss3;               /* receives {loss, L1, SSIM} */
    float* d_rgba_grad;           /* [H,W,4], receives d(loss)/d(rgba) */
    float* d_exposure_grad12;     /* receives d(loss)/dE, or NULL */
    float background, lambda_l1, lambda_ssim;
} GutPhotometricLoss;
int gut_photometric_loss_run(void* stream, int32_t height, int32_t width, const GutPhotometricLoss* loss);

/* ---- "next" row N3: MCMC relocation kernel (threedgrut/strategy/src/gaussian_mcmc.cu:33-73).
 * opacities [n], scales [n,3], ratios [n] (int32, 1..n_max), binoms [n_max,n_max] -> new_opacities [n], new_scales [n,3] */
int gut_mcmc_relocation(void* stream, int32_t n, const float* d_opacities, const float* d_scales, const int32_t* d_ratios,
                        const float* d_binoms, int32_t n_max, float* d_new_opacities, float* d_new_scales);

/* MCMCStrategy.perturb_gaussians (threedgrut/strategy/mcmc.py:147-164), which the reference's trainer runs after EVERY optimiser
 * step of an MCMC run (configs/strategy/mcmc.yaml: perturb.frequency 1): positions += Sigma @ (unit_normal * op_sigmoid(1 - density) *
 * noise_scale) on the raw [N,12] rows (pos3 | density logit | quat wxyz raw | log-scale3 | pad), Sigma = R S S^T R^T, noise_scale =
 * perturb.noise_lr * the current position learning rate.  d_act12 (may be NULL): the trainer's activated rows, whose positions are
 * updated too.  d_unit_normals (may be NULL): [N,3] standard-normal draws to use; NULL = Philox4x32-10 keyed by (seed, step) with the
 * row index as counter (the same draws on every rank).  One pass, 96 bytes per Gaussian, instead of four batched 3x3 matmuls. */
int gut_mcmc_perturb(void* stream, uint32_t num_particles, float* d_raw12, float* d_act12, float noise_scale, uint64_t seed,
                     uint64_t step, const float* d_unit_normals);

/* ---- The scene as a mesh: TSDF fusion of distance planes, surface nets (new functionality, the reference has none) ----
 * The volume is a dense axis-aligned box of X x Y x Z voxels of edge `voxel`; voxel (i, j, k) has its centre at
 * origin + voxel * (i + 1/2, j + 1/2, k + 1/2) and the linear index (k Y + j) X + i.  The state is the caller's: int32 d_acc and
 * uint32 d_cnt [Z,Y,X], optionally uint32 d_rgb_sum [Z,Y,X,3] and d_rgb_cnt [Z,Y,X] (both or neither); all zero = empty.
 *
 * gut_tsdf_integrate adds n_views (1 .. GUT_TSDF_MAX_VIEWS) views in ONE launch, one thread per voxel, the state words of a voxel
 * read once, held in registers over the views and stored once, only if a view updated the voxel.  Per view and voxel, in fp32
 * without contraction: the centre p goes to the sensor frame by the camera's world-to-sensor pose and through the camera model by the
 * projection kernel's arithmetic (pinhole without and with distortion, fisheye); an invalid projection or one outside the image skips
 * the view; the pixel is (floor(u), floor(v)); D = d_distance there, 0 or not finite skips; s = D - |p - o| with o the pixel's ray
 * origin in the sensor frame (d_ray_origin NULL: the sensor position); s < -truncation skips; else
 *     acc += rint(min(1, s / truncation) * 65536),  cnt += 1,
 * and, with colours on both sides and |s| <= truncation, rgb_sum += rint(255 * clamp(rgb, 0, 1)) per channel, rgb_cnt += 1.
 * Sums of integers: the state does not depend on the order of the views or on how they are split into calls; no atomics, a voxel
 * belongs to one thread.  The caller keeps the number of integrated views at or below 32767 (acc is an int32 of quanta).
 * Refused on the host, nothing written: a NULL grid / views / camera / d_acc / d_cnt / d_distance, a pointer not 4-byte aligned,
 * one of d_rgb_sum and d_rgb_cnt without the other, n_views outside 1 .. GUT_TSDF_MAX_VIEWS, voxel or truncation not finite and
 * positive, a dimension < 1 or X Y Z > 2^30, width or height < 1, an unknown camera model, and a rolling shutter in motion
 * (pose_start != pose_end).  Handle-free; everything is queued on `stream`. */
#define GUT_TSDF_MAX_VIEWS 8
typedef struct GutTsdfGrid {
    float origin[3];
    float voxel;
    int32_t dims[3];            /* X, Y, Z */
    float truncation;
    int32_t* d_acc;             /* [Z,Y,X] sum of rint(f * 65536) */
    uint32_t* d_cnt;            /* [Z,Y,X] views that updated the voxel */
    uint32_t* d_rgb_sum;        /* [Z,Y,X,3] or NULL */
    uint32_t* d_rgb_cnt;        /* [Z,Y,X] or NULL */
} GutTsdfGrid;
typedef struct GutTsdfView {
    const GutCamera* camera;    /* host */
    int32_t width, height;
    const float* d_distance;    /* [H,W], gut_trace_surface's level-mode plane: 0 = no surface */
    const float* d_rgba;        /* [H,W,4] of the forward, or NULL */
    const float* d_ray_origin;  /* [H,W,3] in the sensor frame, or NULL: the sensor position */
} GutTsdfView;
int gut_tsdf_integrate(void* stream, const GutTsdfGrid* grid, int32_t n_views, const GutTsdfView* views);

/* Surface nets on the integer state.  A lattice point is OBSERVED iff cnt >= min_count, INSIDE iff acc < 0; its value is
 * float(acc) / (float(cnt) * 65536).  Cell (i, j, k), i < X-1, j < Y-1, k < Z-1, has the corners (i + dx, j + dy, k + dz), corner
 * number dx + 2 dy + 4 dz; it is ACTIVE iff all eight are observed and not all on one side.  Its vertex is the mean of the crossings
 * t = f0 / (f0 - f1) of those of its twelve edges whose ends differ in side, summed in this order of (corner, corner):
 *     x: (0,1) (2,3) (4,5) (6,7)   y: (0,2) (1,3) (4,6) (5,7)   z: (0,4) (1,5) (2,6) (3,7)
 * at origin + voxel * ((i, j, k) + 1/2 + mean); its colour the mean of rgb_sum / (255 rgb_cnt) over the corners with rgb_cnt > 0,
 * grey 0.5 without any.  Vertices are ordered by the cell's linear index.  A lattice edge p -> p + e_a (a = x, y, z) whose ends are
 * observed and differ in side emits one quad if its four surrounding cells lie in the grid and are fully observed: with (a, b, c) a
 * cyclic permutation of (x, y, z), the cells p - e_b - e_c, p - e_c, p, p - e_b in this order if p is inside, in the reverse
 * order starting from the same cell otherwise (the normal points from inside to outside), split into the triangles (0,1,2), (0,2,3).
 * Quads are ordered by the linear index of p, then by axis.
 *   gut_surface_nets_count: d_cell [Z,Y,X] bytes (bit 0: the cell exists and is fully observed, bit 1: active), d_quads [Z,Y,X]
 *     bytes (the lattice point's number of quads, 0 .. 3).  Two launches.
 *   gut_surface_nets_emit:  with the EXCLUSIVE prefix sums of (d_cell >> 1) and of d_quads as int32 [Z,Y,X] (the caller scans),
 *     writes d_vertices / d_colours [V,3] and d_faces int32 [2 Q,3].  One launch.
 * Refusals as above (grid, min_count < 1, NULL or misaligned pointers); the colour arrays of the grid may be NULL. */
int gut_surface_nets_count(void* stream, const GutTsdfGrid* grid, uint32_t min_count, uint8_t* d_cell, uint8_t* d_quads);
int gut_surface_nets_emit(void* stream, const GutTsdfGrid* grid, uint32_t min_count, const uint8_t* d_cell, const uint8_t* d_quads,
                          const int32_t* d_vertex_offset, const int32_t* d_quad_offset, float* d_vertices, float* d_colours,
                          int32_t* d_faces);

/* ---- A learnt radiance at infinity: a cube-map background (new functionality, the reference has none) ----
 * The map is d_texels [6, R, R, 3] float32, plain RGB, indexed [face, row, column, channel].  For pixel p with the camera-space
 * direction d = d_ray_direction[p] and the camera-to-world rotation M (row-major, the nine floats the compositors apply to a ray), in
 * fp32 without contraction:
 *     e_i = (M[i][0] d0 + M[i][1] d1) + M[i][2] d2;   a_i = |e_i|
 *     axis = 0 if a0 >= a1 && a0 >= a2, else 1 if a1 >= a2, else 2;   m = a_axis;   face = 2 axis + (e_axis < 0)
 *     u = e_(axis+1)%3 / m,  v = e_(axis+2)%3 / m           (no sign flips)
 *     s = (u + 1) (0.5 R) - 0.5,  i0 = floor(s),  fx = s - i0;   t, j0, fy likewise from v
 *     columns clamp(i0, 0, R-1), clamp(i0+1, 0, R-1); rows likewise from j0 (clamped to the edge WITHIN the face)
 *     w00 = (1-fx)(1-fy), w10 = fx (1-fy), w01 = (1-fx) fy, w11 = fx fy    (w_ab: column a, row b)
 *     B(p)_k = ((w00 T00_k + w10 T10_k) + w01 T01_k) + w11 T11_k
 * A pixel with m == 0 or a non-finite e_i is VOID: its plane value is +0 and it scatters nothing.
 * gut_environment_sample writes the [H,W,3] plane in full, one launch.
 * gut_environment_backward is the adjoint grad[texel, k] = sum_p w(p, texel) c(p)_k of a cotangent c, given either as the plane
 * d_plane_grad [H,W,3] or as the pair d_rgba / d_rgba_grad [H,W,4] of the fused loss, from which c_k = (1 - alpha) g_k is formed
 * (1 - alpha rounded first, then each product).  Exactly one of the two forms is set.  A non-finite c counts as 0.  Every product
 * w c_k is rounded to fp32 on its own, multiplied by 2^s (exact), rounded to nearest even to an integer and added with integer
 * atomics: identical inputs give identical bits.  s comes from the largest finite |c| of the call, |c| < 2^e: s = 40 - e, less
 * ceil(log2(H W)) - 22 for more than 2^22 pixels, clamped to -126 .. 126, 0 for a zero cotangent; one s for the three channels.
 * Every element of d_texel_grad is written as float(sum) 2^-s.  Products below the normal fp32 range are outside the contract.
 * Queued on `stream`, nothing read back: one memset of the workspace (gut_environment_workspace_bytes, 0 for a resolution that is
 * refused), the maximum, the scatter (a 16x16 pixel tile per workgroup, summed in an LDS table of GUT_ENVIRONMENT_SLOTS texels, one
 * 64-bit atomic per occupied slot and channel; a contribution that finds no slot adds to the workspace directly), the conversion.
 * Return 1, on the host, nothing queued: a NULL pointer, resolution < 1 or > GUT_ENVIRONMENT_MAX_RESOLUTION (18 R^2 stays below
 * 2^31), height or width < 1, more than 2^30 pixels, both or neither cotangent form; a HIP error is reported the same way.  gut_last_error says which.
 * gut_environment_rotation (host only): M of a camera, the sensor-to-world rotation at the middle of its two poses exactly as the
 * trace calls build it. */
#define GUT_ENVIRONMENT_SLOTS 128
#define GUT_ENVIRONMENT_MAX_RESOLUTION 8192
typedef struct GutEnvironmentView {
    const float* d_ray_direction;   /* [H,W,3] */
    float rotation[9];              /* M, row-major */
    int32_t height, width;
} GutEnvironmentView;
typedef struct GutEnvironmentCotangent {
    const float* d_plane_grad;      /* [H,W,3], or NULL */
    const float* d_rgba;            /* [H,W,4], or NULL; with d_rgba_grad */
    const float* d_rgba_grad;       /* [H,W,4], or NULL */
} GutEnvironmentCotangent;
int gut_environment_sample(void* stream, const GutEnvironmentView* view, const float* d_texels, int32_t resolution, float* d_plane_out);
size_t gut_environment_workspace_bytes(int32_t resolution);
int gut_environment_backward(void* stream, const GutEnvironmentView* view, const GutEnvironmentCotangent* cotangent, int32_t resolution,
                             void* d_workspace, float* d_texel_grad);
int gut_environment_rotation(const GutCamera* camera, float* rotation9);

/* ---- Per-view bilateral grids of affine colour transforms (new functionality, the reference has none) ----
 * A view's grid is d_grid [12, L, Gh, Gw] float32 (levels, rows, columns); channel 4 i + j is entry [i][j] of a 3x4 transform.  For
 * pixel (x, y), in fp32 without contraction and in this order:
 *     comp_k = rgb_k + B_k (1 - alpha)          B: `background` (d_background NULL) or the [H,W,3] plane d_background
 *     g = (0.299 comp_0 + 0.587 comp_1) + 0.114 comp_2;  gc = min(max(g, 0), 1), a NaN g as 0;  inside = 0 < g < 1
 *     sx = x ((Gw-1)/(W-1)), sy = y ((Gh-1)/(H-1)) (scales formed once, on the host, 0 for an axis of one pixel), sz = gc (L-1)
 *     i0 = floor(s), f = s - i0, indices i0 and min(i0+1, n-1), weights 1-f and f per axis;  w_abc = (wa wb) wc, x fastest
 *     A_k = sum over the eight taps in order of w_n G[k, tap_n];   out_i = ((A_i0 comp_0 + A_i1 comp_1) + A_i2 comp_2) + A_i3
 * gut_bilateral_slice writes rgba' = (out, alpha) in full, one launch.
 * gut_bilateral_backward takes d_rgba_out_grad [H,W,4], the gradient a loss wrote for rgba' (g' = its rgb part, a non-finite value as
 * 0), and writes d_rgba_grad [H,W,4] and d_grid_grad [12, L, Gh, Gw], every element of both:
 *     grid_grad[4i+j, tap_n] = sum_pixels w_n (g'_i c4_j), c4 = (comp, 1): each product rounded to fp32 on its own (a non-finite
 *         g'_i c4_j as 0), times 2^s (exact), to nearest even, integer adds only: identical inputs give identical bits.  s is
 *         gut_environment_backward's with the magnitude m = max_pixels max_i |g'_i| max(1, max_j |comp_j|) over the finite comp_j.
 *     d comp_j = ((A_0j g'_0 + A_1j g'_1) + A_2j g'_2) [+ (lum_j (L-1)) D if inside],  lum = (0.299, 0.587, 0.114),
 *         D = (g'_0 d_0 + g'_1 d_1) + g'_2 d_2,  d_i = ((dA_i0 comp_0 + dA_i1 comp_1) + dA_i2 comp_2) + dA_i3,
 *         dA_k = sum over the xy taps in order of (wa wb) (G[k, z1] - G[k, z0])
 *     rgba_grad.rgb = d comp;  rgba_grad.a = -((B_0 d comp_0 + B_1 d comp_1) + B_2 d comp_2) + rgba_out_grad.a
 *     lambda_tv != 0: grid_grad += lambda_tv dTV/dG, TV = sum_axes (1 / n_axis) sum_pairs (G[next] - G[cur])^2, n_axis = 12 pairs:
 *         acc = 0; per axis x, y, z of length > 1: acc = acc + (2 / n_axis) (a - b), a = G[c] - G[previous] (0 at the first
 *         index), b = G[next] - G[c] (0 at the last); grad = grad + lambda_tv acc.  lambda_tv == 0 adds nothing.
 * Queued on `stream`, nothing read back: one memset of the workspace (gut_bilateral_workspace_bytes, 0 for dimensions that are
 * refused), the maximum, the adjoint (a 16x16 pixel tile per workgroup, summed in a direct-indexed LDS table of GUT_BILATERAL_TABLE
 * 64-bit sums over the tile's footprint in the grid, one 64-bit atomic per non-zero sum; a tile whose footprint exceeds the table
 * adds to the workspace directly), the conversion with the TV term.
 * gut_bilateral_backward_image writes d_rgba_grad alone, the same bits, in one launch: no maximum, no sums, no atomics and no
 * workspace (a step outside the grids' iteration window: the image gradient has to pass through the slice, the grid learns nothing).
 * gut_bilateral_adam_step: one Adam step on the n = 12 L Gh Gw floats of one view, in place, gut_exposure_adam_step's arithmetic:
 * *d_count (the view's visit count, below 2^20) is advanced once and gives the bias correction.  One launch.
 * Return 1, on the host, nothing queued: a NULL pointer other than d_background, a dimension outside 1 .. GUT_BILATERAL_MAX_DIM,
 * height or width < 1, more than 2^30 pixels, a non-finite lambda_tv, an image pointer that is not 16-byte aligned or a workspace
 * that is not 8-byte aligned, n outside 1 .. 12 GUT_BILATERAL_MAX_DIM^3; a HIP error is reported the same way.  gut_last_error says
 * which. */
#define GUT_BILATERAL_MAX_DIM 256
#define GUT_BILATERAL_TABLE 1024
typedef struct GutBilateralGrid {
    float* d_grid;                  /* [12, levels, rows, columns] */
    int32_t levels, rows, columns;
} GutBilateralGrid;
size_t gut_bilateral_workspace_bytes(int32_t levels, int32_t rows, int32_t columns);
int gut_bilateral_slice(void* stream, int32_t height, int32_t width, const float* d_rgba,
                        const float* d_background  /* [H,W,3] or NULL: then `background` is the constant */,
                        float background, const GutBilateralGrid* grid, float* d_rgba_out);
int gut_bilateral_backward(void* stream, int32_t height, int32_t width, const float* d_rgba, const float* d_background, float background,
                           const GutBilateralGrid* grid, const float* d_rgba_out_grad, float lambda_tv, void* d_workspace,
                           float* d_rgba_grad, float* d_grid_grad);
int gut_bilateral_backward_image(void* stream, int32_t height, int32_t width, const float* d_rgba, const float* d_background,
                                 float background, const GutBilateralGrid* grid, const float* d_rgba_out_grad, float* d_rgba_grad);
int gut_bilateral_adam_step(void* stream, const float* d_grad, float* d_grid, float* d_m, float* d_v, int32_t* d_count, int64_t n,
                            float lr, float beta1, float beta2, float eps);

const char* gut_last_error(void);
int gut_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GUT_HIP_H */
