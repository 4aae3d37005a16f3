// gut_internal.h — types shared by the HIP translation units of libgut_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gut_hip.h"

namespace gut {

constexpr int kTile = 16;                 // GUTParameters::Tiling::BlockX/Y  (gutRendererParameters.h:22-31)
constexpr int kBlock = 256;
constexpr uint32_t kInvalid = 0xFFFFFFFFu;

// 3x4 affine transform, row-major: y = R x + t
struct Affine {
    float r[3][3];
    float t[3];
};
__device__ __forceinline__ void affine_point(const Affine& a, float wx, float wy, float wz, float& cx, float& cy, float& cz) {
    cx = a.r[0][0] * wx + a.r[0][1] * wy + a.r[0][2] * wz + a.t[0];
    cy = a.r[1][0] * wx + a.r[1][1] * wy + a.r[1][2] * wz + a.t[1];
    cz = a.r[2][0] * wx + a.r[2][1] * wy + a.r[2][2] * wz + a.t[2];
}

// rows of rotationT from a wxyz quaternion (slang/common/transforms.slang:22-39); forced inline, so every unit compiles it under
// its own contraction flags
__device__ __forceinline__ void quat_rows(float w, float x, float y, float z, float r[3][3]) {
    const float xx = x * x, yy = y * y, zz = z * z;
    const float xy = x * y, xz = x * z, yz = y * z;
    const float rx = w * x, ry = w * y, rz = w * z;
    r[0][0] = 1.0f - 2.0f * (yy + zz); r[0][1] = 2.0f * (xy + rz); r[0][2] = 2.0f * (xz - ry);
    r[1][0] = 2.0f * (xy - rz); r[1][1] = 1.0f - 2.0f * (xx + zz); r[1][2] = 2.0f * (yz + rx);
    r[2][0] = 2.0f * (xz + ry); r[2][1] = 2.0f * (yz - rx); r[2][2] = 1.0f - 2.0f * (xx + yy);
}

// Everything the device code needs to know about the view; built on the host (gut_api.cpp).
struct ViewParams {
    Affine w2s_end;     // world->sensor at the end pose (rolling-shutter fallback, cameraProjections.cuh:162-170)
    float pose_start[7], pose_end[7];  // t(3), q(x,y,z,w): interpolated per sigma point for rolling shutters
    int32_t shutter;
    Affine w2s_start;   // world->sensor at the start pose: projects the sigma points (cameraProjections.cuh:154-157)
    Affine w2s_mid;     // world->sensor at the interpolated mid pose: depth key (gutProjector.cuh:137,317)
    Affine s2w;         // sensor->world: ray transform; s2w.t is the sensor position in world space
    int32_t model;
    int32_t width, height;
    int32_t grid_x, grid_y;
    float principal_point[2];
    float focal_length[2];
    float radial[6];
    float tangential[2];
    float thin_prism[4];
    float max_angle;
    int32_t shutter_iterations;   // GAUSSIAN_N_ROLLING_SHUTTER_ITERATIONS (threedgut.cuh:63), rolling shutters only
};

// Derived render constants (host-computed in fp32 with the same operation order as the oracle).
struct RenderConsts {
    float alpha_threshold, max_alpha, min_response, min_transmittance;
    float min_sensor_z, cov_dilation;
    float ut_delta, ut_w0_mean, ut_wi, ut_w0_cov, ut_margin;
    int32_t rect_bounding, tight_opacity_bounding, tile_culling, global_z_order;
    float max_d2;   // -2 ln(min_response): d2 above this can never be accepted (kernel degree 2; kernel_cutoff_d2 otherwise)
};

// largest d2 at which the kernel's response still reaches r (0 < r < 1), without safety margin
__host__ __device__ inline float kernel_cutoff_d2(int degree, float r) {
    float s, n;
    switch (degree) {
    case 8: s = 0.000685871056241f; n = 8.0f; break;
    case 5: s = 0.0185185185185f; n = 5.0f; break;
    case 4: s = 0.0555555555556f; n = 4.0f; break;
    case 3: s = 0.166666666667f; n = 3.0f; break;
    case 1: s = 1.5f; n = 1.0f; break;
    case 0: { const float t = (1.0f - r) / 0.329630334487f; return t * t; }
    default: return -2.0f * logf(r);
    }
    return powf(-logf(r) / s, 2.0f / n);
}

// device-side counters (one 64-byte line)
struct Counters {
    unsigned long long visible;        // V
    unsigned long long traversed_fwd;  // E_f
    unsigned long long traversed_bwd;  // E_b
    unsigned long long side_stream_rows;
    unsigned long long side_stream_rows_first;
    unsigned long long pad[3];
};

// Lazy moment decay of the fused optimiser kernels (GutLazyMoments of the C ABI + the step being applied).  A 64-row wave that
// cannot receive a gradient in a step — no row has a tile, or the forward walked none of its Gaussians — gets its parameter
// update from m, v READ but NOT WRITTEN BACK: wave_step[w] remembers up to which step the stored moments are current, and
// whoever reads them next first multiplies by beta^(steps missed) from a host-made table (pow1[k] = fl(beta1^k), pow1[0] = 1).
// Saves 472 of the 1488 bytes per row of the zero-gradient update.  wave_step == nullptr: every update writes its moments.
struct LazyMoments {
    uint32_t* wave_step = nullptr;
    const float* pow1 = nullptr;
    const float* pow2 = nullptr;
    uint32_t len = 0;
    uint32_t t = 0;     // the optimiser step being applied (1-based)
    uint32_t* overrun = nullptr;   // GutLazyMoments.d_overrun
};

// The MCMC recipe's opacity / scale regularisers (GutRegularisation of the C ABI, configs/base_mcmc.yaml:13-18):
//     dL/d(density logit) = density_coeff * sigmoid(d) (1 - sigmoid(d)),   dL/d(log-scale k) = scale_coeff * exp(s_k)
// on the pre-update row, added to the row's photometric gradient (after any 1/world scaling) by whichever kernel updates the row.
// With a regulariser no row is gradient-free in the [N,12] block: its moments are stored every step (eager), while the [N,48]
// block keeps the lazy decay.  partials[w] = (sum of sigmoid(d), sum of exp(s_0) + exp(s_1) + exp(s_2)) over the rows of 64-row
// wave w, written by the kernel that owns the wave (gut_regularisation_loss reduces them).
struct Regularisation {
    float density_coeff = 0.0f;   // lambda_opacity / N
    float scale_coeff = 0.0f;     // lambda_scale / (3 N)
    float2* partials = nullptr;   // [ceil(N / 64)] or null
    __host__ __device__ bool on() const { return density_coeff != 0.0f || scale_coeff != 0.0f; }
};

// ---- what the fused optimiser's host code hands from the ABI boundary down to the launches (host side only) ----
// the seven device tensors of the optimiser's state; act12 receives the activated rows of the updated parameters (or null)
struct OptimiserState {
    float *raw12 = nullptr, *raw_m = nullptr, *raw_v = nullptr;   // [N,12] parameters and their two moments
    float *sh48 = nullptr, *sh_m = nullptr, *sh_v = nullptr;      // [N,48]
    float* act12 = nullptr;
};
// Adam's settings for one step; the learning rates by value, so that a stored copy outlives the caller's arrays
struct AdamSettings {
    float lr12[12], lr48[48];
    float beta1, beta2, eps;
    uint32_t step;   // 1-based; 0 = no bias correction
};
inline AdamSettings make_adam_settings(const float* lr12, const float* lr48, float beta1, float beta2, float eps, uint32_t step) {
    AdamSettings a;
    for (int i = 0; i < 12; ++i) a.lr12[i] = lr12[i];
    for (int i = 0; i < 48; ++i) a.lr48[i] = lr48[i];
    a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.step = step;
    return a;
}
// one launch of the side-stream pass (k_adam_rows_without_gradient): its 256-row blocks and which of their waves it owns
struct SideStreamBlocks {
    uint32_t block_begin = 0, block_end = 0;
    const uint8_t* wave_walked = nullptr;   // per-wave marks of the forward's walk, or null
    uint32_t split_block = 0;               // first block of the second launch's share of the waves without tiles
    uint32_t extra_end = 0;                 // blocks < extra_end: unwalked waves with tiles also go to the second launch
    bool second_launch = false;
};
// the handle's rows the single-view optimiser reads: the sensor position [3], the gradient rows the backward compositor left
// (zeroed as they are read), the tile counts and the per-Gaussian features of the cached forward
struct ScratchGradients {
    const float* camera_position = nullptr;
    float* grad16 = nullptr;
    const uint32_t* tiles_count = nullptr;
    const float* feat = nullptr;
};
// gs.py:106-115 statistics accumulated by the optimiser kernel (gut_set_position_gradient_statistics), or null
struct PositionStatistics {
    float* accum = nullptr;
    int32_t* denom = nullptr;
};

// what K1 zeroes on its way (the frame's small clears): ranges [tiles] uint2, trav_bwd [tiles], wave_walked [4 * blocks] bytes (or null)
struct FrameClears {
    uint2* ranges = nullptr;
    uint32_t* trav_bwd = nullptr;
    uint8_t* wave_walked = nullptr;
    uint32_t tiles = 0;
    float* cam_pos = nullptr;   // [3]: K1 also leaves the sensor position (ViewParams.s2w.t) on the device
    uint32_t* tile_entries = nullptr;   // [tiles], zero on entry: K1 adds every tile's entry count (grouped binning), or null
};

// ---- launch wrappers implemented in the .hip files -------------------------------------------------
void launch_project(hipStream_t s, const ViewParams& v, const RenderConsts& c, uint32_t n, int sh_degree,
                    const float* density12, const float* sph48, uint32_t* tiles_count, float* proj_pos,
                    float* conic_opacity, float* extent, float* depth, float* feat, float* visibility,
                    uint32_t* wave_sums /* [4 * blocks]: tile count of every 64-row wave (first level of the scan) */, const float* sph_albedo /* non-null: sph48 is features_specular [N,45], this is features_albedo [N,3] */,
                    const FrameClears& clears);
// second level of the scan of the tile counts: block_prefix[b] = list entries of the Gaussians before 256-row block b, *total = M
// tile_entries (K1's per-tile counts, or null; left zero): tile_start [tiles + 1] = their exclusive scan (tile_start[tiles] = M), tile_cursor
// [tiles] = the same
void launch_scan_wave_sums(hipStream_t s, uint32_t n, const uint32_t* wave_sums, uint32_t* block_prefix, uint32_t* total,
                           uint32_t* host_out /* device view of pinned host words, or null */, const uint32_t* walk_sums /* or null */,
                           uint32_t* tile_entries, uint32_t tiles, uint32_t* tile_start, uint32_t* tile_cursor);
// lazy order's binning (replaces K3 + sort + K5): entries[tile_start[t] ..] := {depth bits, particle id} of tile t's entries, in no
// particular order; ranges := the tiles' slices clamped to capacity ((0, 0) for empty tiles); slots >= capacity are dropped
void launch_expand_grouped(hipStream_t s, const ViewParams& v, const RenderConsts& c, uint32_t n, const float* proj_pos,
                           const float* conic_opacity, const float* extent, const float* depth, uint32_t tiles,
                           const uint32_t* tile_start, uint32_t* tile_cursor, uint32_t* ranges, uint64_t* entries, uint32_t capacity);
void launch_expand(hipStream_t s, const ViewParams& v, const RenderConsts& c, uint32_t n, const uint32_t* tiles_count,
                   const uint32_t* wave_sums, const uint32_t* block_prefix, const uint32_t* total /* device word: M; the tail
                   [M, capacity) of keys / ids is padded here */, const float* proj_pos, const float* conic_opacity, const float* extent, const float* depth,
                   uint64_t* keys, uint32_t* ids, uint32_t capacity);
void launch_pad_keys(hipStream_t s, const uint32_t* count, uint32_t sort_n, uint64_t* keys, uint32_t* ids);
// debug view only: ordered_ids[range.x + tile_ordered[t] .. range.y) := padding id for every tile t
void launch_mask_unordered(hipStream_t s, uint32_t tiles, const uint32_t* ranges, const uint32_t* tile_ordered, uint32_t* ordered_ids);
void launch_tile_ranges(hipStream_t s, uint32_t m, const uint64_t* sorted_keys, uint32_t* ranges);
// K8 output as the four tensors of the reference's _Autograd.backward instead of one [N,12] tensor (pos == nullptr: [N,12])
struct GradFields {
    float* pos = nullptr;   // [N,3]
    float* dns = nullptr;   // [N,1]
    float* rot = nullptr;   // [N,4] (16-byte aligned)
    float* scl = nullptr;   // [N,3]
    float* alb = nullptr;   // [N,3]  } with spec: the SH gradient as the model's two feature tensors instead of [N,48]
    float* spec = nullptr;  // [N,45] } (16-byte aligned)
};
void launch_project_bwd(hipStream_t s, const ViewParams& v, uint32_t n, int sh_degree, const float* density12,
                        const uint32_t* tiles_count, const float* feat, float* grad16 /* rows read are left zero */,
                        float* density_grad12, float* sph_grad48, bool raw_grads, const GradFields& fields = GradFields());
void launch_pack_fields(hipStream_t s, uint32_t n, const float* pos, const float* dns, const float* rot, const float* scl,
                        float* density12);
// out[row][c] = c < in_width ? in[row][c] : 0 for c < out_width: widens [N, 3 (d+1)^2] radiance rows to the kernels' 48 columns and
// narrows the [N,48] gradient back (render.particle_radiance_sph_degree < 3)
void launch_resize_sph_rows(hipStream_t s, uint32_t n, uint32_t in_width, uint32_t out_width, const float* in, float* out);
void launch_pack_activate_fields(hipStream_t s, uint32_t n, const float* pos, const float* dns_logit, const float* rot_raw,
                                 const float* log_scl, float* act12);   // gut_train.hip (activate_row)

// ---- the compositors (gut_render.hip, gut_render_general.hip, gut_render_sorted.hip) and the walk (gut_contrib.hip) ----
// What every compositor launch reads, built once per call (gut_api.cpp); host side only, the kernels take its fields as arguments
struct CompositorOperands {
    const ViewParams& v;
    const RenderConsts& c;
    const float* density12;    // [N,12] rows
    const float* feat;         // [N,3] per-Gaussian colours of the cached forward
    const float* ray_ori;
    const float* ray_dir;
    const uint32_t* ranges;    // [tiles] uint2: each tile's slice of the id list
    const uint32_t* ids;       // the depth-ordered id list (forward with the lazy order: unused, see LazyOrderLists)
    int kernel_degree;         // render.particle_kernel_degree; != 2 runs the kGeneral instantiations
};
struct RenderImages { float *rgba, *dist, *hits; };   // the forward's three planes
// lazy order only (all null: the id list is fully sorted): the tiles' {depth bits, particle id} words, grouped by tile, in; the ids
// in the order the forward consumed them and the number of each tile's entries it ordered, out
struct LazyOrderLists {
    const uint64_t* tile_keys = nullptr;
    uint32_t* ordered_ids = nullptr;
    uint32_t* tile_ordered = nullptr;
};
// the forward's planes and the loss's gradients with respect to them; hit_distance: read by the sorted variant only
struct BwdUpstream { const float *rgba, *rgba_grad, *hit_distance, *hit_distance_grad /* may be NULL (= all zeros) */; };

// tile_order: launch order of the tiles (longest lists first) or null
void launch_render(hipStream_t s, const CompositorOperands& o, const uint32_t* d_num_intersections, const RenderImages& out,
                   uint32_t* tile_traversed, const LazyOrderLists& lazy, const uint32_t* tile_order);
// tile_walked: the forward's per-tile traversal depth, the backward stops there
void launch_render_bwd(hipStream_t s, const CompositorOperands& o, const BwdUpstream& up, float* grad16, uint32_t* tile_traversed,
                       const uint32_t* tile_order, const uint32_t* tile_walked);
// the same two launches for render.particle_kernel_degree != 2 (gut_render_general.hip; reached through launch_render / launch_render_bwd)
decltype(launch_render) launch_render_general;
decltype(launch_render_bwd) launch_render_bwd_general;
void launch_tile_order(hipStream_t s, uint32_t tiles, const uint32_t* traversed, uint32_t* order, const uint32_t* ranges = nullptr,
                       bool by_length = false, uint32_t* walk_sums = nullptr);
// gut_contrib.hip: the forward's walk again (unsorted variant, kernel degree 2), without colours.  What every form of
// the walk reads, built once per call from the compositors' record (walk_operands) and passed to the kernel by value
struct WalkOperands {
    ViewParams v;
    RenderConsts c;
    const float* density12;
    const float* ray_ori;
    const float* ray_dir;
    const uint32_t* ranges;
    const uint32_t* ordered_ids;   // the list the backward compositor reads
    const uint32_t* tile_order;    // a launch order of all the tiles (required)
    const uint32_t* tile_walked;   // the forward's per-tile traversal depth
    uint32_t num_particles;
    uint32_t tiles;                // v.grid_x * v.grid_y: one workgroup each
};
inline WalkOperands walk_operands(const CompositorOperands& o, const uint32_t* tile_order, const uint32_t* tile_walked, uint32_t num_particles) {
    return WalkOperands{o.v, o.c, o.density12, o.ray_ori, o.ray_dir, o.ranges, o.ids, tile_order, tile_walked, num_particles,
                        (uint32_t)(o.v.grid_x * o.v.grid_y)};
}
// adds every walked Gaussian's sum and maximum of blending weights and its composited-pixel count to scores [N] (integer atomics).
// plane [H,W] (null: the records alone): every weight is also multiplied by the pixel's value clamped to [0, 1] and summed into
// weighted_q32 [N]; with a plane, scores may be null (the weighted sums alone)
void launch_contribution(hipStream_t s, const WalkOperands& o, GutContribution* scores, const float* plane = nullptr,
                         uint64_t* weighted_q32 = nullptr);
// the same walk rendering per-Gaussian attributes: attrs [N, num_channels] row-major -> out [num_channels, H, W], every
// element written; one launch per group of four channels
void launch_attributes(hipStream_t s, const WalkOperands& o, uint32_t num_channels, const float* attrs, float* out);
// the adjoint of launch_attributes: out_grad [num_channels, H, W] -> attrs_grad [N, num_channels] row-major, every
// element written; per group of four channels the planes' maxima, one walk and one pass over the rows.  rows_q: scratch of
// 32 bytes per particle; max_bits: scratch of four words
void launch_attributes_bwd(hipStream_t s, const WalkOperands& o, uint32_t num_channels, const float* out_grad, float* attrs_grad,
                           void* rows_q, uint32_t* max_bits);
// the same walk choosing one composited entry per pixel: mode GUT_SURFACE_LEVEL (the first entry behind which the
// transmittance is below `level`) or GUT_SURFACE_MAX_WEIGHT; its hit distance, id and weight to [H,W] planes, every element written
// (0.0f, 0xFFFFFFFF, 0.0f where nothing was chosen); id and weight may be null
void launch_surface(hipStream_t s, const WalkOperands& o, int mode, float level, float* distance, uint32_t* id, float* weight);
// sorted (k_buffer_size = K > 0) compositor variant, gut_render_sorted.hip
void launch_render_sorted(hipStream_t s, const CompositorOperands& o, int K, const uint32_t* d_num_intersections, const RenderImages& out);
void launch_render_sorted_bwd(hipStream_t s, const CompositorOperands& o, int K, const BwdUpstream& up, float* grad16, bool reference_undo);
void launch_project_bwd_compact(hipStream_t s, uint32_t n, const float* density12, const uint32_t* tiles_count,
                                const float* feat, float* grad16 /* rows read are left zero */, float* raw_grad12, float* mrgb);
// fused per-Gaussian backward epilogue + SH-gradient + Adam (gut_train.hip), single view, reads the handle's gradient rows
void launch_sh_adam_from_scratch(hipStream_t s, uint32_t n, int sh_degree, const ScratchGradients& grads, const OptimiserState& state,
                                 const AdamSettings& adam, const float* visibility,
                                 const SideStreamBlocks* early /* the side stream's second launch if it took waves of this step, or null */,
                                 const LazyMoments& lazy, const uint8_t* rule_walked /* per-wave marks valid for EVERY wave, or null */,
                                 const PositionStatistics& stats = PositionStatistics(), const Regularisation& reg = Regularisation());
void launch_compact_gradient_rows(hipStream_t s, uint32_t n, const float* act12, const uint32_t* tiles_count, const float* feat,
                                  float* grad16, float* records, uint32_t capacity, uint32_t* count);
// Adam step of the rows that get no gradient this iteration (tiles_count == 0), see k_adam_rows_without_gradient
void launch_adam_rows_without_gradient(hipStream_t s, uint32_t n, const uint32_t* tiles_count, const OptimiserState& state,
                                       const AdamSettings& adam, const SideStreamBlocks& blocks, const LazyMoments& lazy,
                                       const Regularisation& reg = Regularisation());
void launch_count_side_stream_rows(hipStream_t s, uint32_t n, const uint32_t* tiles_count, const uint8_t* wave_walked,
                                   uint32_t split_block, uint32_t extra_end, Counters* out);
void launch_mark_waves_with_tiles(hipStream_t s, uint32_t n, const uint32_t* tiles_count, uint8_t* wave_flags);
void launch_mark_walked_waves(hipStream_t s, uint32_t n, uint32_t tiles, const uint32_t* ranges, const uint32_t* tile_walked,
                              const uint32_t* ids, uint8_t* wave_walked);
void launch_stats_reduce(hipStream_t s, uint32_t n, const uint32_t* tiles_count, uint32_t t, const uint32_t* trav_fwd,
                         const uint32_t* trav_bwd, Counters* out);
// gut_pose.hip: out8 := {F, M, rows with a tile, 0}, the pose-gradient reduction of the gradient rows K7 left (read only; rows with
// tiles_count != 0), around the sensor position cam_pos [3]; partials: pose_gradient_scratch_bytes() of scratch.  Two launches.
size_t pose_gradient_scratch_bytes();
void launch_pose_gradient(hipStream_t s, uint32_t n, const uint32_t* tiles_count, const float* grad16, const float* density12,
                          const float* cam_pos, float* partials, float* out8);
// the consuming form (gut_trace_bwd_pose): the same numbers, and every row with a tile is left as 64 zero bytes.  test_before_store:
// read the whole row and store only where a word is set (what the library launches); false: four unconditional zero stores per
// visited row (kept for measurements)
void launch_pose_gradient_consume(hipStream_t s, uint32_t n, const uint32_t* tiles_count, float* grad16, const float* density12,
                                  const float* cam_pos, float* partials, float* out8, bool test_before_store);
void launch_pose_adam(hipStream_t s, const float* grad8, float* m6, float* v6, int32_t* count, float lr_translation, float lr_rotation,
                      float beta1, float beta2, float eps, float* delta6);

// gut_fuse.hip: TSDF fusion of distance planes into the caller's integer volume, surface nets on it.  The records
// are built and checked on the host (gut_api.cpp) and travel as kernel arguments.
struct FuseGrid {
    float origin[3];
    float voxel;
    int32_t X, Y, Z;
    float truncation;
    int32_t* acc;
    uint32_t* cnt;
    uint32_t* rgb_sum;   // [Z,Y,X,3] or null
    uint32_t* rgb_cnt;   // null with rgb_sum
};
struct FuseView {
    Affine w2s;          // world->sensor (pose_start == pose_end)
    int32_t variant;     // K1's: 0 pinhole without distortion, 1 pinhole with, 2 fisheye
    int32_t width, height;
    float principal_point[2];
    float focal_length[2];
    float radial[6];
    float tangential[2];
    float thin_prism[4];
    float max_angle;
    const float* distance;   // [H,W]
    const float* rgba;       // [H,W,4] or null
    const float* origin;     // [H,W,3], sensor frame, or null
};
struct FuseViews {
    FuseView v[GUT_TSDF_MAX_VIEWS];
};
void launch_tsdf_integrate(hipStream_t s, const FuseGrid& g, int n_views, const FuseViews& views);
void launch_surface_nets_count(hipStream_t s, const FuseGrid& g, uint32_t min_count, uint8_t* cell, uint8_t* quads);
void launch_surface_nets_emit(hipStream_t s, const FuseGrid& g, uint32_t min_count, const uint8_t* cell, const uint8_t* quads,
                              const int32_t* vertex_offset, const int32_t* quad_offset, float* vertices, float* colours, int32_t* faces);

// gut_environment.hip: the cube-map background, its sampler and its adjoint.  The records are checked on the host
// (gut_api.cpp) and travel as kernel arguments.
struct EnvView {
    const float* ray_direction;   // [H,W,3], camera space
    float rotation[9];            // camera-to-world, row-major: the compositor's s2w.r
    int32_t height, width;
};
struct EnvCotangent {
    const float* plane_grad;      // [H,W,3], or null: then the pair below
    const float* rgba;            // [H,W,4]
    const float* rgba_grad;       // [H,W,4]
};
size_t environment_workspace_bytes(int resolution);
void launch_environment_sample(hipStream_t s, const EnvView& v, const float* texels, int resolution, float* plane);
hipError_t launch_environment_backward(hipStream_t s, const EnvView& v, const EnvCotangent& c, int resolution, void* workspace,
                                       float* texel_grad);

// gut_bilateral.hip: per-view bilateral grids of affine colour transforms, the slice and its adjoint.  The record
// is checked on the host (gut_api.cpp), which also forms the two scale factors, and travels as a kernel argument.
struct BilView {
    const float* rgba;               // [H,W,4]
    const float* background_plane;   // [H,W,3], or null: then `background`
    float background;
    const float* grid;               // [12, L, Gh, Gw]
    int32_t levels, rows, columns;
    int32_t height, width;
    float scale_x, scale_y;          // (Gw - 1) / (W - 1) and (Gh - 1) / (H - 1) as float32 divisions; 0 for W == 1 / H == 1
};
size_t bilateral_workspace_bytes(int levels, int rows, int columns);
void launch_bilateral_slice(hipStream_t s, const BilView& v, float* rgba_out);
hipError_t launch_bilateral_backward(hipStream_t s, const BilView& v, const float* out_grad, float lambda_tv, const float (&tv_coeff)[3],
                                     void* workspace, float* rgba_grad, float* grid_grad);
void launch_bilateral_backward_image(hipStream_t s, const BilView& v, const float* out_grad, float* rgba_grad);
void launch_bilateral_adam(hipStream_t s, const float* grad, float* grid, float* m1, float* m2, int32_t* count, uint32_t n, float lr,
                           float beta1, float beta2, float eps);

// scan / sort (rocPRIM device-wide primitives; temp storage owned by the caller)
size_t scan_temp_bytes(uint32_t n);
hipError_t run_scan(hipStream_t s, void* temp, size_t temp_bytes, const uint32_t* in, uint32_t* out, uint32_t n);
size_t sort_temp_bytes(uint32_t m, int end_bit);
hipError_t run_sort(hipStream_t s, void* temp, size_t temp_bytes, const uint64_t* keys_in, uint64_t* keys_out,
                    const uint32_t* vals_in, uint32_t* vals_out, uint32_t m, int end_bit);

}  // namespace gut
