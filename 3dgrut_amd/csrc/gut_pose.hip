// gut_pose.hip — the camera-pose gradient of a view as a reduction of the per-Gaussian gradient rows the backward compositor
// (K7) left in the handle (gut_set_pose_gradient).
//
// The backward differentiates only the per-ray 3-D evaluation, and that depends on the relative placement of ray and Gaussian
// alone: moving a global-shutter camera rigidly equals moving every Gaussian by the inverse motion with its colour held fixed.
// With g_mu / g_q a row's gradient w.r.t. the activated position / quaternion (wxyz), c the sensor position and q the row's
// activated quaternion:
//     F = sum_i g_mu_i,        M = sum_i (mu_i - c) x g_mu_i + tau_i,        tau_i,k = 1/2 g_q_i . ((0, e_k) (x) q_i)
// and for the world-axis twist c' = c + rho, R_c2w' = exp([phi]x) R_c2w:  dL/d rho = -F,  dL/d phi = -M.
//
// Two launches, no float atomics: k_pose_partials keeps six fp32 accumulators per lane over a grid-stride loop of 64-row waves,
// reduces them across the wave and the workgroup in a fixed order and writes one partial per workgroup; k_pose_finish (one wave)
// sums the partials in a fixed order.  The grid depends on N alone, so the six numbers are a pure function of the rows.
// gut_trace_bwd_pose launches a CONSUMING form of k_pose_partials: the same numbers, and the rows it read are left zero.
#include "gut_internal.h"
#include "gut_rows.h"

namespace gut {

constexpr uint32_t kPoseMaxBlocks = 1024;   // partials of one reduction (handle scratch: 32 bytes each)

// kPoseRead: rows are read, never written: the epilogue that follows (K8 / the fused optimiser / the compaction) consumes and zeroes
// them.  The two consuming forms (gut_trace_bwd_pose: no epilogue follows) leave every row they visited, the rows with a tile, as 64
// zero bytes, the scale and colour slots K7 also writes included: kPoseConsumeStore stores four zero float4 per visited row whatever
// it held, kPoseConsumeTest reads the whole row and stores only where a word is set.  Arithmetic, grid and summation order are those
// of the reading form.
enum PoseRows { kPoseRead = 0, kPoseConsumeStore = 1, kPoseConsumeTest = 2 };

template <int kRows> struct PoseRowPointer { typedef const float4* __restrict__ type; };
template <> struct PoseRowPointer<kPoseConsumeStore> { typedef float4* __restrict__ type; };
template <> struct PoseRowPointer<kPoseConsumeTest> { typedef float4* __restrict__ type; };

template <int kRows>
__global__ __launch_bounds__(kBlock) void k_pose_partials(uint32_t n, const uint32_t* __restrict__ tiles_count,
                                                         typename PoseRowPointer<kRows>::type grad16, const float4* __restrict__ density12,
                                                         const float* __restrict__ cam_pos, float* __restrict__ partials) {
    __shared__ float wave_part[kBlock / 64][8];
    const float cx = cam_pos[0], cy = cam_pos[1], cz = cam_pos[2];
    float fx = 0.f, fy = 0.f, fz = 0.f, mx = 0.f, my = 0.f, mz = 0.f;
    uint32_t rows = 0;
    // n <= 2^32 - 1 and gridDim.x * kBlock <= 2^18: the index is kept in 64 bits so that the stride cannot wrap
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        if (tiles_count[i] == 0) continue;
        ++rows;
        const float4 g0 = grad16[4 * i + 0];   // d pos3, d density
        const float4 g1 = grad16[4 * i + 1];   // d quat wxyz
        if constexpr (kRows == kPoseConsumeStore) {
            clear_gradient_row(grad16, i);
        } else if constexpr (kRows == kPoseConsumeTest) {
            const float4 g2 = grad16[4 * i + 2], g3 = grad16[4 * i + 3];   // d scale3 and the colour slots: not summed, zeroed
            const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
            // bit tests: a word that holds -0.f or a NaN is rewritten as well
            auto set = [](const float4& v) { return (__float_as_uint(v.x) | __float_as_uint(v.y) | __float_as_uint(v.z) | __float_as_uint(v.w)) != 0u; };
            if (set(g0)) grad16[4 * i + 0] = zero;
            if (set(g1)) grad16[4 * i + 1] = zero;
            if (set(g2)) grad16[4 * i + 2] = zero;
            if (set(g3)) grad16[4 * i + 3] = zero;
        }
        // A row K7 gave nothing contributes exactly zero; its activated row is not fetched.  (Under the two-pass optimiser the
        // side stream rewrites the activated rows of waves the forward walked nothing of while this kernel runs: those rows have
        // zero gradients, so they are never read here.)
        if (g0.x == 0.f && g0.y == 0.f && g0.z == 0.f && g1.x == 0.f && g1.y == 0.f && g1.z == 0.f && g1.w == 0.f) continue;
        const float4 a = density12[3 * i + 0];  // pos3, density
        const float4 q = density12[3 * i + 1];  // quat wxyz, normalised
        const float rx = a.x - cx, ry = a.y - cy, rz = a.z - cz;
        fx += g0.x; fy += g0.y; fz += g0.z;
        // (0, e_x) (x) q = (-x, w, -z, y),  (0, e_y) (x) q = (-y, z, w, -x),  (0, e_z) (x) q = (-z, -y, x, w)
        const float tx = 0.5f * (-g1.x * q.y + g1.y * q.x - g1.z * q.w + g1.w * q.z);
        const float ty = 0.5f * (-g1.x * q.z + g1.y * q.w + g1.z * q.x - g1.w * q.y);
        const float tz = 0.5f * (-g1.x * q.w - g1.y * q.z + g1.z * q.y + g1.w * q.x);
        mx += (ry * g0.z - rz * g0.y) + tx;
        my += (rz * g0.x - rx * g0.z) + ty;
        mz += (rx * g0.y - ry * g0.x) + tz;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        fx += __shfl_xor(fx, m); fy += __shfl_xor(fy, m); fz += __shfl_xor(fz, m);
        mx += __shfl_xor(mx, m); my += __shfl_xor(my, m); mz += __shfl_xor(mz, m);
        rows += __shfl_xor(rows, m);
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        wave_part[wave][0] = fx; wave_part[wave][1] = fy; wave_part[wave][2] = fz;
        wave_part[wave][3] = mx; wave_part[wave][4] = my; wave_part[wave][5] = mz;
        wave_part[wave][6] = __uint_as_float(rows); wave_part[wave][7] = 0.f;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const uint32_t k = threadIdx.x;
        float out;
        if (k == 6) {
            uint32_t r = 0;
            for (int w = 0; w < kBlock / 64; ++w) r += __float_as_uint(wave_part[w][6]);
            out = __uint_as_float(r);
        } else {
            out = wave_part[0][k];
            for (int w = 1; w < kBlock / 64; ++w) out += wave_part[w][k];
        }
        partials[8 * (size_t)blockIdx.x + k] = out;
    }
}

// one wave: lane = component + 8 * slice; slice s sums the partials s, s + 8, ... in order, then the eight slices are combined by
// a fixed butterfly.  out8 = {F, M, rows summed, 0}
__global__ __launch_bounds__(64) void k_pose_finish(uint32_t num_partials, const float* __restrict__ partials, float* __restrict__ out8) {
    const uint32_t k = threadIdx.x & 7u, slice = threadIdx.x >> 3;
    float acc = 0.f;
    uint32_t rows = 0;
    for (uint32_t j = slice; j < num_partials; j += 8u) {
        const float p = partials[8 * (size_t)j + k];
        if (k == 6) rows += __float_as_uint(p);
        else acc += p;
    }
#pragma unroll
    for (int m = 8; m <= 32; m <<= 1) {
        acc += __shfl_xor(acc, m);
        rows += __shfl_xor(rows, m);
    }
    if (slice == 0) out8[k] = k == 6 ? (float)rows : (k == 7 ? 0.f : acc);
}

size_t pose_gradient_scratch_bytes() { return sizeof(float) * 8 * kPoseMaxBlocks; }

static uint32_t pose_blocks(uint32_t n) {
    return (uint32_t)(((uint64_t)n + kBlock - 1) / kBlock < kPoseMaxBlocks ? ((uint64_t)n + kBlock - 1) / kBlock : kPoseMaxBlocks);
}

void launch_pose_gradient(hipStream_t s, uint32_t n, const uint32_t* tiles_count, const float* grad16, const float* density12,
                          const float* cam_pos, float* partials, float* out8) {
    if (n == 0) return;
    const uint32_t blocks = pose_blocks(n);
    hipLaunchKernelGGL(k_pose_partials<kPoseRead>, dim3(blocks), dim3(kBlock), 0, s, n, tiles_count, reinterpret_cast<const float4*>(grad16),
                       reinterpret_cast<const float4*>(density12), cam_pos, partials);
    hipLaunchKernelGGL(k_pose_finish, dim3(1), dim3(64), 0, s, blocks, partials, out8);
}

void launch_pose_gradient_consume(hipStream_t s, uint32_t n, const uint32_t* tiles_count, float* grad16, const float* density12,
                                  const float* cam_pos, float* partials, float* out8, bool test_before_store) {
    if (n == 0) return;
    const uint32_t blocks = pose_blocks(n);
    if (test_before_store)
        hipLaunchKernelGGL(k_pose_partials<kPoseConsumeTest>, dim3(blocks), dim3(kBlock), 0, s, n, tiles_count, reinterpret_cast<float4*>(grad16),
                           reinterpret_cast<const float4*>(density12), cam_pos, partials);
    else
        hipLaunchKernelGGL(k_pose_partials<kPoseConsumeStore>, dim3(blocks), dim3(kBlock), 0, s, n, tiles_count, reinterpret_cast<float4*>(grad16),
                           reinterpret_cast<const float4*>(density12), cam_pos, partials);
    hipLaunchKernelGGL(k_pose_finish, dim3(1), dim3(64), 0, s, blocks, partials, out8);
}

// Adam on the six pose coordinates of ONE view (3dgrut_amd/pose_refine.py): gradient (-F, -M) from the reduction's output, the
// view's own moments and visit count (bias correction by that count), rates lr_translation for rho and lr_rotation for phi;
// delta6 receives the increment (d rho, d phi) the host composes with the view's pose.  One launch of one wave.
__global__ __launch_bounds__(64) void k_pose_adam(const float* __restrict__ grad8, float* __restrict__ m6, float* __restrict__ v6,
                                                  int32_t* __restrict__ count, float lr_translation, float lr_rotation, float beta1,
                                                  float beta2, float eps, float* __restrict__ delta6) {
    const uint32_t k = threadIdx.x;
    const int32_t t = count[0] + 1;   // every lane reads the count before lane 0 stores it (one wave: the barrier below orders them)
    __syncthreads();
    if (k == 0) count[0] = t;
    if (k >= 6) return;
    const float g = -grad8[k];
    const float m = beta1 * m6[k] + (1.0f - beta1) * g;
    const float v = beta2 * v6[k] + (1.0f - beta2) * g * g;
    m6[k] = m;
    v6[k] = v;
    const float m_hat = m / (1.0f - powf(beta1, (float)t));
    const float v_hat = v / (1.0f - powf(beta2, (float)t));
    delta6[k] = -(k < 3 ? lr_translation : lr_rotation) * m_hat / (sqrtf(v_hat) + eps);
}

void launch_pose_adam(hipStream_t s, const float* grad8, float* m6, float* v6, int32_t* count, float lr_translation, float lr_rotation,
                      float beta1, float beta2, float eps, float* delta6) {
    hipLaunchKernelGGL(k_pose_adam, dim3(1), dim3(64), 0, s, grad8, m6, v6, count, lr_translation, lr_rotation, beta1, beta2, eps, delta6);
}

}  // namespace gut
