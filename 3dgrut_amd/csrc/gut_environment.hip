// gut_environment.hip — a learnt radiance at infinity: a cube map behind the Gaussians, for gfx950:
//   k_env_sample     one thread per pixel: direction -> face, texel coordinates, bilinear weights -> the [H,W,3] background plane
//   k_env_max_abs    the largest finite |c| of a cotangent, as float bits (a DPP maximum per wave, one atomicMax per wave)
//   k_env_scatter    the adjoint: every product w c_k as an integer of the unit 2^-s, summed per texel in LDS by a 16x16 pixel tile,
//                    one 64-bit integer atomic per occupied slot and channel
//   k_env_convert    int64 sums -> the caller's float gradient, every element written
//
// THIS FILE IS COMPILED WITH -ffp-contract=off: the face of a pixel and its texels are integer decisions of fp32 arithmetic, and the
// plane is compared bit for bit with a float32 restatement on the CPU.  Every step is IEEE-exact +,-,*,/ in the order of §20; the
// sampler and the adjoint share ONE copy of the coordinate code (env_taps).  No float atomics anywhere: the sums are integers, so a
// texel's total does not depend on the order in which workgroups, waves or the two routes (LDS table, direct) deliver it.
#include "gut_render_common.h"
#include "gut_fixed.h"   // the fixed-point unit: pow2f_env, finite_or_zero_env, env_scale_exponent

namespace gut {

namespace {

constexpr uint32_t kEnvSlots = GUT_ENVIRONMENT_SLOTS;   // entries of a workgroup's table, a power of two
constexpr uint32_t kEnvProbes = 8;                      // slots a contribution tries before it takes the direct route
constexpr uint32_t kEnvEmpty = 0xFFFFFFFFu;
constexpr int kEnvTile = 16;                            // the scatter's workgroup owns kEnvTile x kEnvTile pixels
constexpr uint32_t kEnvMaxBlocks = 1024;                // grid of the maximum's grid-stride loop
static_assert((kEnvSlots & (kEnvSlots - 1u)) == 0u && kEnvSlots <= (uint32_t)kBlock, "one flushing thread per slot");
static_assert(kEnvTile * kEnvTile == kBlock, "one thread per pixel of the tile");

// The four taps of a pixel: texel (first of its three channels) and weight, w_ab pairing column a with row b in the order
// 00, 10, 01, 11.  Returns false for a void pixel: a direction that is zero or not finite.  Steps 1 to 5 of DESIGN.md §20.
struct EnvTaps {
    uint32_t at[4];
    float w[4];
};
__device__ __forceinline__ bool env_taps(const EnvView& v, size_t pix, int R, EnvTaps& t) {
    const float d0 = v.ray_direction[3 * pix + 0], d1 = v.ray_direction[3 * pix + 1], d2 = v.ray_direction[3 * pix + 2];
    float e[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) e[i] = (v.rotation[3 * i + 0] * d0 + v.rotation[3 * i + 1] * d1) + v.rotation[3 * i + 2] * d2;
    const float a0 = fabsf(e[0]), a1 = fabsf(e[1]), a2 = fabsf(e[2]);
    constexpr float kMaxFinite = 3.4028234664e+38f;
    if (!(a0 <= kMaxFinite && a1 <= kMaxFinite && a2 <= kMaxFinite)) return false;   // inf or NaN
    const int axis = (a0 >= a1 && a0 >= a2) ? 0 : (a1 >= a2 ? 1 : 2);
    const float m = axis == 0 ? a0 : (axis == 1 ? a1 : a2);
    if (m == 0.0f) return false;
    const float major = axis == 0 ? e[0] : (axis == 1 ? e[1] : e[2]);
    const float eu = axis == 0 ? e[1] : (axis == 1 ? e[2] : e[0]);   // cyclic, no sign flips
    const float ev = axis == 0 ? e[2] : (axis == 1 ? e[0] : e[1]);
    const uint32_t face = 2u * (uint32_t)axis + (major < 0.0f ? 1u : 0u);
    const float u = eu / m, w = ev / m;                              // correctly rounded; |u|, |w| <= 1
    const float half = 0.5f * (float)R;
    const float s = (u + 1.0f) * half - 0.5f, q = (w + 1.0f) * half - 0.5f;   // -0.5 .. R - 0.5
    const float fi = floorf(s), fj = floorf(q);
    const float fx = s - fi, fy = q - fj;
    const int i0 = (int)fi, j0 = (int)fj;                            // -1 .. R - 1
    const int c0 = min(max(i0, 0), R - 1), c1 = min(max(i0 + 1, 0), R - 1);
    const int r0 = min(max(j0, 0), R - 1), r1 = min(max(j0 + 1, 0), R - 1);
    const float wx0 = 1.0f - fx, wy0 = 1.0f - fy;
    t.w[0] = wx0 * wy0;
    t.w[1] = fx * wy0;
    t.w[2] = wx0 * fy;
    t.w[3] = fx * fy;
    const uint32_t base = face * (uint32_t)R * (uint32_t)R;          // 18 R^2 <= 2^31 (GUT_ENVIRONMENT_MAX_RESOLUTION)
    t.at[0] = 3u * (base + (uint32_t)r0 * (uint32_t)R + (uint32_t)c0);
    t.at[1] = 3u * (base + (uint32_t)r0 * (uint32_t)R + (uint32_t)c1);
    t.at[2] = 3u * (base + (uint32_t)r1 * (uint32_t)R + (uint32_t)c0);
    t.at[3] = 3u * (base + (uint32_t)r1 * (uint32_t)R + (uint32_t)c1);
    return true;
}

__global__ __launch_bounds__(kBlock) void k_env_sample(EnvView v, const float* __restrict__ texels, int R, float* __restrict__ plane) {
    const size_t pix = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (pix >= (size_t)v.height * (size_t)v.width) return;
    float b[3] = {0.0f, 0.0f, 0.0f};
    EnvTaps t;
    if (env_taps(v, pix, R, t)) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            b[k] = ((t.w[0] * texels[t.at[0] + k] + t.w[1] * texels[t.at[1] + k]) + t.w[2] * texels[t.at[2] + k]) + t.w[3] * texels[t.at[3] + k];
    }
    plane[3 * pix + 0] = b[0];
    plane[3 * pix + 1] = b[1];
    plane[3 * pix + 2] = b[2];
}

// The cotangent of a pixel, non-finite values as 0.  kRgba: c = (1 - alpha) g_rgb, 1 - alpha rounded first, then each product.
template <bool kRgba>
__device__ __forceinline__ void env_cotangent(const EnvCotangent& c, size_t pix, float (&out)[3]) {
    if constexpr (kRgba) {
        const float t = 1.0f - c.rgba[4 * pix + 3];
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = finite_or_zero_env(t * c.rgba_grad[4 * pix + k]);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = finite_or_zero_env(c.plane_grad[3 * pix + k]);
    }
}

template <bool kRgba>
__global__ __launch_bounds__(kBlock) void k_env_max_abs(EnvCotangent c, size_t pixels, uint32_t* __restrict__ max_bits) {
    float m = 0.0f;
    for (size_t pix = (size_t)blockIdx.x * kBlock + threadIdx.x; pix < pixels; pix += (size_t)gridDim.x * kBlock) {
        float g[3];
        env_cotangent<kRgba>(c, pix, g);
        m = fmaxf(m, fmaxf(fabsf(g[0]), fmaxf(fabsf(g[1]), fabsf(g[2]))));
    }
    m = dpp_wave_max_lane63(m);
    if ((threadIdx.x & 63u) == 63u && m > 0.0f) atomicMax(max_bits, __float_as_uint(m));   // non-negative floats order as their bits
}

template <bool kRgba>
__global__ __launch_bounds__(kBlock) void k_env_scatter(EnvView v, EnvCotangent c, int R, const uint32_t* __restrict__ max_bits,
                                                        unsigned long long* __restrict__ sums_q) {
    __shared__ uint32_t s_key[kEnvSlots];
    __shared__ unsigned long long s_sum[kEnvSlots][3];
    const uint32_t tid = threadIdx.x;
    if (tid < kEnvSlots) {
        s_key[tid] = kEnvEmpty;
        s_sum[tid][0] = 0ull;
        s_sum[tid][1] = 0ull;
        s_sum[tid][2] = 0ull;
    }
    __syncthreads();
    const int px = (int)blockIdx.x * kEnvTile + (int)(tid & (kEnvTile - 1)), py = (int)blockIdx.y * kEnvTile + (int)(tid >> 4);
    if (px < v.width && py < v.height) {
        const size_t pix = (size_t)py * (size_t)v.width + (size_t)px;
        float g[3];
        env_cotangent<kRgba>(c, pix, g);
        EnvTaps t;
        if ((g[0] != 0.0f || g[1] != 0.0f || g[2] != 0.0f) && env_taps(v, pix, R, t)) {
            const float scale = pow2f_env(env_scale_exponent(max_bits[0], (uint64_t)v.height * (uint64_t)v.width));
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                long long q[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float p = t.w[n] * g[k];        // rounded to fp32 on its own (no contraction in this unit)
                    q[k] = __float2ll_rn(p * scale);      // exact product, then to nearest, ties to even
                }
                if (q[0] == 0ll && q[1] == 0ll && q[2] == 0ll) continue;
                const uint32_t key = t.at[n];
                uint32_t slot = (key * 2654435761u) >> (32 - __builtin_ctz(kEnvSlots));
                bool placed = false;
                for (uint32_t probe = 0; probe < kEnvProbes; ++probe) {
                    const uint32_t seen = atomicCAS(&s_key[slot], kEnvEmpty, key);
                    if (seen == kEnvEmpty || seen == key) {
                        placed = true;
                        break;
                    }
                    slot = (slot + 1u) & (kEnvSlots - 1u);
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (q[k] == 0ll) continue;
                    if (placed) atomicAdd(&s_sum[slot][k], (unsigned long long)q[k]);
                    else atomicAdd(sums_q + key + k, (unsigned long long)q[k]);
                }
            }
        }
    }
    __syncthreads();
    if (tid < kEnvSlots) {
        const uint32_t key = s_key[tid];
        if (key != kEnvEmpty) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const unsigned long long q = s_sum[tid][k];
                if (q != 0ull) atomicAdd(sums_q + key + k, q);
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_env_convert(const long long* __restrict__ sums_q, const uint32_t* __restrict__ max_bits,
                                                        uint64_t pixels, uint32_t count, float* __restrict__ grad) {
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= count) return;
    grad[i] = __ll2float_rn(sums_q[i]) * pow2f_env(-env_scale_exponent(max_bits[0], pixels));
}

inline size_t env_sums_bytes(int R) { return sizeof(long long) * 18u * (size_t)R * (size_t)R; }

}  // namespace

size_t environment_workspace_bytes(int resolution) { return env_sums_bytes(resolution) + 16; }   // the sums, then the maximum's word

void launch_environment_sample(hipStream_t s, const EnvView& v, const float* texels, int resolution, float* plane) {
    const size_t pixels = (size_t)v.height * (size_t)v.width;
    hipLaunchKernelGGL(k_env_sample, dim3((uint32_t)((pixels + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, v, texels, resolution, plane);
}

hipError_t launch_environment_backward(hipStream_t s, const EnvView& v, const EnvCotangent& c, int resolution, void* workspace,
                                       float* texel_grad) {
    const size_t pixels = (size_t)v.height * (size_t)v.width;
    unsigned long long* const sums_q = static_cast<unsigned long long*>(workspace);
    uint32_t* const max_bits = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + env_sums_bytes(resolution));
    if (hipError_t err = hipMemsetAsync(workspace, 0, environment_workspace_bytes(resolution), s)) return err;
    const size_t want = (pixels + kBlock - 1) / kBlock;
    const dim3 max_grid((uint32_t)(want < kEnvMaxBlocks ? want : kEnvMaxBlocks));
    const dim3 tiles((uint32_t)((v.width + kEnvTile - 1) / kEnvTile), (uint32_t)((v.height + kEnvTile - 1) / kEnvTile));
    const uint32_t count = 18u * (uint32_t)resolution * (uint32_t)resolution;
    if (c.plane_grad) {
        hipLaunchKernelGGL(k_env_max_abs<false>, max_grid, dim3(kBlock), 0, s, c, pixels, max_bits);
        hipLaunchKernelGGL(k_env_scatter<false>, tiles, dim3(kBlock), 0, s, v, c, resolution, max_bits, sums_q);
    } else {
        hipLaunchKernelGGL(k_env_max_abs<true>, max_grid, dim3(kBlock), 0, s, c, pixels, max_bits);
        hipLaunchKernelGGL(k_env_scatter<true>, tiles, dim3(kBlock), 0, s, v, c, resolution, max_bits, sums_q);
    }
    hipLaunchKernelGGL(k_env_convert, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, s, reinterpret_cast<const long long*>(sums_q),
                       max_bits, (uint64_t)pixels, count, texel_grad);
    return hipSuccess;
}

}  // namespace gut
