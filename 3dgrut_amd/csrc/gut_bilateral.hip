// gut_bilateral.hip — per-view bilateral grids of affine colour transforms, for gfx950:
//   k_bilateral_slice     one thread per pixel: composite, guidance, eight taps of twelve channels, the 3x4 transform applied
//   k_bilateral_max_abs   the call's magnitude m = max_pixels max_i |g'_i| max(1, max_j |comp_j|), as float bits
//   k_bilateral_backward  the adjoint: rgba_grad per pixel, and the 96 products w_n (g'_i c4_j) per pixel as integers of the unit
//                         2^-s, summed by a 16x16 pixel tile in a direct-indexed LDS table over the tile's footprint in the grid,
//                         one 64-bit integer atomic per non-zero sum
//   k_bilateral_finish    int64 sums -> the caller's float gradient, plus the total-variation term; every element written
//   k_bilateral_adam      the per-view Adam step over the view's 12 L Gh Gw floats (view_adam_element, shared with the exposures)
//
// THIS FILE IS COMPILED WITH -ffp-contract=off: the slice, both gradients, the TV term and the step are compared bit for bit with a
// float32 restatement on the CPU.  Every step is IEEE-exact +,-,*,/ in the order of §21; the slice and the adjoint share ONE copy
// of the composite, coordinate, weight and gather code (bil_composite, bil_pixel, bil_gather).  No float atomics anywhere: the sums
// are integers, so a cell's total does not depend on the order in which workgroups, waves or the two routes (LDS table, direct)
// deliver it.
#include "gut_render_common.h"
#include "gut_fixed.h"

namespace gut {

namespace {

constexpr int kBilTile = 16;                              // the adjoint's workgroup owns kBilTile x kBilTile pixels
constexpr uint32_t kBilTable = GUT_BILATERAL_TABLE;       // 64-bit sums of a workgroup's table
constexpr uint32_t kBilMaxBlocks = 1024;                  // grid of the maximum's grid-stride loop
constexpr uint32_t kBilAdamBlocks = 2048;                 // grid of the step's grid-stride loop: the ticket below counts them in 12 bits
constexpr uint32_t kBilTicketShift = 20;                  // the visit count lives in the low 20 bits while a step is in flight
static_assert(kBilTile * kBilTile == kBlock, "one thread per pixel of the tile");
static_assert(kBilAdamBlocks < (1u << (32 - kBilTicketShift)), "the tickets of a step fit above the count");

// Steps 1 to 3 of §21 for one pixel: the composite, the guidance and the taps.  Tap n pairs xy tap n & 3 (00, 10, 01, 11, x
// fastest) with level n >> 2; w_n = wxy[n & 3] * wz[n >> 2]; its cell is z[n >> 2] * Gh * Gw + xy[n & 3].
struct BilPixel {
    float comp[3], B[3];    // the composite and the background it was made over
    float wxy[4], wz[2];
    uint32_t xy[4], z[2];   // row * Gw + column; level
    int col[2], row[2];     // the two columns and the two rows xy was made of
    bool inside;
};

// Step 1: the background of a pixel and its composite, comp_k = rgb_k + B_k (1 - alpha).  ONE copy for the slice, the maximum and
// the adjoint.
__device__ __forceinline__ void bil_composite(const BilView& v, size_t pix, const float4 rgba, float (&comp)[3], float (&B)[3]) {
    const float alpha1 = 1.0f - rgba.w;
    B[0] = B[1] = B[2] = v.background;
    if (v.background_plane) {
        B[0] = v.background_plane[3 * pix + 0];
        B[1] = v.background_plane[3 * pix + 1];
        B[2] = v.background_plane[3 * pix + 2];
    }
    comp[0] = rgba.x + B[0] * alpha1;
    comp[1] = rgba.y + B[1] * alpha1;
    comp[2] = rgba.z + B[2] * alpha1;
}

// floor(s), the fraction and the two indices of one axis of length n; s >= 0 and finite.
__device__ __forceinline__ void bil_axis(float s, int n, float& f, int& i0, int& i1) {
    const float fl = floorf(s);
    f = s - fl;
    i0 = min(max((int)fl, 0), n - 1);   // (the clamp of i0 never acts: s <= n - 1 up to one rounding, whose floor is n - 1)
    i1 = min(i0 + 1, n - 1);
}

__device__ __forceinline__ void bil_pixel(const BilView& v, int x, int y, size_t pix, const float4 rgba, BilPixel& p) {
    bil_composite(v, pix, rgba, p.comp, p.B);
    const float g = (0.299f * p.comp[0] + 0.587f * p.comp[1]) + 0.114f * p.comp[2];
    const float gc = fminf(fmaxf(g, 0.0f), 1.0f);   // fmaxf(NaN, 0) is 0
    p.inside = 0.0f < g && g < 1.0f;
    float fx, fy, fz;
    int c0, c1, r0, r1, z0, z1;
    bil_axis((float)x * v.scale_x, v.columns, fx, c0, c1);
    bil_axis((float)y * v.scale_y, v.rows, fy, r0, r1);
    bil_axis(gc * (float)(v.levels - 1), v.levels, fz, z0, z1);
    const float wx0 = 1.0f - fx, wy0 = 1.0f - fy;
    p.wxy[0] = wx0 * wy0;
    p.wxy[1] = fx * wy0;
    p.wxy[2] = wx0 * fy;
    p.wxy[3] = fx * fy;
    p.wz[0] = 1.0f - fz;
    p.wz[1] = fz;
    const uint32_t Gw = (uint32_t)v.columns;
    p.xy[0] = (uint32_t)r0 * Gw + (uint32_t)c0;
    p.xy[1] = (uint32_t)r0 * Gw + (uint32_t)c1;
    p.xy[2] = (uint32_t)r1 * Gw + (uint32_t)c0;
    p.xy[3] = (uint32_t)r1 * Gw + (uint32_t)c1;
    p.z[0] = (uint32_t)z0;
    p.z[1] = (uint32_t)z1;
    p.col[0] = c0;
    p.col[1] = c1;
    p.row[0] = r0;
    p.row[1] = r1;
}

// Step 4: A_k = sum over the taps in order of w_n G[k, tap_n], each product rounded on its own; kDerivative: also
// dA_k = sum over the xy taps in order of wxy (G[k, z1] - G[k, z0]), the derivative of A_k by sz inside the pixel's piece.
template <bool kDerivative>
__device__ __forceinline__ void bil_gather(const BilView& v, const BilPixel& p, float (&A)[12], float (&dA)[12]) {
    const uint32_t plane = (uint32_t)v.rows * (uint32_t)v.columns, cells = plane * (uint32_t)v.levels;   // 12 cells <= 12 2^24
    const uint32_t base0 = p.z[0] * plane, base1 = p.z[1] * plane;
    float w[8];
#pragma unroll
    for (int n = 0; n < 8; ++n) w[n] = p.wxy[n & 3] * p.wz[n >> 2];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const float* __restrict__ G = v.grid + (size_t)k * cells;
        float lo[4], hi[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            lo[n] = G[base0 + p.xy[n]];
            hi[n] = G[base1 + p.xy[n]];
        }
        float a = w[0] * lo[0];
#pragma unroll
        for (int n = 1; n < 4; ++n) a = a + w[n] * lo[n];
#pragma unroll
        for (int n = 0; n < 4; ++n) a = a + w[4 + n] * hi[n];
        A[k] = a;
        if constexpr (kDerivative) {
            float d = p.wxy[0] * (hi[0] - lo[0]);
#pragma unroll
            for (int n = 1; n < 4; ++n) d = d + p.wxy[n] * (hi[n] - lo[n]);
            dA[k] = d;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_bilateral_slice(BilView v, float* __restrict__ rgba_out) {
    const size_t pix = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (pix >= (size_t)v.height * (size_t)v.width) return;
    const int y = (int)(pix / (size_t)v.width), x = (int)(pix - (size_t)y * (size_t)v.width);
    const float4 rgba = reinterpret_cast<const float4*>(v.rgba)[pix];
    BilPixel p;
    bil_pixel(v, x, y, pix, rgba, p);
    float A[12], unused[12];
    bil_gather<false>(v, p, A, unused);
    float4 out;
    out.x = ((A[0] * p.comp[0] + A[1] * p.comp[1]) + A[2] * p.comp[2]) + A[3];
    out.y = ((A[4] * p.comp[0] + A[5] * p.comp[1]) + A[6] * p.comp[2]) + A[7];
    out.z = ((A[8] * p.comp[0] + A[9] * p.comp[1]) + A[10] * p.comp[2]) + A[11];
    out.w = rgba.w;
    reinterpret_cast<float4*>(rgba_out)[pix] = out;
}

// The loss's cotangent of a pixel: the rgb part with non-finite values as 0, the alpha part as it is.
__device__ __forceinline__ float4 bil_cotangent(const float* __restrict__ out_grad, size_t pix) {
    float4 g = reinterpret_cast<const float4*>(out_grad)[pix];
    g.x = finite_or_zero_env(g.x);
    g.y = finite_or_zero_env(g.y);
    g.z = finite_or_zero_env(g.z);
    return g;
}

// A pixel's share of the magnitude: max_i |g'_i| max(1, max_j |comp_j|) over the finite comp_j; a non-finite product counts as 0,
// as the product t_ij it bounds does in the scatter.
__device__ __forceinline__ float bil_magnitude(const float4 g, const float (&comp)[3]) {
    const float gm = fmaxf(fabsf(g.x), fmaxf(fabsf(g.y), fabsf(g.z)));
    float cm = 1.0f;
#pragma unroll
    for (int j = 0; j < 3; ++j) cm = fmaxf(cm, finite_or_zero_env(fabsf(comp[j])));
    return finite_or_zero_env(gm * cm);
}

__global__ __launch_bounds__(kBlock) void k_bilateral_max_abs(BilView v, const float* __restrict__ out_grad, uint32_t* __restrict__ max_bits) {
    const size_t pixels = (size_t)v.height * (size_t)v.width;
    float m = 0.0f;
    for (size_t pix = (size_t)blockIdx.x * kBlock + threadIdx.x; pix < pixels; pix += (size_t)gridDim.x * kBlock) {
        const float4 rgba = reinterpret_cast<const float4*>(v.rgba)[pix];
        float comp[3], B[3];
        bil_composite(v, pix, rgba, comp, B);
        m = fmaxf(m, bil_magnitude(bil_cotangent(out_grad, pix), comp));
    }
    m = dpp_wave_max_lane63(m);
    if ((threadIdx.x & 63u) == 63u && m > 0.0f) atomicMax(max_bits, __float_as_uint(m));   // non-negative floats order as their bits
}

// The first and the last index an axis of a tile can reach: pixels lo .. hi of the image axis, bil_axis's own arithmetic (a float
// product with a non-negative scale is monotone in the pixel, so every pixel between lies between).
__device__ __forceinline__ void bil_footprint(int lo, int hi, float scale, int n, int& first, int& count) {
    float f;
    int a0, a1, b0, b1;
    bil_axis((float)lo * scale, n, f, a0, a1);
    bil_axis((float)hi * scale, n, f, b0, b1);
    first = a0;
    count = b1 - a0 + 1;
}

// kScatter false: the image gradient alone (outside the grids' iteration window): no table, no barrier, no atomics.
template <bool kScatter>
__global__ __launch_bounds__(kBlock) void k_bilateral_backward(BilView v, const float* __restrict__ out_grad, const uint32_t* __restrict__ max_bits,
                                                               float* __restrict__ rgba_grad, unsigned long long* __restrict__ sums_q) {
    __shared__ unsigned long long s_sum[kScatter ? kBilTable : 1];
    const uint32_t tid = threadIdx.x;
    // the tile's footprint in the grid: workgroup-uniform
    const int x_lo = (int)blockIdx.x * kBilTile, y_lo = (int)blockIdx.y * kBilTile;
    int cx, ncx, cy, ncy;
    bil_footprint(x_lo, min(x_lo + kBilTile - 1, v.width - 1), v.scale_x, v.columns, cx, ncx);
    bil_footprint(y_lo, min(y_lo + kBilTile - 1, v.height - 1), v.scale_y, v.rows, cy, ncy);
    const uint32_t local_plane = (uint32_t)ncx * (uint32_t)ncy;                       // <= 2^16
    const uint32_t entries = local_plane * (uint32_t)v.levels * 12u;                  // <= 2^16 2^8 12 < 2^28
    const bool table = kScatter && entries <= kBilTable;
    if (table) {
        for (uint32_t e = tid; e < entries; e += (uint32_t)kBlock) s_sum[e] = 0ull;
    }
    __syncthreads();
    const uint32_t plane = (uint32_t)v.rows * (uint32_t)v.columns, cells = plane * (uint32_t)v.levels;
    const int px = x_lo + (int)(tid & (kBilTile - 1)), py = y_lo + (int)(tid >> 4);
    if (px < v.width && py < v.height) {
        const size_t pix = (size_t)py * (size_t)v.width + (size_t)px;
        const float4 rgba = reinterpret_cast<const float4*>(v.rgba)[pix];
        const float4 g4 = bil_cotangent(out_grad, pix);
        const float g[3] = {g4.x, g4.y, g4.z};
        BilPixel p;
        bil_pixel(v, px, py, pix, rgba, p);
        float A[12], dA[12];
        bil_gather<true>(v, p, A, dA);
        // the image gradient
        float dc[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) dc[j] = (A[j] * g[0] + A[4 + j] * g[1]) + A[8 + j] * g[2];
        if (p.inside) {
            float d[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) d[i] = ((dA[4 * i] * p.comp[0] + dA[4 * i + 1] * p.comp[1]) + dA[4 * i + 2] * p.comp[2]) + dA[4 * i + 3];
            const float D = (g[0] * d[0] + g[1] * d[1]) + g[2] * d[2];
            const float lm1 = (float)(v.levels - 1);
            dc[0] = dc[0] + (0.299f * lm1) * D;
            dc[1] = dc[1] + (0.587f * lm1) * D;
            dc[2] = dc[2] + (0.114f * lm1) * D;
        }
        const float (&B)[3] = p.B;
        float4 out;
        out.x = dc[0];
        out.y = dc[1];
        out.z = dc[2];
        out.w = -((B[0] * dc[0] + B[1] * dc[1]) + B[2] * dc[2]) + g4.w;
        reinterpret_cast<float4*>(rgba_grad)[pix] = out;
        // the grid gradient
        if constexpr (kScatter) if (g[0] != 0.0f || g[1] != 0.0f || g[2] != 0.0f) {
            const float scale = pow2f_env(env_scale_exponent(max_bits[0], (uint64_t)v.height * (uint64_t)v.width));
            float w[8];
            uint32_t cell[8], slot[8];
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                w[n] = p.wxy[n & 3] * p.wz[n >> 2];
                const uint32_t xy = p.xy[n & 3], z = p.z[n >> 2];
                cell[n] = z * plane + xy;
                const uint32_t row = (uint32_t)(p.row[(n >> 1) & 1] - cy), col = (uint32_t)(p.col[n & 1] - cx);
                slot[n] = z * local_plane + row * (uint32_t)ncx + col;   // < local_plane * levels
            }
            const uint32_t local_cells = local_plane * (uint32_t)v.levels;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float t = finite_or_zero_env(j < 3 ? g[i] * p.comp[j] : g[i]);   // rounded on its own; c4_3 = 1 is exact
                    if (t == 0.0f) continue;
                    const uint32_t k = (uint32_t)(4 * i + j);
#pragma unroll
                    for (int n = 0; n < 8; ++n) {
                        const long long q = __float2ll_rn((w[n] * t) * scale);   // product rounded, exact scaling, to nearest even
                        if (q == 0ll) continue;
                        const uint32_t e = k * local_cells + slot[n];
                        if (table && e < entries) atomicAdd(&s_sum[e], (unsigned long long)q);
                        else atomicAdd(sums_q + (size_t)k * cells + cell[n], (unsigned long long)q);
                    }
                }
            }
        }
    }
    __syncthreads();
    if (table) {
        const uint32_t local_cells = local_plane * (uint32_t)v.levels;
        for (uint32_t e = tid; e < entries; e += (uint32_t)kBlock) {
            const unsigned long long q = s_sum[e];
            if (q == 0ull) continue;
            const uint32_t k = e / local_cells, c = e - k * local_cells;
            const uint32_t z = c / local_plane, r = c - z * local_plane;
            const uint32_t row = r / (uint32_t)ncx, col = r - row * (uint32_t)ncx;
            atomicAdd(sums_q + (size_t)k * cells + z * plane + (row + (uint32_t)cy) * (uint32_t)v.columns + (col + (uint32_t)cx), q);
        }
    }
}

// Sums to floats, and lambda_tv dTV/dG of §21: per axis x, y, z of length > 1, with a = G[c] - G[previous] (0 at the first index) and
// b = G[next] - G[c] (0 at the last), acc = acc + coeff_axis (a - b) from acc = 0; grad = grad + lambda_tv acc.  coeff = 2 / n_axis.
struct BilTv {
    float lambda_tv;
    float coeff[3];   // x, y, z; unused for an axis of length 1
};

template <bool kTv>
__global__ __launch_bounds__(kBlock) void k_bilateral_finish(const long long* __restrict__ sums_q, const uint32_t* __restrict__ max_bits,
                                                             uint64_t pixels, const float* __restrict__ grid, int L, int Gh, int Gw, BilTv tv,
                                                             float* __restrict__ grad) {
    const uint32_t plane = (uint32_t)Gh * (uint32_t)Gw, cells = plane * (uint32_t)L;
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= 12u * cells) return;
    float out = __ll2float_rn(sums_q[i]) * pow2f_env(-env_scale_exponent(max_bits[0], pixels));
    if constexpr (kTv) {
        const uint32_t c = i % cells;
        const uint32_t z = c / plane, r = c - z * plane;
        const uint32_t y = r / (uint32_t)Gw, x = r - y * (uint32_t)Gw;
        const uint32_t at[3] = {x, y, z}, len[3] = {(uint32_t)Gw, (uint32_t)Gh, (uint32_t)L}, stride[3] = {1u, (uint32_t)Gw, plane};
        const float here = grid[i];
        float acc = 0.0f;
#pragma unroll
        for (int axis = 0; axis < 3; ++axis) {
            if (len[axis] < 2u) continue;
            const float a = at[axis] > 0u ? here - grid[i - stride[axis]] : 0.0f;
            const float b = at[axis] + 1u < len[axis] ? grid[i + stride[axis]] - here : 0.0f;
            acc = acc + tv.coeff[axis] * (a - b);
        }
        out = out + tv.lambda_tv * acc;
    }
    grad[i] = out;
}

// The step of one view.  The visit count is advanced once, by the workgroup that arrives last: every workgroup takes a ticket in the
// bits above kBilTicketShift, reads the count below them from the same atomic, and the last one stores count + 1 with the tickets
// cleared.  No workgroup waits for another.  A view is visited fewer than 2^20 times.
__global__ __launch_bounds__(kBlock) void k_bilateral_adam(const float* __restrict__ grad, float* __restrict__ grid, float* __restrict__ m1,
                                                           float* __restrict__ m2, int32_t* __restrict__ count, uint32_t n, float lr, float beta1,
                                                           float beta2, float eps) {
    __shared__ int32_t s_t;
    if (threadIdx.x == 0) {
        const uint32_t seen = atomicAdd(reinterpret_cast<uint32_t*>(count), 1u << kBilTicketShift);
        const int32_t t = (int32_t)(seen & ((1u << kBilTicketShift) - 1u)) + 1;
        s_t = t;
        if ((seen >> kBilTicketShift) == gridDim.x - 1u) atomicExch(reinterpret_cast<uint32_t*>(count), (uint32_t)t);
    }
    __syncthreads();
    const int32_t t = s_t;
    for (uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x; i < n; i += gridDim.x * (uint32_t)kBlock)
        view_adam_element(grad[i], grid + i, m1 + i, m2 + i, t, lr, beta1, beta2, eps);
}

inline size_t bil_sums_bytes(int L, int Gh, int Gw) { return sizeof(long long) * 12u * (size_t)L * (size_t)Gh * (size_t)Gw; }

}  // namespace

size_t bilateral_workspace_bytes(int levels, int rows, int columns) { return bil_sums_bytes(levels, rows, columns) + 16; }   // sums, maximum

void launch_bilateral_slice(hipStream_t s, const BilView& v, float* rgba_out) {
    const size_t pixels = (size_t)v.height * (size_t)v.width;
    hipLaunchKernelGGL(k_bilateral_slice, dim3((uint32_t)((pixels + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, v, rgba_out);
}

hipError_t launch_bilateral_backward(hipStream_t s, const BilView& v, const float* out_grad, float lambda_tv, const float (&tv_coeff)[3],
                                     void* workspace, float* rgba_grad, float* grid_grad) {
    const size_t pixels = (size_t)v.height * (size_t)v.width;
    unsigned long long* const sums_q = static_cast<unsigned long long*>(workspace);
    uint32_t* const max_bits = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + bil_sums_bytes(v.levels, v.rows, v.columns));
    if (hipError_t err = hipMemsetAsync(workspace, 0, bilateral_workspace_bytes(v.levels, v.rows, v.columns), s)) return err;
    const size_t want = (pixels + kBlock - 1) / kBlock;
    const dim3 max_grid((uint32_t)(want < kBilMaxBlocks ? want : kBilMaxBlocks));
    const dim3 tiles((uint32_t)((v.width + kBilTile - 1) / kBilTile), (uint32_t)((v.height + kBilTile - 1) / kBilTile));
    const uint32_t count = 12u * (uint32_t)v.levels * (uint32_t)v.rows * (uint32_t)v.columns;
    hipLaunchKernelGGL(k_bilateral_max_abs, max_grid, dim3(kBlock), 0, s, v, out_grad, max_bits);
    hipLaunchKernelGGL(k_bilateral_backward<true>, tiles, dim3(kBlock), 0, s, v, out_grad, max_bits, rgba_grad, sums_q);
    const BilTv tv{lambda_tv, {tv_coeff[0], tv_coeff[1], tv_coeff[2]}};
    const auto finish = lambda_tv != 0.0f ? k_bilateral_finish<true> : k_bilateral_finish<false>;
    hipLaunchKernelGGL(finish, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, s, reinterpret_cast<const long long*>(sums_q), max_bits,
                       (uint64_t)pixels, v.grid, v.levels, v.rows, v.columns, tv, grid_grad);
    return hipSuccess;
}

void launch_bilateral_backward_image(hipStream_t s, const BilView& v, const float* out_grad, float* rgba_grad) {
    const dim3 tiles((uint32_t)((v.width + kBilTile - 1) / kBilTile), (uint32_t)((v.height + kBilTile - 1) / kBilTile));
    hipLaunchKernelGGL(k_bilateral_backward<false>, tiles, dim3(kBlock), 0, s, v, out_grad, static_cast<const uint32_t*>(nullptr), rgba_grad,
                       static_cast<unsigned long long*>(nullptr));
}

void launch_bilateral_adam(hipStream_t s, const float* grad, float* grid, float* m1, float* m2, int32_t* count, uint32_t n, float lr,
                           float beta1, float beta2, float eps) {
    const uint32_t want = (n + (uint32_t)kBlock - 1u) / (uint32_t)kBlock;
    hipLaunchKernelGGL(k_bilateral_adam, dim3(want < kBilAdamBlocks ? want : kBilAdamBlocks), dim3(kBlock), 0, s, grad, grid, m1, m2, count, n,
                       lr, beta1, beta2, eps);
}

}  // namespace gut
