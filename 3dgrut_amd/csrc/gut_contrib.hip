// gut_contrib.hip — per-Gaussian contribution scores of a view (gut_trace_contribution) for gfx950 (wave64).
//
// k_contribution re-walks what the forward compositor (k_render, gut_render.hip) walked — one 256-thread workgroup per 16x16 tile, one
// lane per pixel, the tile's ordered-id list in chunks of 256 entries staged in LDS, bounded by the forward's per-tile walked depth as
// the backward compositor bounds it — and takes the forward's decisions by the forward's arithmetic: the per-(pixel, entry) evaluation
// below is a copy of k_render's without the colours, and this unit is built with the flags of gut_render.hip, so the compiler contracts
// the same expressions (the one place where it does not is pinned with explicit FMAs, see `entry`).  It reads no colours and writes no image.  Where the forward composited, w = T_before * alpha; 0 elsewhere.
//
// Per (tile, entry) the 256 values of w are reduced to their sum, their maximum and the number of them above zero in a FIXED order:
// inside a wave a DPP tree (the lane pairing of every step is fixed), the four waves' partials in their own LDS slots
// [wave][entry], combined in wave order ((w0 + w1) + w2) + w3 after the chunk's walk.  No LDS float atomics: their arrival order is
// not fixed.  An entry no pixel composited issues nothing; the others add into the caller's 16-byte GutContribution record with
// integer atomics only (the sum as round(sum * 2^32) in 64 bits), so the totals do not depend on the order in which tiles or views
// arrive: identical inputs give identical bits.
//
// The weighted form (gut_trace_contribution_weighted) is the same walk with one more factor: each lane loads its pixel's
// value e of a caller plane once, clamped to [0, 1], multiplies the weight `entry` returns by it AFTERWARDS (the evaluation itself is
// untouched), and w * e goes through the same tree, its own LDS plane and the same wave order into a uint64 array of the caller's.
//
// The attribute form (gut_trace_attributes) is the walk in the other direction: per-Gaussian values are staged with the
// entries and every lane sums w * value over the entries its pixel composited, in list order, in its own registers, and writes the
// sums to the caller's planes: no reduction across lanes, no partials, no atomics.
//
// The attribute gradient (gut_trace_attributes_bwd) is the adjoint of that form and the weighted form without its
// clamp, four signed channels per walk: each lane loads its pixel's cotangent of the channel group once, every w * g[k] is rounded on
// its own and goes through the tree, per-wave LDS slots and the wave order, and the flush adds round(sum * 2^s_k) with a 64-bit integer
// atomic into a scratch row of the handle's, s_k a power of two from the largest |g[k]| of the plane (k_plane_max_abs).  k_grad_rows
// turns the integers into the caller's float rows.
#include "gut_internal.h"
#include "gut_render_common.h"

#include <algorithm>
#include <type_traits>

namespace gut {

namespace {

// the staged entry of k_render (gut_render.hip) without its colour: the thirteen floats of every (pixel, entry) test, the scales (read
// by hits only) and the particle id
struct ContribEntry {  // 64 bytes
    float4 q0;         // oc = M (sensor_pos - mean), density
    float4 q1;         // m00 m01 m02 m10
    float4 q2;         // m11 m12 m20 m21
    float4 q3;         // s.x s.y s.z m22
};

__device__ __forceinline__ const ContribEntry& stage_at(const ContribEntry* stage, uint32_t j) {
    return *reinterpret_cast<const ContribEntry*>(reinterpret_cast<const char*>(stage) + __umul24(j, (uint32_t)sizeof(ContribEntry)));
}

template <int kCtrl, int kRowMask>
__device__ __forceinline__ float dpp_add(float v) {
    const int moved = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), kCtrl, kRowMask, 0xF, true);
    return v + __builtin_bit_cast(float, moved);
}
template <int kCtrl, int kRowMask>
__device__ __forceinline__ float dpp_max(float v) {   // v >= 0: the 0 a lane without a source reads is neutral
    const int moved = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), kCtrl, kRowMask, 0xF, true);
    return fmaxf(v, __builtin_bit_cast(float, moved));
}
// sum / maximum over the 64 lanes of the wave, in a fixed tree; the result ends up in lane 63 (as wave_sum_lane63 of gut_render.hip)
__device__ __forceinline__ float wave_sum_lane63(float v) {
    v = dpp_add<0x111, 0xF>(v);  // row_shr:1
    v = dpp_add<0x112, 0xF>(v);  // row_shr:2
    v = dpp_add<0x114, 0xF>(v);  // row_shr:4
    v = dpp_add<0x118, 0xF>(v);  // row_shr:8   -> lane 15 of every row holds the row total
    v = dpp_add<0x142, 0xA>(v);  // row_bcast:15 into rows 1 and 3
    v = dpp_add<0x143, 0xC>(v);  // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave total
    return v;
}
__device__ __forceinline__ float wave_max_lane63(float v) {
    v = dpp_max<0x111, 0xF>(v);
    v = dpp_max<0x112, 0xF>(v);
    v = dpp_max<0x114, 0xF>(v);
    v = dpp_max<0x118, 0xF>(v);
    v = dpp_max<0x142, 0xA>(v);
    v = dpp_max<0x143, 0xC>(v);
    return v;
}

constexpr uint32_t kWaves = kBlock / 64;

// the attribute walk's operands (gut_trace_attributes), of one channel group
struct AttrArgs {
    const float* rows;   // the group's first channel of row 0
    float* out;          // the group's first plane
    uint32_t stride;     // floats per row: the number of channels
    uint32_t cols;       // channels of this group, 1..4
    uint32_t vec16;      // every row of the group starts on a 16-byte boundary and has four channels: one 16-byte load
};
struct NoAttrArgs {};

// the attribute gradient's operands (gut_trace_attributes_bwd), of one channel group
struct GradArgs {
    const float* planes;        // the group's first cotangent plane [H,W]
    long long* rows_q;          // [N,4] fixed-point sums, zeroed by the caller per group
    const uint32_t* max_bits;   // [4]: the float bits of the largest finite |g| of each of the group's planes (k_plane_max_abs)
    uint32_t cols;              // channels of this group, 1..4
};

// The exponent s of the fixed-point unit 2^-s of a plane whose largest finite |g| has the bits max_bits: |g| < 2^e with e read from
// the exponent field, and s = 40 - e less the bits by which the view has more than 2^14 tiles.  A tile's sum of 256 products w g
// (w <= 1) is then below 2^48 (+ its rounding) and a row's total over all the tiles below 2^62.  Clamped so that 2^s and 2^-s are
// normal floats; a plane of zeros takes s = 0 (every product is 0).
__device__ __forceinline__ int grad_scale_exponent(uint32_t max_bits, uint32_t tiles) {
    if (max_bits == 0u) return 0;
    const int e = max((int)(max_bits >> 23), 1) - 126;
    const int extra = max(32 - (int)__clz((int)(tiles - 1u)) - 14, 0);   // ceil(log2(tiles)) - 14
    return min(max(40 - e - (tiles > 1u ? extra : 0), -126), 126);
}
__device__ __forceinline__ float pow2f(int s) { return __uint_as_float((uint32_t)(s + 127) << 23); }   // s in -126..126
__device__ __forceinline__ float finite_or_zero(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u ? 0.0f : x; }

// kPlain: the GutContribution records (sum, maximum, count of w).  kWeighted: the sum of w * e into weighted_q32, e the pixel's value
// of `plane` clamped to [0, 1].  <true, false> is the kernel of §13; the other two read `plane`, <false, true>
// writes no record (scores is not read).
// kAttr (1 or 4, with neither of the others): the walk renders per-Gaussian attributes.  Thread j also stages entry
// j's values of the channel group (of a group of four the first attr.cols; one 16-byte load where attr.vec16 says the rows allow
// it); a lane that composited entry j with w > 0 adds w x those values to its pixel's sums, which go to the planes
// attr.out[k][H][W], every pixel of the tile.  No partials and no flush.  The mode's operands travel in one trailing argument,
// empty in the other modes: their kernels keep their argument layout and their code.
// kGrad (1 or 4, with none of the others): the adjoint of kAttr.  Each lane holds its pixel's cotangent g[k] of the
// channel group (a non-finite value and a pixel outside the image count as 0, no clamp); per (wave, entry) some lane composited,
// w * g[k] is rounded on its own, reduced by the tree into the wave's LDS slot, and thread j's flush combines the waves' slots of
// entry j in wave order and adds round(sum * 2^s_k) to the Gaussian's row of grad.rows_q with a 64-bit integer atomic.
template <bool kPlain, bool kWeighted, int kAttr = 0, int kGrad = 0>
__global__ __launch_bounds__(kBlock, 4) void k_contribution(ViewParams v, RenderConsts c, const float4* __restrict__ density12,
                                                           const float* __restrict__ ray_ori, const float* __restrict__ ray_dir,
                                                           const uint2* __restrict__ ranges, const uint32_t* __restrict__ ordered_ids,
                                                           const uint32_t* __restrict__ tile_order,
                                                           const uint32_t* __restrict__ tile_walked, uint32_t num_particles,
                                                           GutContribution* __restrict__ scores, const float* __restrict__ plane,
                                                           unsigned long long* __restrict__ weighted_q32,
                                                           std::conditional_t<kAttr != 0, AttrArgs, std::conditional_t<kGrad != 0, GradArgs, NoAttrArgs>> attr) {
    static_assert(kGrad != 0 ? ((kGrad == 1 || kGrad == 4) && kAttr == 0 && !kPlain && !kWeighted)
                  : kAttr == 0 ? (kPlain || kWeighted) : ((kAttr == 1 || kAttr == 4) && !kPlain && !kWeighted), "nothing to write");
    using AttrSlot = std::conditional_t<kAttr == 1, float, float4>;
    using GradSlot = std::conditional_t<kGrad == 1, float, float4>;
    __shared__ ContribEntry stage[kBlock];
    __shared__ uint32_t s_id[kBlock];
    __shared__ uint32_t s_first_invalid;
    __shared__ uint32_t s_mask[kBlock];              // see k_render
    __shared__ uint16_t s_list[kWaves][kBlock];      // see k_render
    __shared__ StripPlanes s_planes;
    // the waves' partials of the chunk: written by lane 63 of wave w for the entries some pixel of the wave composited; s_cnt is zeroed
    // per chunk and says which of the others are valid (s_wsum: the weighted sums)
    __shared__ float s_sum[kPlain ? kWaves : 1][kPlain ? kBlock : 1], s_max[kPlain ? kWaves : 1][kPlain ? kBlock : 1];
    __shared__ float s_wsum[kWeighted ? kWaves : 1][kWeighted ? kBlock : 1];
    __shared__ uint32_t s_cnt[(kAttr || kGrad) ? 1 : kWaves][(kAttr || kGrad) ? 1 : kBlock];
    // kGrad: the waves' sums of w * g[k] of the chunk; s_hit (zeroed per chunk) says which slots are valid
    __shared__ GradSlot s_gsum[kGrad ? kWaves : 1][kGrad ? kBlock : 1];
    __shared__ uint8_t s_hit[kGrad ? kWaves : 1][kGrad ? kBlock : 4];
    __shared__ AttrSlot s_attr[kAttr ? kBlock : 1];   // entry j's values of the channel group

    const uint32_t tile = tile_order[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const int px = (int)(tile % (uint32_t)v.grid_x) * kTile + tile_px(tid);   // wave = 8x8 block (gut_render_common.h)
    const int py = (int)(tile / (uint32_t)v.grid_x) * kTile + tile_py(tid);
    const bool inside = (px < v.width) && (py < v.height);
    const size_t pix = (size_t)py * (size_t)v.width + (size_t)px;
    const RayState ray = make_ray(v, ray_ori, ray_dir, pix, inside);
    // the pixel's weight, once: clamped on load, so a NaN counts as 0, every w * e lies in [0, w] and a tile's sum stays below 256
    float e = 0.0f;
    if constexpr (kWeighted) e = fminf(fmaxf(inside ? plane[pix] : 0.0f, 0.0f), 1.0f);
    // kGrad: the pixel's cotangent of the channel group, once, and the planes' fixed-point scales 2^s_k (block-uniform)
    float g[kGrad ? kGrad : 1] = {};
    float q_scale[kGrad ? kGrad : 1] = {};
    if constexpr (kGrad != 0) {
        const size_t plane_stride = (size_t)v.width * (size_t)v.height;
        const uint32_t tiles = (uint32_t)(v.grid_x * v.grid_y);
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)kGrad; ++k) {
            if (k < attr.cols) {
                if (inside) g[k] = finite_or_zero(attr.planes[k * plane_stride + pix]);
                q_scale[k] = pow2f(grad_scale_exponent(attr.max_bits[k], tiles));
            }
        }
    }

    if (tid == 0) s_first_invalid = kBlock;
    const bool centred = __syncthreads_and(ray.centred ? 1 : 0) != 0;  // block-uniform
    build_strip_planes(s_planes, ray, inside, centred, tid);
    const uint32_t wave_bit = 1u << (tid >> 6);
    const uint32_t wave = tid >> 6, lane = tid & 63u;

    uint2 range = ranges[tile];
    // no further than the forward walked (k_render_backward bounds its walk the same way): nothing behind that position was
    // composited, and with the lazy order only that prefix of the ordered-id list is ordered at all
    range.y = range.x + min(range.y - range.x, tile_walked[tile]);
    const uint32_t total = range.y - range.x;
    float T = ray.valid ? 1.0f : -1.0f;   // alive <=> T > 0; a ray that ends keeps -T (k_render)
    float acc[kAttr ? kAttr : 1] = {};    // kAttr: the pixel's sums of w x attribute

    auto walk = [&](auto centred_tag) __attribute__((always_inline)) {
    constexpr bool kCentred = decltype(centred_tag)::value;
    for (uint32_t base = 0; base < total; base += kBlock) {
        if (!__syncthreads_or(T > 0.0f ? 1 : 0)) break;  // whole tile terminated
        {
            const uint32_t k = range.x + base + tid;
            uint32_t id = kInvalid;
            if (k < range.y) id = ordered_ids[k];
            if (id != kInvalid && id >= num_particles) id = kInvalid;   // (never in a list the forward built: keeps every access in bounds)
            ContribEntry e;
            uint32_t strips = 0xFu;
            if (id != kInvalid) {
                const float4 a = density12[3 * (size_t)id + 0];
                const float4 q = density12[3 * (size_t)id + 1];
                const float4 s = density12[3 * (size_t)id + 2];
                float r[3][3];
                quat_rows(q.x, q.y, q.z, q.w, r);
                const float i0 = 1.0f / s.x, i1 = 1.0f / s.y, i2 = 1.0f / s.z;
                const float m00 = r[0][0] * i0, m01 = r[0][1] * i0, m02 = r[0][2] * i0;
                const float m10 = r[1][0] * i1, m11 = r[1][1] * i1, m12 = r[1][2] * i1;
                const float m20 = r[2][0] * i2, m21 = r[2][1] * i2, m22 = r[2][2] * i2;
                const float c0 = v.s2w.t[0] - a.x, c1 = v.s2w.t[1] - a.y, c2 = v.s2w.t[2] - a.z;
                e.q0 = make_float4(m00 * c0 + m01 * c1 + m02 * c2, m10 * c0 + m11 * c1 + m12 * c2, m20 * c0 + m21 * c1 + m22 * c2, a.w);
                e.q1 = make_float4(m00, m01, m02, m10);
                e.q2 = make_float4(m11, m12, m20, m21);
                e.q3 = make_float4(s.x, s.y, s.z, m22);
                strips = strip_mask<false>(s_planes, v, c, a, r, s, 2);
            }
            stage[tid] = e;
            s_id[tid] = id;
            s_mask[tid] = strips;
            if constexpr (kGrad != 0) {
#pragma unroll
                for (uint32_t w = 0; w < kWaves; ++w) s_hit[w][tid] = 0u;
            } else if constexpr (kAttr == 0) {
#pragma unroll
                for (uint32_t w = 0; w < kWaves; ++w) s_cnt[w][tid] = 0u;
            } else if constexpr (kAttr == 1) {
                s_attr[tid] = id != kInvalid ? attr.rows[(size_t)id * attr.stride] : 0.0f;
            } else {
                float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (id != kInvalid) {
                    const float* const row = attr.rows + (size_t)id * attr.stride;
                    if (attr.vec16 != 0u) {
                        a = *reinterpret_cast<const float4*>(row);
                    } else {   // never past the row's end: the last group of a K that is no multiple of four
                        a.x = row[0];
                        if (attr.cols > 1u) a.y = row[1];
                        if (attr.cols > 2u) a.z = row[2];
                        if (attr.cols > 3u) a.w = row[3];
                    }
                }
                s_attr[tid] = a;
            }
            if (id == kInvalid && k < range.y) atomicMin(&s_first_invalid, tid);
        }
        __syncthreads();

        const uint32_t cnt_all = min((uint32_t)kBlock, total - base);
        const uint32_t cnt = min(cnt_all, s_first_invalid);  // padding ids end the list for everyone
        // k_render's evaluation of one entry for this lane's pixel; returns the weight it composited with (0: it did not)
        // The three products u = M d are written with explicit fused multiply-adds: for `a x + b y + c z` the compiler is free to
        // round either of the first two products on its own, and in k_render it does so differently in the two copies of the
        // evaluation its unrolled-by-two pipeline has (odd and even positions of the wave's list: seen in the ISA of both of its
        // instantiations) — and differently again in a copy of the same source here.  kSecond names the copy; with the forms pinned
        // the sum of the pixel counts equals the forward's hit-count plane.  Everything else contracts as in k_render.
        auto entry = [&](auto second_tag, const float4& cs, const float4& q1, const float4& q2, const float m22, const uint32_t j)
                         __attribute__((always_inline)) -> float {
            constexpr bool kSecond = decltype(second_tag)::value;
            float wout = 0.0f;
            if (T > 0.0f) {
                float o0 = cs.x, o1 = cs.y, o2 = cs.z;
                if (!kCentred) {
                    o0 += q1.x * ray.ex + q1.y * ray.ey + q1.z * ray.ez;
                    o1 += q1.w * ray.ex + q2.x * ray.ey + q2.y * ray.ez;
                    o2 += q2.z * ray.ex + q2.w * ray.ey + m22 * ray.ez;
                }
                const float u0 = kSecond ? __builtin_fmaf(q1.z, ray.dz, __builtin_fmaf(q1.x, ray.dx, q1.y * ray.dy))
                                         : __builtin_fmaf(q1.z, ray.dz, __builtin_fmaf(q1.y, ray.dy, q1.x * ray.dx));
                const float u1 = __builtin_fmaf(q2.y, ray.dz, __builtin_fmaf(q1.w, ray.dx, q2.x * ray.dy));
                const float u2 = kSecond ? __builtin_fmaf(m22, ray.dz, __builtin_fmaf(q2.z, ray.dx, q2.w * ray.dy))
                                         : __builtin_fmaf(m22, ray.dz, __builtin_fmaf(q2.w, ray.dy, q2.z * ray.dx));
                const float x0 = u1 * o2 - u2 * o1, x1 = u2 * o0 - u0 * o2, x2 = u0 * o1 - u1 * o0;
                const float l2 = u0 * u0 + u1 * u1 + u2 * u2;
                const float il2 = fast_rcp(l2);
                const float d2 = (x0 * x0 + x1 * x1 + x2 * x2) * il2;  // |grd x gro|^2 with grd = u/|u|
                if (d2 < c.max_d2) {
                    const float resp = fast_exp(-0.5f * d2);
                    const float alpha = fminf(c.max_alpha, resp * cs.w);
                    if ((resp > c.min_response) && (alpha > c.alpha_threshold)) {
                        // hitT = | s * grd * (grd . -gro) |
                        const float proj = -(u0 * o0 + u1 * o1 + u2 * o2) * il2;  // (grd.-gro)/|u|
                        const float4 sc = stage_at(stage, j).q3;                   // the scales: read by hits only
                        const float h0 = sc.x * u0 * proj, h1 = sc.y * u1 * proj, h2 = sc.z * u2 * proj;
                        const float hit_t = fast_sqrt(h0 * h0 + h1 * h1 + h2 * h2);
                        if ((hit_t > ray.tmin) && (hit_t < ray.tmax)) {
                            const float w = alpha * T;
                            T *= (1.0f - alpha);
                            wout = w;
                            if (T < c.min_transmittance) T = -T;   // the ray ends here
                        }
                    }
                }
            }
            return wout;
        };
        // the wave's reduction of one entry's weights into its own slots (wave-uniform branch: nothing where no pixel composited)
        auto reduce = [&](const float w, const uint32_t j) __attribute__((always_inline)) {
            if constexpr (kAttr != 0) {
                // the lanes that composited read one address, a broadcast; an entry nobody composited is never multiplied in
                if (w > 0.0f) {
                    if constexpr (kAttr == 1) {
                        acc[0] = __builtin_fmaf(w, s_attr[j], acc[0]);
                    } else {
                        const float4 a = s_attr[j];
                        acc[0] = __builtin_fmaf(w, a.x, acc[0]);
                        acc[1] = __builtin_fmaf(w, a.y, acc[1]);
                        acc[2] = __builtin_fmaf(w, a.z, acc[2]);
                        acc[3] = __builtin_fmaf(w, a.w, acc[3]);
                    }
                }
                return;
            }
            const unsigned long long hit = __ballot(w > 0.0f);
            if (hit == 0ull) return;
            if constexpr (kGrad != 0) {
                // every product rounded on its own (see kWeighted below), every channel through its own tree
                float sums[kGrad];
#pragma unroll
                for (int k = 0; k < kGrad; ++k) {
                    float wg = w * g[k];
                    asm volatile("" : "+v"(wg));
                    sums[k] = wave_sum_lane63(wg);
                }
                if (lane == 63u) {
                    if constexpr (kGrad == 1) s_gsum[wave][j] = sums[0];
                    else s_gsum[wave][j] = make_float4(sums[0], sums[1], sums[2], sums[3]);
                    s_hit[wave][j] = 1u;
                }
                return;
            }
            if constexpr (kPlain) {
                const float sum = wave_sum_lane63(w), mx = wave_max_lane63(w);
                if (lane == 63u) {
                    s_sum[wave][j] = sum;
                    s_max[wave][j] = mx;
                }
            }
            if constexpr (kWeighted) {
                // the product is rounded on its own in every instantiation: behind the empty asm the first add of the tree cannot
                // be contracted with it into a fused multiply-add
                float we = w * e;
                asm volatile("" : "+v"(we));
                const float wsum = wave_sum_lane63(we);
                if (lane == 63u) s_wsum[wave][j] = wsum;
            }
            if (lane == 63u) s_cnt[wave][j] = (uint32_t)__popcll(hit);
        };
        // as in k_render: the wave compacts the chunk to the entries that can reach its 8x8 block, then walks that list with the
        // two-register-set software pipeline
        {
            uint16_t* list = s_list[wave];
            uint32_t nw = 0;
#pragma unroll
            for (uint32_t r = 0; r < kWaves; ++r) {
                const uint32_t e = r * 64u + lane;
                const bool keep = (e < cnt) && ((s_mask[e] & wave_bit) != 0u);
                const unsigned long long bal = __ballot(keep);
                if (keep) list[nw + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)e;
                nw += (uint32_t)__popcll(bal);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            uint32_t ja = list[0], jb = list[1];  // list positions i and i+1 (garbage beyond nw is never evaluated)
            ja = min(ja, (uint32_t)kBlock - 1u);
            jb = min(jb, (uint32_t)kBlock - 1u);
            float4 a0 = stage_at(stage, ja).q0, a1 = stage_at(stage, ja).q1, a2 = stage_at(stage, ja).q2;
            float a3 = stage_at(stage, ja).q3.w;
            float4 b0, b1, b2;
            float b3;
            uint32_t i = 0;
            while (i < nw) {
                if (__ballot(T > 0.0f) == 0ull) break;  // wave-uniform
                b0 = stage_at(stage, jb).q0; b1 = stage_at(stage, jb).q1; b2 = stage_at(stage, jb).q2; b3 = stage_at(stage, jb).q3.w;
                const uint32_t jc = min((uint32_t)list[min(i + 2, (uint32_t)kBlock - 1)], (uint32_t)kBlock - 1u);
                reduce(entry(std::false_type{}, a0, a1, a2, a3, ja), ja);
                if (++i >= nw) break;
                if (__ballot(T > 0.0f) == 0ull) break;
                a0 = stage_at(stage, jc).q0; a1 = stage_at(stage, jc).q1; a2 = stage_at(stage, jc).q2; a3 = stage_at(stage, jc).q3.w;
                const uint32_t jd = min((uint32_t)list[min(i + 2, (uint32_t)kBlock - 1)], (uint32_t)kBlock - 1u);
                reduce(entry(std::true_type{}, b0, b1, b2, b3, jb), jb);
                ++i;
                ja = jc;
                jb = jd;
            }
        }
        if (cnt < cnt_all) T = -fabsf(T);  // list ended at a padding entry

        // ---- flush: thread j combines the four waves' partials of entry j in wave order and adds them to the Gaussian's record ----
        // (kAttr: nothing to flush; the barrier at the head of the loop stands between this chunk's reads and the next staging)
        if constexpr (kGrad != 0) {
        __syncthreads();
        if (tid < cnt) {
            bool any = false;
            float sum[kGrad] = {};
#pragma unroll
            for (uint32_t w = 0; w < kWaves; ++w) {
                if (s_hit[w][tid] != 0u) {
                    any = true;
                    const GradSlot p = s_gsum[w][tid];
                    if constexpr (kGrad == 1) {
                        sum[0] += p;
                    } else {
                        sum[0] += p.x; sum[1] += p.y; sum[2] += p.z; sum[3] += p.w;
                    }
                }
            }
            if (any) {
                // |sum| < 2^-s 2^48 (grad_scale_exponent): the product is exact in fp32 (a power-of-two scale), the conversion rounds
                // to nearest, ties to even; the signed value is added in two's complement
                long long* const row = attr.rows_q + 4 * (size_t)s_id[tid];
#pragma unroll
                for (int k = 0; k < kGrad; ++k) {
                    const long long q = __float2ll_rn(sum[k] * q_scale[k]);
                    if (q != 0ll) atomicAdd(reinterpret_cast<unsigned long long*>(row + k), (unsigned long long)q);
                }
            }
        }
        } else if constexpr (kAttr == 0) {
        __syncthreads();
        if (tid < cnt) {
            uint32_t pixels = 0;
            float sum = 0.0f, mx = 0.0f, wsum = 0.0f;
#pragma unroll
            for (uint32_t w = 0; w < kWaves; ++w) {
                const uint32_t n = s_cnt[w][tid];
                if (n != 0u) {
                    pixels += n;
                    if constexpr (kPlain) {
                        sum += s_sum[w][tid];
                        mx = fmaxf(mx, s_max[w][tid]);
                    }
                    if constexpr (kWeighted) wsum += s_wsum[w][tid];
                }
            }
            if (pixels != 0u) {
                // a tile's sum is at most 256: the product is below 2^41 and exact in fp32 (a power-of-two scale), the conversion rounds to nearest
                if constexpr (kPlain) {
                    GutContribution* const row = scores + s_id[tid];
                    atomicAdd(reinterpret_cast<unsigned long long*>(&row->weight_sum_q32), __float2ull_rn(sum * 4294967296.0f));
                    atomicMax(&row->max_weight_bits, __float_as_uint(mx));
                    atomicAdd(&row->pixels, pixels);
                }
                if constexpr (kWeighted) {
                    if (wsum > 0.0f) atomicAdd(weighted_q32 + s_id[tid], __float2ull_rn(wsum * 4294967296.0f));
                }
            }
        }
        }
        // (the next chunk's staging starts behind the barrier at the head of the loop)
    }
    };
    if (centred) walk(std::true_type{}); else walk(std::false_type{});
    if constexpr (kAttr != 0) {
        // every pixel of the image, 0 where nothing was composited: the planes need no initialisation
        if (inside) {
            const size_t plane_stride = (size_t)v.width * (size_t)v.height;
            float* const out = attr.out;
            out[pix] = acc[0];
            if constexpr (kAttr == 4) {
                if (attr.cols > 1u) out[plane_stride + pix] = acc[1];
                if (attr.cols > 2u) out[2 * plane_stride + pix] = acc[2];
                if (attr.cols > 3u) out[3 * plane_stride + pix] = acc[3];
            }
        }
    }
}

// the largest finite |g| of each of a group's planes, as float bits (non-negative floats order as their bits): blockIdx.y is the plane
__global__ __launch_bounds__(kBlock) void k_plane_max_abs(const float* __restrict__ planes, size_t plane_stride, uint32_t* __restrict__ max_bits) {
    const float* const plane = planes + (size_t)blockIdx.y * plane_stride;
    float m = 0.0f;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < plane_stride; i += (size_t)gridDim.x * kBlock)
        m = fmaxf(m, fabsf(finite_or_zero(plane[i])));
    m = wave_max_lane63(m);
    if ((threadIdx.x & 63u) == 63u && m > 0.0f) atomicMax(max_bits + blockIdx.y, __float_as_uint(m));
}

// row i of the caller's gradient [N, stride], channels first .. first + cols: float(q) * 2^-s_k; every element of the group is written
__global__ __launch_bounds__(kBlock) void k_grad_rows(const long long* __restrict__ rows_q, const uint32_t* __restrict__ max_bits,
                                                      uint32_t tiles, uint32_t n, uint32_t cols, uint32_t stride, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const long long* const q = rows_q + 4 * (size_t)i;
    float* const row = out + (size_t)i * stride;
    for (uint32_t k = 0; k < cols; ++k) row[k] = __ll2float_rn(q[k]) * pow2f(-grad_scale_exponent(max_bits[k], tiles));
}

}  // namespace

void launch_contribution(hipStream_t s, const ViewParams& v, const RenderConsts& c, const float* density12, const float* ray_ori,
                         const float* ray_dir, const uint32_t* ranges, const uint32_t* ordered_ids, const uint32_t* tile_order,
                         const uint32_t* tile_walked, uint32_t num_particles, GutContribution* scores, const float* plane,
                         uint64_t* weighted_q32) {
    const uint32_t tiles = (uint32_t)(v.grid_x * v.grid_y);
    if (tiles == 0) return;
    // no plane: the records alone; a plane: its weighted sums, with the records in the same walk where the caller wants them
    const auto kernel = !plane ? k_contribution<true, false> : scores ? k_contribution<true, true> : k_contribution<false, true>;
    hipLaunchKernelGGL(kernel, dim3(tiles), dim3(kBlock), 0, s, v, c, reinterpret_cast<const float4*>(density12), ray_ori, ray_dir,
                       reinterpret_cast<const uint2*>(ranges), ordered_ids, tile_order, tile_walked, num_particles, scores, plane,
                       reinterpret_cast<unsigned long long*>(weighted_q32), NoAttrArgs{});
}

void launch_attributes(hipStream_t s, const ViewParams& v, const RenderConsts& c, const float* density12, const float* ray_ori,
                       const float* ray_dir, const uint32_t* ranges, const uint32_t* ordered_ids, const uint32_t* tile_order,
                       const uint32_t* tile_walked, uint32_t num_particles, uint32_t num_channels, const float* attrs, float* out) {
    const uint32_t tiles = (uint32_t)(v.grid_x * v.grid_y);
    if (tiles == 0) return;
    const size_t plane_stride = (size_t)v.width * (size_t)v.height;
    // one walk per group of four channels; a last group of one channel takes the single-channel kernel.  The 16-byte gather where
    // every row of the group starts on a 16-byte boundary, decided from the pointer here
    const bool aligned = (num_channels % 4u) == 0u && ((uintptr_t)attrs & 15u) == 0u;
    for (uint32_t first = 0; first < num_channels; first += 4u) {
        const uint32_t cols = num_channels - first < 4u ? num_channels - first : 4u;
        const AttrArgs a{attrs + first, out + (size_t)first * plane_stride, num_channels, cols, aligned && cols == 4u ? 1u : 0u};
        const auto kernel = cols == 1u ? k_contribution<false, false, 1> : k_contribution<false, false, 4>;
        hipLaunchKernelGGL(kernel, dim3(tiles), dim3(kBlock), 0, s, v, c, reinterpret_cast<const float4*>(density12), ray_ori, ray_dir,
                           reinterpret_cast<const uint2*>(ranges), ordered_ids, tile_order, tile_walked, num_particles,
                           (GutContribution*)nullptr, (const float*)nullptr, (unsigned long long*)nullptr, a);
    }
}

void launch_attributes_bwd(hipStream_t s, const ViewParams& v, const RenderConsts& c, const float* density12, const float* ray_ori,
                           const float* ray_dir, const uint32_t* ranges, const uint32_t* ordered_ids, const uint32_t* tile_order,
                           const uint32_t* tile_walked, uint32_t num_particles, uint32_t num_channels, const float* out_grad,
                           float* attrs_grad, void* rows_q, uint32_t* max_bits) {
    const uint32_t tiles = (uint32_t)(v.grid_x * v.grid_y);
    if (tiles == 0 || num_particles == 0) return;
    const size_t plane_stride = (size_t)v.width * (size_t)v.height;
    const uint32_t max_blocks = (uint32_t)std::min<size_t>((plane_stride + kBlock - 1) / kBlock, 256);
    const uint32_t row_blocks = (num_particles + kBlock - 1) / kBlock;
    // per group of four channels: the planes' maxima, the walk into the zeroed fixed-point rows, the rows into the caller's floats
    for (uint32_t first = 0; first < num_channels; first += 4u) {
        const uint32_t cols = num_channels - first < 4u ? num_channels - first : 4u;
        const GradArgs a{out_grad + (size_t)first * plane_stride, static_cast<long long*>(rows_q), max_bits, cols};
        (void)hipMemsetAsync(max_bits, 0, 4 * sizeof(uint32_t), s);
        (void)hipMemsetAsync(rows_q, 0, 4 * sizeof(long long) * (size_t)num_particles, s);
        hipLaunchKernelGGL(k_plane_max_abs, dim3(max_blocks, cols), dim3(kBlock), 0, s, a.planes, plane_stride, max_bits);
        const auto kernel = cols == 1u ? k_contribution<false, false, 0, 1> : k_contribution<false, false, 0, 4>;
        hipLaunchKernelGGL(kernel, dim3(tiles), dim3(kBlock), 0, s, v, c, reinterpret_cast<const float4*>(density12), ray_ori, ray_dir,
                           reinterpret_cast<const uint2*>(ranges), ordered_ids, tile_order, tile_walked, num_particles,
                           (GutContribution*)nullptr, (const float*)nullptr, (unsigned long long*)nullptr, a);
        hipLaunchKernelGGL(k_grad_rows, dim3(row_blocks), dim3(kBlock), 0, s, a.rows_q, max_bits, tiles, num_particles, cols, num_channels,
                           attrs_grad + first);
    }
}

}  // namespace gut
