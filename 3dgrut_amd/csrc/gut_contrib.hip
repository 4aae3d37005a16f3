// gut_contrib.hip — the forward's walk once more, and what is done with its blending weights (DESIGN.md §13–§15, §17), for gfx950
// (wave64).
//
// THE WALK.  k_walk re-walks what the forward compositor (k_render, gut_render.hip) walked — one 256-thread workgroup per 16x16 tile,
// one lane per pixel, the tile's ordered-id list in chunks of 256 entries staged in LDS, bounded by the forward's per-tile walked
// depth as the backward compositor bounds it — and takes the forward's decisions by the forward's arithmetic: the per-(pixel, entry)
// evaluation below is a copy of k_render's without the colours, and this unit is built with the flags of gut_render.hip, so the
// compiler contracts the same expressions (the one place where it does not is pinned with explicit FMAs, see `entry`).  The pixel
// layout (tile_pixel), the staged entry (TestEntry: k_render's PackEntry without the colour and id), stage_at, the strip culling and
// the per-wave compaction (compact_wave_list) are the compositors' own, from gut_render_common.h; the walk loop and `entry` are this
// kernel's, and so is the conversion of a list entry in its staging (see there for why not make_entry).  It reads no
// colours and writes no image.  Where the forward composited, w = T_before * alpha; 0 elsewhere.  The walk names no form: every
// evaluated (pixel, entry) weight goes to a SINK, a struct with its operands (Args, by value), its LDS (Shared, declared once by
// the kernel), its per-lane state and one hook per place where the forms differ:
//     Sink(args, shared, v, pix, inside)   per-lane set-up from the pixel
//     stage(tid, id)                       per-thread staging of the chunk's entry tid (its own barrier-protected LDS)
//     accept(w, j, wave, lane)             per evaluated entry j of the chunk, all 64 lanes of the wave, w = 0 where not composited
//     kWantsHit, hit(w, hit_t, t_after, id)  at the place where the lane's pixel composites an entry: its weight, its hit distance
//                                          as `entry` formed it and |T| behind it (compiled in for a sink that asks for it only)
//     kFlush, flush(j, s_id)               after a chunk's walk, behind a barrier, thread j < the chunk's count
//     finish(v, pix, inside)               after the tile's walk
//
// THE REDUCING SINKS (ScoreSink, GradientSink) reduce the 256 values of a (tile, entry) in a FIXED order: inside a wave the DPP tree
// of gut_render_common.h (the lane pairing of every step is fixed; never the shuffle form), the four waves' partials in their own
// LDS slots [wave][entry], combined in wave order ((w0 + w1) + w2) + w3 by the flush.  No LDS float atomics: their arrival order
// is not fixed.  An entry no pixel composited issues nothing; the others reach the caller's memory with integer atomics only, so
// the totals do not depend on the order in which tiles or views arrive: identical inputs give identical bits.
//
// ScoreSink<kPlain, kWeighted> (gut_trace_contribution, §13; gut_trace_contribution_weighted, §14).  kPlain: the sum, the maximum and
// the number above zero of the weights into the caller's 16-byte GutContribution record (the sum as round(sum * 2^32) in 64 bits).
// kWeighted: each lane loads its pixel's value e of a caller plane once, clamped to [0, 1], multiplies the weight `entry` returns
// by it AFTERWARDS (the evaluation itself is untouched), and w * e, rounded on its own, goes through the same tree, its own LDS
// plane and the same wave order into a uint64 array of the caller's.  <true, false> is the kernel of §13; <false, true> writes no
// record.
//
// AttributeSink<K> (gut_trace_attributes, §15) is the walk in the other direction: thread j stages entry j's values of the channel
// group with the entries (of a group of four the first `cols`; one 16-byte load where the rows allow it) and every lane sums
// w * value over the entries its pixel composited, in list order, in its own registers, and writes the sums to the caller's planes,
// every pixel of the tile: no reduction across lanes, no partials, no flush, no atomics.
//
// GradientSink<K> (gut_trace_attributes_bwd, §17) is the adjoint of that form and the weighted form without its clamp, K signed
// channels per walk: each lane loads its pixel's cotangent g[k] of the channel group once (a non-finite value and a pixel outside
// the image count as 0), every w * g[k] is rounded on its own and goes through the tree, per-wave LDS slots and the wave order, and
// the flush adds round(sum * 2^s_k) with a 64-bit integer atomic into a scratch row of the handle's, s_k a power of two from the
// largest |g[k]| of the plane (k_plane_max_abs).  k_grad_rows turns the integers into the caller's float rows.
//
// SurfaceSink<kMode> (gut_trace_surface, §18) answers "where": per pixel ONE composited entry's hit distance, id and weight, chosen
// in the lane's own registers while the walk passes — the first entry behind which |T| is below a level (GUT_SURFACE_LEVEL; 0.5: the
// median), or the entry of the largest weight (GUT_SURFACE_MAX_WEIGHT).  The only sink that takes the hit hook.  A choice per pixel
// from that pixel's entries alone: no reduction across lanes, no LDS, no flush, no atomics; every pixel of the image is written.
#include "gut_internal.h"
#include "gut_render_common.h"

#include <algorithm>
#include <type_traits>

namespace gut {

namespace {

constexpr uint32_t kWaves = kBlock / 64;

// ---- ScoreSink -------------------------------------------------------------------------------------------------------------------
// the waves' partials of the chunk: written by lane 63 of wave w for the entries some pixel of the wave composited; cnt is zeroed
// per chunk and says which of the others are valid
template <bool> struct PlainSlots {};
template <> struct PlainSlots<true> { float sum[kWaves][kBlock], max[kWaves][kBlock]; };
template <bool> struct WeightedSlots {};
template <> struct WeightedSlots<true> { float wsum[kWaves][kBlock]; };

struct ScoreArgs {
    GutContribution* scores;            // kPlain
    const float* plane;                 // kWeighted
    unsigned long long* weighted_q32;   // kWeighted
};

template <bool kPlain, bool kWeighted>
struct ScoreSink {
    static_assert(kPlain || kWeighted, "nothing to write");
    using Args = ScoreArgs;
    struct Shared : PlainSlots<kPlain>, WeightedSlots<kWeighted> { uint32_t cnt[kWaves][kBlock]; };
    static constexpr bool kFlush = true;
    static constexpr bool kWantsHit = false;

    const Args& a;
    Shared& sh;
    float e = 0.0f;   // the pixel's weight, once: clamped on load, so a NaN counts as 0, every w * e lies in [0, w] and a tile's sum stays below 256

    __device__ __forceinline__ ScoreSink(const Args& args, Shared& shared, const ViewParams&, size_t pix, bool inside) : a(args), sh(shared) {
        if constexpr (kWeighted) e = fminf(fmaxf(inside ? a.plane[pix] : 0.0f, 0.0f), 1.0f);
    }
    __device__ __forceinline__ void stage(uint32_t tid, uint32_t) {
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) sh.cnt[w][tid] = 0u;
    }
    // the wave's reduction of one entry's weights into its own slots (wave-uniform branch: nothing where no pixel composited)
    __device__ __forceinline__ void accept(const float w, const uint32_t j, const uint32_t wave, const uint32_t lane) {
        const unsigned long long hit = __ballot(w > 0.0f);
        if (hit == 0ull) return;
        if constexpr (kPlain) {
            const float sum = dpp_wave_sum_lane63(w), mx = dpp_wave_max_lane63(w);
            if (lane == 63u) {
                sh.sum[wave][j] = sum;
                sh.max[wave][j] = mx;
            }
        }
        if constexpr (kWeighted) {
            // the product is rounded on its own in every instantiation: behind the empty asm the first add of the tree cannot
            // be contracted with it into a fused multiply-add
            float we = w * e;
            asm volatile("" : "+v"(we));
            const float wsum = dpp_wave_sum_lane63(we);
            if (lane == 63u) sh.wsum[wave][j] = wsum;
        }
        if (lane == 63u) sh.cnt[wave][j] = (uint32_t)__popcll(hit);
    }
    // thread j combines the four waves' partials of entry j in wave order and adds them to the Gaussian's record
    __device__ __forceinline__ void flush(const uint32_t j, const uint32_t* s_id) {
        uint32_t pixels = 0;
        float sum = 0.0f, mx = 0.0f, wsum = 0.0f;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) {
            const uint32_t n = sh.cnt[w][j];
            if (n != 0u) {
                pixels += n;
                if constexpr (kPlain) {
                    sum += sh.sum[w][j];
                    mx = fmaxf(mx, sh.max[w][j]);
                }
                if constexpr (kWeighted) wsum += sh.wsum[w][j];
            }
        }
        if (pixels != 0u) {
            // a tile's sum is at most 256: the product is below 2^41 and exact in fp32 (a power-of-two scale), the conversion rounds to nearest
            if constexpr (kPlain) {
                GutContribution* const row = a.scores + s_id[j];
                atomicAdd(reinterpret_cast<unsigned long long*>(&row->weight_sum_q32), __float2ull_rn(sum * 4294967296.0f));
                atomicMax(&row->max_weight_bits, __float_as_uint(mx));
                atomicAdd(&row->pixels, pixels);
            }
            if constexpr (kWeighted) {
                if (wsum > 0.0f) atomicAdd(a.weighted_q32 + s_id[j], __float2ull_rn(wsum * 4294967296.0f));
            }
        }
    }
    __device__ __forceinline__ void finish(const ViewParams&, size_t, bool) {}
};

// ---- AttributeSink: one channel group, K = 1 or 4 --------------------------------------------------------------------------------
struct AttributeArgs {
    const float* rows;   // the group's first channel of row 0
    float* out;          // the group's first plane
    uint32_t stride;     // floats per row: the number of channels
    uint32_t cols;       // channels of this group, 1..4
    uint32_t vec16;      // every row of the group starts on a 16-byte boundary and has four channels: one 16-byte load
};

template <int K>
struct AttributeSink {
    static_assert(K == 1 || K == 4, "a group of one or of up to four channels");
    using Args = AttributeArgs;
    using Slot = std::conditional_t<K == 1, float, float4>;
    struct Shared { Slot attr[kBlock]; };   // entry j's values of the channel group
    // (nothing to flush; the barrier at the head of the chunk loop stands between this chunk's reads and the next staging)
    static constexpr bool kFlush = false;
    static constexpr bool kWantsHit = false;

    const Args& a;
    Shared& sh;
    float acc[K] = {};   // the pixel's sums of w x attribute

    __device__ __forceinline__ AttributeSink(const Args& args, Shared& shared, const ViewParams&, size_t, bool) : a(args), sh(shared) {}
    __device__ __forceinline__ void stage(uint32_t tid, uint32_t id) {
        if constexpr (K == 1) {
            sh.attr[tid] = id != kInvalid ? a.rows[(size_t)id * a.stride] : 0.0f;
        } else {
            float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (id != kInvalid) {
                const float* const row = a.rows + (size_t)id * a.stride;
                if (a.vec16 != 0u) {
                    r = *reinterpret_cast<const float4*>(row);
                } else {   // never past the row's end: the last group of a K that is no multiple of four
                    r.x = row[0];
                    if (a.cols > 1u) r.y = row[1];
                    if (a.cols > 2u) r.z = row[2];
                    if (a.cols > 3u) r.w = row[3];
                }
            }
            sh.attr[tid] = r;
        }
    }
    // the lanes that composited read one address, a broadcast; an entry nobody composited is never multiplied in
    __device__ __forceinline__ void accept(const float w, const uint32_t j, uint32_t, uint32_t) {
        if (w > 0.0f) {
            if constexpr (K == 1) {
                acc[0] = __builtin_fmaf(w, sh.attr[j], acc[0]);
            } else {
                const float4 r = sh.attr[j];
                acc[0] = __builtin_fmaf(w, r.x, acc[0]);
                acc[1] = __builtin_fmaf(w, r.y, acc[1]);
                acc[2] = __builtin_fmaf(w, r.z, acc[2]);
                acc[3] = __builtin_fmaf(w, r.w, acc[3]);
            }
        }
    }
    __device__ __forceinline__ void flush(uint32_t, const uint32_t*) {}
    // every pixel of the image, 0 where nothing was composited: the planes need no initialisation
    __device__ __forceinline__ void finish(const ViewParams& v, size_t pix, bool inside) {
        if (inside) {
            const size_t plane_stride = (size_t)v.width * (size_t)v.height;
            float* const out = a.out;
            out[pix] = acc[0];
            if constexpr (K == 4) {
                if (a.cols > 1u) out[plane_stride + pix] = acc[1];
                if (a.cols > 2u) out[2 * plane_stride + pix] = acc[2];
                if (a.cols > 3u) out[3 * plane_stride + pix] = acc[3];
            }
        }
    }
};

// ---- GradientSink: one channel group, K = 1 or 4, with its scale rule and its two small kernels --------------------------------------
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

struct GradientArgs {
    const float* planes;        // the group's first cotangent plane [H,W]
    long long* rows_q;          // [N,4] fixed-point sums, zeroed by the caller per group
    const uint32_t* max_bits;   // [4]: the float bits of the largest finite |g| of each of the group's planes (k_plane_max_abs)
    uint32_t cols;              // channels of this group, 1..4
};

template <int K>
struct GradientSink {
    static_assert(K == 1 || K == 4, "a group of one or of up to four channels");
    using Args = GradientArgs;
    using Slot = std::conditional_t<K == 1, float, float4>;
    // the waves' sums of w * g[k] of the chunk; hit (zeroed per chunk) says which slots are valid
    struct Shared {
        Slot gsum[kWaves][kBlock];
        uint8_t hit[kWaves][kBlock];
    };
    static constexpr bool kFlush = true;
    static constexpr bool kWantsHit = false;

    const Args& a;
    Shared& sh;
    float g[K] = {};         // the pixel's cotangent of the channel group, once
    float q_scale[K] = {};   // the planes' fixed-point scales 2^s_k (block-uniform)

    __device__ __forceinline__ GradientSink(const Args& args, Shared& shared, const ViewParams& v, size_t pix, bool inside) : a(args), sh(shared) {
        const size_t plane_stride = (size_t)v.width * (size_t)v.height;
        const uint32_t tiles = (uint32_t)(v.grid_x * v.grid_y);
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)K; ++k) {
            if (k < a.cols) {
                if (inside) g[k] = finite_or_zero(a.planes[k * plane_stride + pix]);
                q_scale[k] = pow2f(grad_scale_exponent(a.max_bits[k], tiles));
            }
        }
    }
    __device__ __forceinline__ void stage(uint32_t tid, uint32_t) {
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) sh.hit[w][tid] = 0u;
    }
    // per (wave, entry) some lane composited: every product rounded on its own (see ScoreSink), every channel through its own tree
    __device__ __forceinline__ void accept(const float w, const uint32_t j, const uint32_t wave, const uint32_t lane) {
        const unsigned long long hit = __ballot(w > 0.0f);
        if (hit == 0ull) return;
        float sums[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            float wg = w * g[k];
            asm volatile("" : "+v"(wg));
            sums[k] = dpp_wave_sum_lane63(wg);
        }
        if (lane == 63u) {
            if constexpr (K == 1) sh.gsum[wave][j] = sums[0];
            else sh.gsum[wave][j] = make_float4(sums[0], sums[1], sums[2], sums[3]);
            sh.hit[wave][j] = 1u;
        }
    }
    // thread j combines the waves' slots of entry j in wave order and adds them to the Gaussian's row of rows_q
    __device__ __forceinline__ void flush(const uint32_t j, const uint32_t* s_id) {
        bool any = false;
        float sum[K] = {};
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) {
            if (sh.hit[w][j] != 0u) {
                any = true;
                const Slot p = sh.gsum[w][j];
                if constexpr (K == 1) {
                    sum[0] += p;
                } else {
                    sum[0] += p.x; sum[1] += p.y; sum[2] += p.z; sum[3] += p.w;
                }
            }
        }
        if (any) {
            // |sum| < 2^-s 2^48 (grad_scale_exponent): the product is exact in fp32 (a power-of-two scale), the conversion rounds
            // to nearest, ties to even; the signed value is added in two's complement
            long long* const row = a.rows_q + 4 * (size_t)s_id[j];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const long long q = __float2ll_rn(sum[k] * q_scale[k]);
                if (q != 0ll) atomicAdd(reinterpret_cast<unsigned long long*>(row + k), (unsigned long long)q);
            }
        }
    }
    __device__ __forceinline__ void finish(const ViewParams&, size_t, bool) {}
};

// the largest finite |g| of each of a group's planes, as float bits (non-negative floats order as their bits): blockIdx.y is the plane
__global__ __launch_bounds__(kBlock) void k_plane_max_abs(const float* __restrict__ planes, size_t plane_stride, uint32_t* __restrict__ max_bits) {
    const float* const plane = planes + (size_t)blockIdx.y * plane_stride;
    float m = 0.0f;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < plane_stride; i += (size_t)gridDim.x * kBlock)
        m = fmaxf(m, fabsf(finite_or_zero(plane[i])));
    m = dpp_wave_max_lane63(m);
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

// ---- SurfaceSink: one composited entry per pixel, chosen by a level of the transmittance or by the largest weight ---------------------
struct SurfaceArgs {
    float* distance;   // [H,W]
    uint32_t* id;      // [H,W] or null
    float* weight;     // [H,W] or null
    float level;       // GUT_SURFACE_LEVEL: the transmittance below which the pixel's surface lies
};

template <int kMode>
struct SurfaceSink {
    static_assert(kMode == GUT_SURFACE_LEVEL || kMode == GUT_SURFACE_MAX_WEIGHT, "one of the two modes");
    using Args = SurfaceArgs;
    struct Shared {};   // (the state is the lane's own)
    static constexpr bool kFlush = false;
    static constexpr bool kWantsHit = true;

    const Args& a;
    // the pixel's choice so far, carried across the chunks; kInvalid: none yet (a list holds no such id)
    float dist = 0.0f, wgt = 0.0f;
    uint32_t gid = kInvalid;

    __device__ __forceinline__ SurfaceSink(const Args& args, Shared&, const ViewParams&, size_t, bool) : a(args) {}
    __device__ __forceinline__ void stage(uint32_t, uint32_t) {}
    __device__ __forceinline__ void accept(float, uint32_t, uint32_t, uint32_t) {}
    // level: the first entry, in list order, behind which |T| < level, and nothing after it.  Largest weight: a strictly greater
    // weight replaces the choice, so of equal weights the first in list order stays (every composited w is above 0)
    __device__ __forceinline__ void hit(const float w, const float hit_t, const float t_after, const uint32_t id) {
        const bool take = kMode == GUT_SURFACE_LEVEL ? (gid == kInvalid && t_after < a.level) : (w > wgt);
        if (take) {
            dist = hit_t;
            wgt = w;
            gid = id;
        }
    }
    __device__ __forceinline__ void flush(uint32_t, const uint32_t*) {}
    // every pixel of the image, the no-hit values where nothing was chosen: the planes need no initialisation
    __device__ __forceinline__ void finish(const ViewParams&, size_t pix, bool inside) {
        if (inside) {
            a.distance[pix] = dist;
            if (a.id) a.id[pix] = gid;
            if (a.weight) a.weight[pix] = wgt;
        }
    }
};

// ---- the walk --------------------------------------------------------------------------------------------------------------------
template <class Sink>
__global__ __launch_bounds__(kBlock, 4) void k_walk(const WalkOperands o, const typename Sink::Args args) {
    __shared__ TestEntry stage[kBlock];   // k_render's staged entry without its colour (gut_render_common.h); the id goes to s_id
    __shared__ uint32_t s_id[kBlock];
    __shared__ uint32_t s_first_invalid;
    __shared__ uint32_t s_mask[kBlock];              // see k_render
    __shared__ uint16_t s_list[kWaves][kBlock];      // see k_render
    __shared__ StripPlanes s_planes;
    __shared__ typename Sink::Shared s_sink;

    const ViewParams& v = o.v;
    const RenderConsts& c = o.c;
    const float4* const density12 = reinterpret_cast<const float4*>(o.density12);
    const uint32_t tile = o.tile_order[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const TilePixel at = tile_pixel(v, tile, tid);   // wave = 8x8 block
    const RayState ray = make_ray(v, o.ray_ori, o.ray_dir, at.pix, at.inside);
    Sink sink(args, s_sink, v, at.pix, at.inside);

    if (tid == 0) s_first_invalid = kBlock;
    const bool centred = __syncthreads_and(ray.centred ? 1 : 0) != 0;  // block-uniform
    build_strip_planes(s_planes, ray, at.inside, centred, tid);
    const uint32_t wave_bit = 1u << (tid >> 6);
    const uint32_t wave = tid >> 6, lane = tid & 63u;

    uint2 range = reinterpret_cast<const uint2*>(o.ranges)[tile];
    // no further than the forward walked (k_render_backward bounds its walk the same way): nothing behind that position was
    // composited, and with the lazy order only that prefix of the ordered-id list is ordered at all
    range.y = range.x + min(range.y - range.x, o.tile_walked[tile]);
    const uint32_t total = range.y - range.x;
    float T = ray.valid ? 1.0f : -1.0f;   // alive <=> T > 0; a ray that ends keeps -T (k_render)

    auto walk = [&](auto centred_tag) __attribute__((always_inline)) {
    constexpr bool kCentred = decltype(centred_tag)::value;
    for (uint32_t base = 0; base < total; base += kBlock) {
        if (!__syncthreads_or(T > 0.0f ? 1 : 0)) break;  // whole tile terminated
        {
            const uint32_t k = range.x + base + tid;
            uint32_t id = kInvalid;
            if (k < range.y) id = o.ordered_ids[k];
            if (id != kInvalid && id >= o.num_particles) id = kInvalid;   // (never in a list the forward built: keeps every access in bounds)
            // (make_entry's conversion once more, straight into the packed form and without the colour: through make_entry the compiler
            // orders this kernel's values differently and rounds other products of `entry` on their own in the walk of rays that do not
            // start at the sensor position — the contractions `entry` is pinned against, see there)
            TestEntry e;
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
            sink.stage(tid, id);
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
                    // o += M e, the same freedom and the same cure: in both instantiations of k_render (and of k_render_backward) the
                    // first copy rounds m00 ex, m11 ey, m20 ex and the second m01 ey, m11 ey, m21 ey, then adds the sum to oc; left
                    // to the compiler this unit rounded m01 ey, m10 ex, m21 ey in its first copy (ISA of all nine instantiations)
                    o0 += kSecond ? __builtin_fmaf(q1.z, ray.ez, __builtin_fmaf(q1.x, ray.ex, q1.y * ray.ey))
                                  : __builtin_fmaf(q1.z, ray.ez, __builtin_fmaf(q1.y, ray.ey, q1.x * ray.ex));
                    o1 += __builtin_fmaf(q2.y, ray.ez, __builtin_fmaf(q1.w, ray.ex, q2.x * ray.ey));
                    o2 += kSecond ? __builtin_fmaf(m22, ray.ez, __builtin_fmaf(q2.z, ray.ex, q2.w * ray.ey))
                                  : __builtin_fmaf(m22, ray.ez, __builtin_fmaf(q2.w, ray.ey, q2.z * ray.ex));
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
                            if constexpr (Sink::kWantsHit) sink.hit(w, hit_t, fabsf(T), s_id[j]);
                        }
                    }
                }
            }
            return wout;
        };
        // as in k_render: the wave compacts the chunk to the entries that can reach its 8x8 block, then walks that list with the
        // two-register-set software pipeline
        {
            uint16_t* list = s_list[wave];
            const uint32_t nw = compact_wave_list(list, s_mask, cnt, wave_bit, lane);
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
                sink.accept(entry(std::false_type{}, a0, a1, a2, a3, ja), ja, wave, lane);
                if (++i >= nw) break;
                if (__ballot(T > 0.0f) == 0ull) break;
                a0 = stage_at(stage, jc).q0; a1 = stage_at(stage, jc).q1; a2 = stage_at(stage, jc).q2; a3 = stage_at(stage, jc).q3.w;
                const uint32_t jd = min((uint32_t)list[min(i + 2, (uint32_t)kBlock - 1)], (uint32_t)kBlock - 1u);
                sink.accept(entry(std::true_type{}, b0, b1, b2, b3, jb), jb, wave, lane);
                ++i;
                ja = jc;
                jb = jd;
            }
        }
        if (cnt < cnt_all) T = -fabsf(T);  // list ended at a padding entry

        // (a sink without a flush: the barrier at the head of the loop stands between this chunk's reads and the next staging)
        if constexpr (Sink::kFlush) {
            __syncthreads();
            if (tid < cnt) sink.flush(tid, s_id);
        }
    }
    };
    if (centred) walk(std::true_type{}); else walk(std::false_type{});
    sink.finish(v, at.pix, at.inside);
}

template <class Sink>
void launch_walk(hipStream_t s, const WalkOperands& o, const typename Sink::Args& args) {
    hipLaunchKernelGGL(k_walk<Sink>, dim3(o.tiles), dim3(kBlock), 0, s, o, args);
}

}  // namespace

void launch_contribution(hipStream_t s, const WalkOperands& o, GutContribution* scores, const float* plane, uint64_t* weighted_q32) {
    if (o.tiles == 0) return;
    // no plane: the records alone; a plane: its weighted sums, with the records in the same walk where the caller wants them
    const auto launch = !plane ? launch_walk<ScoreSink<true, false>> : scores ? launch_walk<ScoreSink<true, true>> : launch_walk<ScoreSink<false, true>>;
    launch(s, o, {scores, plane, reinterpret_cast<unsigned long long*>(weighted_q32)});
}

void launch_attributes(hipStream_t s, const WalkOperands& o, uint32_t num_channels, const float* attrs, float* out) {
    if (o.tiles == 0) return;
    const size_t plane_stride = (size_t)o.v.width * (size_t)o.v.height;
    // one walk per group of four channels; a last group of one channel takes the single-channel kernel.  The 16-byte gather where
    // every row of the group starts on a 16-byte boundary, decided from the pointer here
    const bool aligned = (num_channels % 4u) == 0u && ((uintptr_t)attrs & 15u) == 0u;
    for (uint32_t first = 0; first < num_channels; first += 4u) {
        const uint32_t cols = num_channels - first < 4u ? num_channels - first : 4u;
        const auto launch = cols == 1u ? launch_walk<AttributeSink<1>> : launch_walk<AttributeSink<4>>;
        launch(s, o, {attrs + first, out + (size_t)first * plane_stride, num_channels, cols, aligned && cols == 4u ? 1u : 0u});
    }
}

void launch_surface(hipStream_t s, const WalkOperands& o, int mode, float level, float* distance, uint32_t* id, float* weight) {
    if (o.tiles == 0) return;
    const auto launch = mode == GUT_SURFACE_LEVEL ? launch_walk<SurfaceSink<GUT_SURFACE_LEVEL>> : launch_walk<SurfaceSink<GUT_SURFACE_MAX_WEIGHT>>;
    launch(s, o, {distance, id, weight, level});
}

void launch_attributes_bwd(hipStream_t s, const WalkOperands& o, uint32_t num_channels, const float* out_grad, float* attrs_grad,
                           void* rows_q, uint32_t* max_bits) {
    if (o.tiles == 0 || o.num_particles == 0) return;
    const size_t plane_stride = (size_t)o.v.width * (size_t)o.v.height;
    const uint32_t max_blocks = (uint32_t)std::min<size_t>((plane_stride + kBlock - 1) / kBlock, 256);
    const uint32_t row_blocks = (o.num_particles + kBlock - 1) / kBlock;
    // per group of four channels: the planes' maxima, the walk into the zeroed fixed-point rows, the rows into the caller's floats
    for (uint32_t first = 0; first < num_channels; first += 4u) {
        const uint32_t cols = num_channels - first < 4u ? num_channels - first : 4u;
        const float* const planes = out_grad + (size_t)first * plane_stride;
        (void)hipMemsetAsync(max_bits, 0, 4 * sizeof(uint32_t), s);
        (void)hipMemsetAsync(rows_q, 0, 4 * sizeof(long long) * (size_t)o.num_particles, s);
        hipLaunchKernelGGL(k_plane_max_abs, dim3(max_blocks, cols), dim3(kBlock), 0, s, planes, plane_stride, max_bits);
        const auto launch = cols == 1u ? launch_walk<GradientSink<1>> : launch_walk<GradientSink<4>>;
        launch(s, o, {planes, static_cast<long long*>(rows_q), max_bits, cols});
        hipLaunchKernelGGL(k_grad_rows, dim3(row_blocks), dim3(kBlock), 0, s, static_cast<const long long*>(rows_q), max_bits, o.tiles,
                           o.num_particles, cols, num_channels, attrs_grad + first);
    }
}

}  // namespace gut
