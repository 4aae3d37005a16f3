// gut_fuse.hip — the scene as a mesh, for gfx950:
//   k_tsdf_integrate   fuses up to GUT_TSDF_MAX_VIEWS distance planes into the caller's integer TSDF volume, one thread per voxel
//   k_nets_cells       surface nets: which cells are fully observed, which hold a sign change
//   k_nets_quads       surface nets: how many quads each lattice point emits
//   k_nets_emit        surface nets: the vertices and the triangles, behind the caller's exclusive scans
//
// THIS FILE IS COMPILED WITH -ffp-contract=off, as gut_project.hip is: a voxel's pixel and its side of the truncation are integer
// decisions of fp32 arithmetic, evaluated in one documented order with IEEE-exact +,-,*,/,sqrt.  The projection IS K1's: both
// units include gut_camera.h, whose functions are generic over the view record ("the projection").
#include "gut_camera.h"

namespace gut {

namespace {

__device__ __forceinline__ float voxel_centre(float origin, float voxel, int i) { return origin + voxel * ((float)i + 0.5f); }

// One view's update of one voxel, accumulated into the thread's registers.  Steps 1 to 6 of DESIGN.md §19.
template <bool kColour>
__device__ __forceinline__ void integrate_view(const FuseView& v, float truncation, float wx, float wy, float wz, int32_t& acc,
                                               uint32_t& cnt, uint32_t (&rgb)[3], uint32_t& rgb_cnt) {
    float cx, cy, cz, u, w;
    affine_point(v.w2s, wx, wy, wz, cx, cy, cz);
    int valid;
    if (v.variant == 0) valid = project_camera<0>(v, cx, cy, cz, 0.0f, u, w);
    else if (v.variant == 1) valid = project_camera<1>(v, cx, cy, cz, 0.0f, u, w);
    else valid = project_camera<2>(v, cx, cy, cz, 0.0f, u, w);
    if (!valid) return;
    const int px = (int)floorf(u), py = (int)floorf(w);
    if (px < 0 || py < 0 || px >= v.width || py >= v.height) return;   // (valid already says 0 < u < W, 0 < v < H)
    const size_t pixel = (size_t)py * (size_t)v.width + (size_t)px;
    const float D = v.distance[pixel];
    if (D == 0.0f || !(fabsf(D) <= 3.4028234664e+38f)) return;   // no surface; inf or NaN
    float ox = 0.0f, oy = 0.0f, oz = 0.0f;
    if (v.origin) {
        ox = v.origin[3 * pixel + 0];
        oy = v.origin[3 * pixel + 1];
        oz = v.origin[3 * pixel + 2];
    }
    const float dx = cx - ox, dy = cy - oy, dz = cz - oz;
    const float range = sqrtf(dx * dx + dy * dy + dz * dz);
    const float s = D - range;
    if (!(s >= -truncation)) return;   // hidden behind the surface (or NaN from a non-finite origin)
    const float q = s / truncation;
    const float f = q < 1.0f ? q : 1.0f;
    acc += (int32_t)rintf(f * 65536.0f);
    cnt += 1u;
    if (kColour) {
        if (v.rgba && fabsf(s) <= truncation) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float x = v.rgba[4 * pixel + c];
                x = x > 0.0f ? x : 0.0f;   // NaN -> 0
                x = x < 1.0f ? x : 1.0f;
                rgb[c] += (uint32_t)rintf(255.0f * x);
            }
            rgb_cnt += 1u;
        }
    }
}

// One thread per voxel, x along the lanes.  The views' sums are formed in registers from zero; a voxel some view updated is then
// read, added to and stored, once; a voxel no view updated is neither read nor written.
template <bool kColour>
__global__ __launch_bounds__(kBlock) void k_tsdf_integrate(FuseGrid g, int n_views, FuseViews views) {
    const uint32_t total = (uint32_t)g.X * (uint32_t)g.Y * (uint32_t)g.Z;   // <= 2^30
    const uint32_t idx = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (idx >= total) return;
    const uint32_t row = idx / (uint32_t)g.X;
    const int i = (int)(idx - row * (uint32_t)g.X), j = (int)(row % (uint32_t)g.Y), k = (int)(row / (uint32_t)g.Y);
    const float wx = voxel_centre(g.origin[0], g.voxel, i), wy = voxel_centre(g.origin[1], g.voxel, j), wz = voxel_centre(g.origin[2], g.voxel, k);
    int32_t acc = 0;
    uint32_t cnt = 0, rgb[3] = {0, 0, 0}, rgb_cnt = 0;
    for (int n = 0; n < n_views; ++n) integrate_view<kColour>(views.v[n], g.truncation, wx, wy, wz, acc, cnt, rgb, rgb_cnt);
    if (cnt == 0) return;
    g.acc[idx] += acc;
    g.cnt[idx] += cnt;
    if (kColour) {
        if (rgb_cnt) {
            uint32_t* sum = g.rgb_sum + 3 * (size_t)idx;
            sum[0] += rgb[0];
            sum[1] += rgb[1];
            sum[2] += rgb[2];
            g.rgb_cnt[idx] += rgb_cnt;
        }
    }
}

// ---- surface nets ----
struct Lattice {
    int i, j, k;
    bool in_grid;
};
__device__ __forceinline__ Lattice lattice_point(const FuseGrid& g) {
    const uint32_t total = (uint32_t)g.X * (uint32_t)g.Y * (uint32_t)g.Z;
    const uint32_t idx = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    const uint32_t row = idx / (uint32_t)g.X;
    return {(int)(idx - row * (uint32_t)g.X), (int)(row % (uint32_t)g.Y), (int)(row / (uint32_t)g.Y), idx < total};
}

// bit 0: the cell exists and its eight corners are observed; bit 1: and they are not all on one side
__global__ __launch_bounds__(kBlock) void k_nets_cells(FuseGrid g, uint32_t min_count, uint8_t* __restrict__ cell) {
    const Lattice p = lattice_point(g);
    if (!p.in_grid) return;
    const uint32_t idx = ((uint32_t)p.k * (uint32_t)g.Y + (uint32_t)p.j) * (uint32_t)g.X + (uint32_t)p.i;
    uint32_t code = 0;
    if (p.i < g.X - 1 && p.j < g.Y - 1 && p.k < g.Z - 1) {
        bool observed = true;
        int inside = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint32_t at = idx + (uint32_t)(c & 1) + (uint32_t)((c >> 1) & 1) * (uint32_t)g.X + (uint32_t)(c >> 2) * (uint32_t)g.X * (uint32_t)g.Y;
            observed = observed && g.cnt[at] >= min_count;
            inside += g.acc[at] < 0 ? 1 : 0;
        }
        code = observed ? ((inside != 0 && inside != 8) ? 3u : 1u) : 0u;
    }
    cell[idx] = (uint8_t)code;
}

// Does the lattice edge p -> p + e_axis emit a quad?  cells[4]: the linear indices of its four cells in winding order for an inside p.
__device__ __forceinline__ bool quad_at(const FuseGrid& g, const uint8_t* __restrict__ cell, const Lattice& p, uint32_t idx, int axis,
                                        uint32_t (&cells)[4], bool& p_inside) {
    const uint32_t sx = 1u, sy = (uint32_t)g.X, sz = (uint32_t)g.X * (uint32_t)g.Y;
    const uint32_t sa = axis == 0 ? sx : (axis == 1 ? sy : sz);
    const uint32_t sb = axis == 0 ? sy : (axis == 1 ? sz : sx);   // (a, b, c) cyclic
    const uint32_t sc = axis == 0 ? sz : (axis == 1 ? sx : sy);
    const int pb = axis == 0 ? p.j : (axis == 1 ? p.k : p.i);
    const int pc = axis == 0 ? p.k : (axis == 1 ? p.i : p.j);
    if (pb < 1 || pc < 1) return false;
    cells[0] = idx - sb - sc;
    cells[1] = idx - sc;
    cells[2] = idx;
    cells[3] = idx - sb;
    // a cell that does not exist (p on the far face) holds 0; a fully observed cell p has p and p + e_axis among its corners
    if (!((cell[cells[0]] & cell[cells[1]] & cell[cells[2]] & cell[cells[3]]) & 1u)) return false;
    p_inside = g.acc[idx] < 0;
    return p_inside != (g.acc[idx + sa] < 0);
}

__global__ __launch_bounds__(kBlock) void k_nets_quads(FuseGrid g, const uint8_t* __restrict__ cell, uint8_t* __restrict__ quads) {
    const Lattice p = lattice_point(g);
    if (!p.in_grid) return;
    const uint32_t idx = ((uint32_t)p.k * (uint32_t)g.Y + (uint32_t)p.j) * (uint32_t)g.X + (uint32_t)p.i;
    uint32_t n = 0, cells[4];
    bool inside;
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) n += quad_at(g, cell, p, idx, axis, cells, inside) ? 1u : 0u;
    quads[idx] = (uint8_t)n;
}

__global__ __launch_bounds__(kBlock) void k_nets_emit(FuseGrid g, const uint8_t* __restrict__ cell, const uint8_t* __restrict__ quads,
                                                      const int32_t* __restrict__ vertex_offset, const int32_t* __restrict__ quad_offset,
                                                      float* __restrict__ vertices, float* __restrict__ colours, int32_t* __restrict__ faces) {
    const Lattice p = lattice_point(g);
    if (!p.in_grid) return;
    const uint32_t idx = ((uint32_t)p.k * (uint32_t)g.Y + (uint32_t)p.j) * (uint32_t)g.X + (uint32_t)p.i;
    if (cell[idx] & 2u) {
        float f[8];
        float rgb[3] = {0.0f, 0.0f, 0.0f};
        int coloured = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint32_t at = idx + (uint32_t)(c & 1) + (uint32_t)((c >> 1) & 1) * (uint32_t)g.X + (uint32_t)(c >> 2) * (uint32_t)g.X * (uint32_t)g.Y;
            f[c] = (float)g.acc[at] / ((float)g.cnt[at] * 65536.0f);
            // the side is the integer's: acc < 0.  (float)acc keeps the sign, and a zero acc gives +0
            if (g.rgb_sum) {
                const uint32_t n = g.rgb_cnt[at];
                if (n) {
                    const float d = 255.0f * (float)n;
                    rgb[0] += (float)g.rgb_sum[3 * (size_t)at + 0] / d;
                    rgb[1] += (float)g.rgb_sum[3 * (size_t)at + 1] / d;
                    rgb[2] += (float)g.rgb_sum[3 * (size_t)at + 2] / d;
                    ++coloured;
                }
            }
        }
        float sum[3] = {0.0f, 0.0f, 0.0f};
        int crossings = 0;
        // the twelve edges in the header's order: axis x, y, z, and per axis the four edges by their lower corner
#pragma unroll
        for (int axis = 0; axis < 3; ++axis) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int lo_bits = axis == 0 ? (e << 1) : (axis == 1 ? ((e & 1) | ((e >> 1) << 2)) : e);
                const int c0 = lo_bits, c1 = lo_bits | (1 << axis);
                const float f0 = f[c0], f1 = f[c1];
                if ((f0 < 0.0f) != (f1 < 0.0f)) {
                    const float t = f0 / (f0 - f1);
                    float at[3] = {(float)(c0 & 1), (float)((c0 >> 1) & 1), (float)(c0 >> 2)};
                    at[axis] = t;
                    sum[0] += at[0];
                    sum[1] += at[1];
                    sum[2] += at[2];
                    ++crossings;
                }
            }
        }
        const float n = (float)crossings;
        const size_t out = 3 * (size_t)vertex_offset[idx];
        vertices[out + 0] = g.origin[0] + g.voxel * (((float)p.i + 0.5f) + sum[0] / n);
        vertices[out + 1] = g.origin[1] + g.voxel * (((float)p.j + 0.5f) + sum[1] / n);
        vertices[out + 2] = g.origin[2] + g.voxel * (((float)p.k + 0.5f) + sum[2] / n);
        const float m = (float)coloured;
        colours[out + 0] = coloured ? rgb[0] / m : 0.5f;
        colours[out + 1] = coloured ? rgb[1] / m : 0.5f;
        colours[out + 2] = coloured ? rgb[2] / m : 0.5f;
    }
    if (quads[idx]) {
        size_t out = 6 * (size_t)quad_offset[idx];
        uint32_t cells[4];
        bool inside;
#pragma unroll
        for (int axis = 0; axis < 3; ++axis) {
            if (!quad_at(g, cell, p, idx, axis, cells, inside)) continue;
            const int32_t v0 = vertex_offset[cells[0]], v1 = vertex_offset[cells[inside ? 1 : 3]], v2 = vertex_offset[cells[2]],
                          v3 = vertex_offset[cells[inside ? 3 : 1]];
            faces[out + 0] = v0; faces[out + 1] = v1; faces[out + 2] = v2;
            faces[out + 3] = v0; faces[out + 4] = v2; faces[out + 5] = v3;
            out += 6;
        }
    }
}

inline dim3 voxel_grid(const FuseGrid& g) {
    const uint32_t total = (uint32_t)g.X * (uint32_t)g.Y * (uint32_t)g.Z;
    return dim3((total + (uint32_t)kBlock - 1) / (uint32_t)kBlock);
}

}  // namespace

void launch_tsdf_integrate(hipStream_t s, const FuseGrid& g, int n_views, const FuseViews& views) {
    if (g.rgb_sum)
        hipLaunchKernelGGL(k_tsdf_integrate<true>, voxel_grid(g), dim3(kBlock), 0, s, g, n_views, views);
    else
        hipLaunchKernelGGL(k_tsdf_integrate<false>, voxel_grid(g), dim3(kBlock), 0, s, g, n_views, views);
}

void launch_surface_nets_count(hipStream_t s, const FuseGrid& g, uint32_t min_count, uint8_t* cell, uint8_t* quads) {
    hipLaunchKernelGGL(k_nets_cells, voxel_grid(g), dim3(kBlock), 0, s, g, min_count, cell);
    hipLaunchKernelGGL(k_nets_quads, voxel_grid(g), dim3(kBlock), 0, s, g, cell, quads);
}

void launch_surface_nets_emit(hipStream_t s, const FuseGrid& g, uint32_t min_count, const uint8_t* cell, const uint8_t* quads,
                              const int32_t* vertex_offset, const int32_t* quad_offset, float* vertices, float* colours, int32_t* faces) {
    (void)min_count;   // the observed / active bits of `cell` already carry it
    hipLaunchKernelGGL(k_nets_emit, voxel_grid(g), dim3(kBlock), 0, s, g, cell, quads, vertex_offset, quad_offset, vertices, colours, faces);
}

}  // namespace gut
