// gut_render_diag.h — the diagnostics of the unsorted compositors (gut_render.hip), kept out of the product kernels.  DIAGNOSTIC BUILDS
// ONLY: the product library defines none of the switches below and every macro of this header expands to nothing; the kernels name
// them at the places the diagnostics observe and carry no conditional of their own.  The general unit (gut_render_general.hip) never
// has diagnostics.
//   -DGUT_CLOCK_STAMPS        (tools/clock_probe.py builds tools/bin/libgut_hip_stamps.so with it) clock stamps of K7's workgroups and
//                             the cycles K6 / K7 spend in the phases of their chunk loops, in three device arrays nothing else reads,
//                             copied to the host by the gut_debug_* exports below
//   -DGUT_K6_EXTRA_LDS=bytes  LDS ballast in k_render: lowers the number of resident workgroups per CU (what a second staging area
//   -DGUT_K7_EXTRA_LDS=bytes  would cost) / the same in k_render_backward (occupancy experiment)
#pragma once
#include "gut_internal.h"

#if defined(GUT_CLOCK_STAMPS) && !defined(GUT_RENDER_GENERAL_TU)
namespace gut {

// Every workgroup of the backward compositor stamps the shader clock (s_memtime, cycles) and the constant 100 MHz counter
// (s_memrealtime) at its start and end — delta cycles / delta real time is the clock the chip actually held during the launch
// (MI355X_MICROARCH.md, "DVFS give-back" item 6) ...
__device__ unsigned long long g_clock_stamps[8192][4];
// ... and thread 0 of every workgroup adds up the cycles it spent in the phases of its chunk loop.  Forward: [0] whole workgroup,
// [1] lazy selection, [2] staging (id + parameter gather, conversion, up to the barrier), [3] walking the chunk (incl. the wait for
// the slowest wave at the next loop head).  Backward: [0] staging, [1] walk, [2] epilogue + flush, [3] whole workgroup.
__device__ unsigned long long g_k6_phases[8192][4];
__device__ unsigned long long g_k7_phases[8192][4];

struct K6Stamps {
    unsigned long long acc[4] = {0, 0, 0, 0}, prev = 0, begin, tA = 0, tB = 0;
    __device__ K6Stamps() : begin(__builtin_amdgcn_s_memtime()) {}
    __device__ void add(int slot, unsigned long long a, unsigned long long b) { if (threadIdx.x == 0) acc[slot] += b - a; }
    __device__ void chunk_begin() {   // behind the barrier at the loop head
        tA = __builtin_amdgcn_s_memtime();
        if (prev) add(3, prev, tA);    // walking the previous chunk + the wait for its slowest wave
        tB = tA;
    }
    __device__ void selected() { tB = __builtin_amdgcn_s_memtime(); add(1, tA, tB); }
    __device__ void staged() {   // (a barrier of the stamped build only: staging ends when the slowest thread has stored)
        __syncthreads();
        prev = __builtin_amdgcn_s_memtime();
        add(2, tB, prev);
    }
    __device__ void finish() {
        if (threadIdx.x == 0 && blockIdx.x < 8192) {
            const unsigned long long end = __builtin_amdgcn_s_memtime();
            if (prev) acc[3] += end - prev;
            g_k6_phases[blockIdx.x][0] = end - begin;
            g_k6_phases[blockIdx.x][1] = acc[1]; g_k6_phases[blockIdx.x][2] = acc[2]; g_k6_phases[blockIdx.x][3] = acc[3];
        }
    }
};

struct K7Stamps {
    unsigned long long acc[3] = {0, 0, 0}, tA = 0, tB = 0, tC = 0;
    __device__ K7Stamps() {
        if (threadIdx.x == 0 && blockIdx.x < 8192) {
            g_clock_stamps[blockIdx.x][0] = __builtin_amdgcn_s_memtime();
            g_clock_stamps[blockIdx.x][1] = __builtin_amdgcn_s_memrealtime();
        }
    }
    __device__ void chunk_begin() { tA = __builtin_amdgcn_s_memtime(); }
    __device__ void staged() { tB = __builtin_amdgcn_s_memtime(); }
    __device__ void walked() { tC = __builtin_amdgcn_s_memtime(); }
    __device__ void chunk_end() {   // [0] staging, [1] walking + wait for the slowest wave, [2] epilogue + flush
        if (threadIdx.x == 0) {
            const unsigned long long tD = __builtin_amdgcn_s_memtime();
            acc[0] += tB - tA; acc[1] += tC - tB; acc[2] += tD - tC;
        }
    }
    __device__ void finish() {
        if (threadIdx.x == 0 && blockIdx.x < 8192) {
            g_clock_stamps[blockIdx.x][2] = __builtin_amdgcn_s_memtime();
            g_clock_stamps[blockIdx.x][3] = __builtin_amdgcn_s_memrealtime();
            g_k7_phases[blockIdx.x][0] = acc[0]; g_k7_phases[blockIdx.x][1] = acc[1]; g_k7_phases[blockIdx.x][2] = acc[2];
            g_k7_phases[blockIdx.x][3] = g_clock_stamps[blockIdx.x][2] - g_clock_stamps[blockIdx.x][0];
        }
    }
};

}  // namespace gut

// each copies one of the arrays above, [8192][4] u64, to the host
extern "C" int gut_debug_clock_stamps(void* host_dst) {
    return hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(gut::g_clock_stamps), sizeof(gut::g_clock_stamps)) == hipSuccess ? 0 : 1;
}
extern "C" int gut_debug_k7_phases(void* host_dst) {
    return hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(gut::g_k7_phases), sizeof(gut::g_k7_phases)) == hipSuccess ? 0 : 1;
}
extern "C" int gut_debug_k6_phases(void* host_dst) {
    return hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(gut::g_k6_phases), sizeof(gut::g_k6_phases)) == hipSuccess ? 0 : 1;
}

#define GUT_STAMPS(Type, name) Type name     // the kernel's stamp state
#define GUT_STAMP(call) call                 // one observation: a method of it
#else
#define GUT_STAMPS(Type, name) do { } while (0)
#define GUT_STAMP(call) do { } while (0)
#endif

// `bytes` of LDS the kernel holds and never uses (the two accesses cannot happen: widths are positive; they keep the array alive)
#define GUT_LDS_BALLAST(bytes, v, sink)                                   \
    __shared__ float s_ballast[(bytes) / 4];                              \
    if (threadIdx.x == 0 && (v).width < 0) s_ballast[0] = 1.0f;           \
    if ((v).width < -1) (sink)[0] = s_ballast[threadIdx.x]
#if defined(GUT_K6_EXTRA_LDS) && !defined(GUT_RENDER_GENERAL_TU)
#define GUT_K6_BALLAST(v, sink) GUT_LDS_BALLAST(GUT_K6_EXTRA_LDS, v, sink)
#else
#define GUT_K6_BALLAST(v, sink) do { } while (0)
#endif
#if defined(GUT_K7_EXTRA_LDS) && !defined(GUT_RENDER_GENERAL_TU)
#define GUT_K7_BALLAST(v, sink) GUT_LDS_BALLAST(GUT_K7_EXTRA_LDS, v, sink)
#else
#define GUT_K7_BALLAST(v, sink) do { } while (0)
#endif
