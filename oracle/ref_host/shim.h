/*
 * shim.h — the few CUDA built-ins the reference's per-hit header needs, for a HOST build.
 *
 * TEST INFRASTRUCTURE ONLY (oracle/Makefile: _ref).  ref_hits.cpp includes this file and then the reference's own
 * kernels/cuda/models/gaussianParticles.cuh (with common/mathUtils.cuh under it) BY PATH from the reference tree; no line
 * of either is restated here.  That header uses CUDA's built-in vector types and a handful of intrinsics only; everything
 * supplied below is componentwise or IEEE-defined, so what runs is the reference's own statement order.
 *
 * Where CUDA leaves a function approximate, the shim takes the correctly rounded / libm form, and variant 0 of
 * oracle/gut_oracle.c is held to the same choices:
 *   - rsqrtf(x) = 1.0f / sqrtf(x)   (CUDA: 2 ulp; under the reference's -use_fast_math an approximate instruction);
 *   - expf, powf, logf, sqrtf and '/' are libm's / IEEE's (CUDA: 1 - 2 ulp, approximate under -use_fast_math);
 *   - no contraction: the library is built with -ffp-contract=off (nvcc fuses multiply-adds at will).
 * The componentwise float3 operators and make_float3(float) are the ones mathUtils.cuh comments out because Slang's
 * prelude provides them in the reference's build.
 */
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
#define __CUDACC__ 1                       /* mathUtils.cuh is empty without it */
#define PARTICLE_RADIANCE_NUM_COEFFS 16    /* the build's -DPARTICLE_RADIANCE_NUM_COEFFS (16 coefficients: SH degree 3) */

struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct int3 { int x, y, z; };

static inline float2 make_float2(float x, float y) { return float2{x, y}; }
static inline float3 make_float3(float x, float y, float z) { return float3{x, y, z}; }
static inline float3 make_float3(float a) { return float3{a, a, a}; }
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
static inline int3 make_int3(int x, int y, int z) { return int3{x, y, z}; }

static inline float3 operator+(const float3& a, const float3& b) { return float3{a.x + b.x, a.y + b.y, a.z + b.z}; }
static inline float3 operator-(const float3& a, const float3& b) { return float3{a.x - b.x, a.y - b.y, a.z - b.z}; }
static inline float3 operator*(const float3& a, const float3& b) { return float3{a.x * b.x, a.y * b.y, a.z * b.z}; }
static inline float3 operator/(const float3& a, const float3& b) { return float3{a.x / b.x, a.y / b.y, a.z / b.z}; }
static inline float3 operator-(const float3& a) { return float3{-a.x, -a.y, -a.z}; }

static inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }
static inline float __saturatef(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
static inline int __float_as_int(float f) { int i; memcpy(&i, &f, 4); return i; }
static inline unsigned int __float_as_uint(float f) { unsigned int u; memcpy(&u, &f, 4); return u; }
static inline float __int_as_float(int i) { float f; memcpy(&f, &i, 4); return f; }
static inline float __uint_as_float(unsigned int u) { float f; memcpy(&f, &u, 4); return f; }

/* one host thread: the atomics are plain read-modify-writes that return the old value */
static inline float atomicAdd(float* p, float v) { const float o = *p; *p = o + v; return o; }
static inline int atomicMin(int* p, int v) { const int o = *p; if (v < o) *p = v; return o; }
static inline int atomicMax(int* p, int v) { const int o = *p; if (v > o) *p = v; return o; }
static inline unsigned int atomicMin(unsigned int* p, unsigned int v) { const unsigned int o = *p; if (v < o) *p = v; return o; }
static inline unsigned int atomicMax(unsigned int* p, unsigned int v) { const unsigned int o = *p; if (v > o) *p = v; return o; }
