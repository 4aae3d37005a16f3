/*
 * ref_hits.cpp — a C ABI over the reference's OWN per-hit functions, compiled for the host.
 *
 * TEST INFRASTRUCTURE ONLY.  Built by `make -C oracle _ref` into oracle/_ref/libgut_refhits.so when the reference tree is
 * at hand; tests/golden/gen_hit_golden.py records what it returns into tests/golden/hit_golden.npz, and the tests read that
 * file.  Nothing here restates the reference: the functions called below are defined in the header included by path.
 *
 * Units: particleResponse<n> / particleResponseGrd<n>, processHitBwd<n, false, false> (the instantiation the unsorted
 * backward calls per hit: volumetric particle, per-Gaussian precomputed radiance), radianceFromSpH, the five-argument
 * radianceFromSpHBwd<false> and quaternionWXYZToMatrix.  n is one of 0, 1, 2, 3, 4, 5, 8; any other value takes the
 * quadratic default, as the reference's own switch does.
 */
#include "shim.h"

#include <3dgut/kernels/cuda/models/gaussianParticles.cuh>

#define REF_DISPATCH(DEGREE, CALL)                \
    switch (DEGREE) {                             \
    case 0: { constexpr int N = 0; CALL; break; } \
    case 1: { constexpr int N = 1; CALL; break; } \
    case 3: { constexpr int N = 3; CALL; break; } \
    case 4: { constexpr int N = 4; CALL; break; } \
    case 5: { constexpr int N = 5; CALL; break; } \
    case 8: { constexpr int N = 8; CALL; break; } \
    default: { constexpr int N = 2; CALL; break; } \
    }

static float3 f3(const float* p) { return make_float3(p[0], p[1], p[2]); }

extern "C" {

float ref_particle_response(int degree, float d2) {
    float r = 0.0f;
    REF_DISPATCH(degree, r = threedgut::particleResponse<N>(d2));
    return r;
}

float ref_particle_response_grd(int degree, float d2, float resp, float resp_grad) {
    float r = 0.0f;
    REF_DISPATCH(degree, r = threedgut::particleResponseGrd<N>(d2, resp, resp_grad));
    return r;
}

/* One per-hit backward step.  particle12: position(3), density, quaternion wxyz(4), scale(3), padding — the layout of the
 * reference's ParticleDensity.  feat3: the particle's (already clamped) radiance.  state_io: running transmittance,
 * radiance(3), depth — updated as the reference updates its reference arguments.  finals: integrated transmittance,
 * radiance(3), depth.  cot: transmittance gradient, radiance gradient(3), depth gradient.  thresholds: min response,
 * min alpha, min transmittance.  Out: the 11-float density gradient and the 3-float feature gradient (zero when the hit is
 * rejected).  Returns 1 when the reference accepted the hit: it then writes the feature gradient, which is pre-set to NaN. */
int ref_process_hit_bwd(int degree, const float* ray_ori, const float* ray_dir, const float* particle12, const float* feat3,
                        const float* thresholds, const float* finals, const float* cot, float* state_io,
                        float* density_grad11, float* feat_grad3) {
    threedgut::ParticleDensity pd, gd;
    memcpy(&pd, particle12, sizeof(pd));
    memset(&gd, 0, sizeof(gd));
    float fg[3] = {NAN, NAN, NAN};
    float T = state_io[0];
    float3 rad = f3(state_io + 1);
    float depth = state_io[4];
    REF_DISPATCH(degree, (threedgut::processHitBwd<N, false, false>(
                             f3(ray_ori), f3(ray_dir), 0u, pd, &gd, feat3, fg, thresholds[0], thresholds[1], thresholds[2], 0,
                             finals[0], T, cot[0], f3(finals + 1), rad, f3(cot + 1), finals[4], depth, cot[4])));
    const int accepted = !std::isnan(fg[0]);
    state_io[0] = T; state_io[1] = rad.x; state_io[2] = rad.y; state_io[3] = rad.z; state_io[4] = depth;
    memcpy(density_grad11, &gd, 11 * sizeof(float));
    for (int c = 0; c < 3; ++c) feat_grad3[c] = accepted ? fg[c] : 0.0f;
    return accepted;
}

void ref_radiance_from_sph(int deg, const float* sph48, const float* dir3, int clamped, float* out3) {
    const float3 r = threedgut::radianceFromSpH(deg, reinterpret_cast<const float3*>(sph48), f3(dir3), clamped != 0);
    out3[0] = r.x; out3[1] = r.y; out3[2] = r.z;
}

/* sph_grad48 is zeroed here, then receives the reference's (non-atomic) adds */
void ref_radiance_from_sph_bwd(int deg, const float* dir3, const float* rad_grad3, const float* radiance_unclamped3, float* sph_grad48) {
    float3 g[16];
    memset(g, 0, sizeof(g));
    threedgut::radianceFromSpHBwd<false>(deg, f3(dir3), f3(rad_grad3), g, f3(radiance_unclamped3));
    memcpy(sph_grad48, g, sizeof(g));
}

void ref_quaternion_to_matrix(const float* q_wxyz, float* rows9) {
    float33 m;
    threedgut::quaternionWXYZToMatrix(make_float4(q_wxyz[0], q_wxyz[1], q_wxyz[2], q_wxyz[3]), m);
    memcpy(rows9, m, sizeof(m));
}

} /* extern "C" */
