// gut_rows.h — what a per-Gaussian row is, once: the layouts, the activations and the backward's chain through them, for every
// kernel that reads or writes one (gut_project.hip: K1, K8, K8c, k_pack_fields; gut_train.hip: the activation and optimiser
// kernels, the record compaction; gut_pose.hip: the consuming pose reduction).  Inlined into each unit, so every kernel keeps the
// -ffp-contract of the unit it is built in (build.py UNITS): that flag is part of its numerics.
//
//   raw row  [N,12]: pos3 | density logit | quat4 (unnormalised) | log-scale3 | unused
//   act row  [N,12]: pos3 | sigmoid       | quat4 / |quat|       | exp3       | |quat|
//   gradient row, 64 bytes, accumulated by K7 w.r.t. the ACTIVATED parameters:
//                    d pos3 | d density   | d quat4              | d scale3   | dRGB3 | pad2
//
// The quaternion's clamped norm rides in the act row's pad column: chain_to_raw needs it for the normalisation and would
// otherwise re-read the raw row.  activate_scale puts it there and chain_to_raw reads it back as sc.w — that pairing lives here
// and nowhere else.  (The three float4 of an act row depend on one raw float4 each, plus that norm for the last.)
#pragma once
#include "gut_internal.h"

namespace gut {

// ---- raw row -> act row (threedgrut/model/model.py:74-93 with base_gs.yaml's sigmoid / normalize / exp) ----
__device__ __forceinline__ float4 activate_position_density(const float4& a) {
    return make_float4(a.x, a.y, a.z, 1.0f / (1.0f + expf(-a.w)));
}
__device__ __forceinline__ float4 activate_quaternion(const float4& q, float* clamped_norm) {
    const float nrm = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    const float inv = 1.0f / fmaxf(nrm, 1e-12f);  // torch.nn.functional.normalize eps
    *clamped_norm = fmaxf(nrm, 1e-12f);
    return make_float4(q.x * inv, q.y * inv, q.z * inv, q.w * inv);
}
__device__ __forceinline__ float4 activate_scale(const float4& s, float clamped_norm) {
    return make_float4(expf(s.x), expf(s.y), expf(s.z), clamped_norm);
}
__device__ __forceinline__ void activate_row(const float4& a, const float4& q, const float4& s, float4* __restrict__ act_row) {
    float nrm;
    act_row[0] = activate_position_density(a);
    act_row[1] = activate_quaternion(q, &nrm);
    act_row[2] = activate_scale(s, nrm);
}

// the three float4 of an [N,12] row, or of its gradient
// RULE: rows go into and come out of the functions below BY VALUE, never by reference.  A local row handed over by reference
// is promoted to registers later in the compiler's pipeline, the vectoriser then packs the chain's multiplies, and under
// -ffp-contract=fast a packed multiply no longer fuses with its add: the result bits of k_compact_gradient_rows change.
struct Row12 {
    float4 a, q, s;   // pos3 | density,  quat4,  scale3 | pad
};

// row i of the model's four tensors (positions [N,3], density [N,1], rotation [N,4], scale [N,3]) as an [N,12] row, pad column 0
// (tracer.py:176-178's torch.cat)
__device__ __forceinline__ Row12 load_field_row(const float* pos, const float* dns, const float4* rot, const float* scl, size_t i) {
    Row12 row;
    row.a = make_float4(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], dns[i]);
    row.q = rot[i];
    row.s = make_float4(scl[3 * i], scl[3 * i + 1], scl[3 * i + 2], 0.0f);
    return row;
}

// ---- the gradient row ----
struct GradientRow {   // as K7 left it
    float4 g0, g1, g2, g3;
};
struct ConsumedRow {   // d(pos3, density), d quat4, d scale3 | 0, and dL/dRGB masked by (precomputed RGB > 0)
    float4 g0, g1, g2;
    float r, g, b;
};
__device__ __forceinline__ GradientRow load_gradient_row(const float4* grad16, size_t i) {
    GradientRow row;
    row.g0 = grad16[4 * i + 0];
    row.g1 = grad16[4 * i + 1];
    row.g2 = grad16[4 * i + 2];
    row.g3 = grad16[4 * i + 3];
    return row;
}
// a row that was read is left zero for the next backward (no 64 N-byte clear per step)
__device__ __forceinline__ void clear_gradient_row(float4* grad16, size_t i) {
    grad16[4 * i + 0] = make_float4(0.f, 0.f, 0.f, 0.f);
    grad16[4 * i + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
    grad16[4 * i + 2] = make_float4(0.f, 0.f, 0.f, 0.f);
    grad16[4 * i + 3] = make_float4(0.f, 0.f, 0.f, 0.f);
}
// the colour slots (g2.w, g3.x, g3.y) masked by feat > 0 (the forward clamped the colour at zero), g2.w zeroed
__device__ __forceinline__ ConsumedRow mask_gradient_row(GradientRow row, const float* feat, size_t i) {
    ConsumedRow c;
    c.g0 = row.g0; c.g1 = row.g1; c.g2 = row.g2;
    c.r = feat[3 * i + 0] > 0.0f ? row.g2.w : 0.0f;
    c.g = feat[3 * i + 1] > 0.0f ? row.g3.x : 0.0f;
    c.b = feat[3 * i + 2] > 0.0f ? row.g3.y : 0.0f;
    c.g2.w = 0.0f;
    return c;
}
// load, clear, mask — what every epilogue does with its row (k_compact_gradient_rows takes the three steps apart: it loads
// before its ballot and masks and clears after it)
__device__ __forceinline__ ConsumedRow consume_gradient_row(float4* grad16, const float* feat, size_t i) {
    const GradientRow row = load_gradient_row(grad16, i);
    clear_gradient_row(grad16, i);
    return mask_gradient_row(row, feat, i);
}

// d(act row) -> d(raw row): sigmoid', normalise', exp' from the act row's own values (sigmoid = act[0].w, qn = act[1],
// sc = act[2] with |quat| in sc.w)
__device__ __forceinline__ Row12 chain_to_raw(float4 g0, float4 g1, float4 g2, float sigmoid, float4 qn, float4 sc) {
    g0.w = g0.w * sigmoid * (1.0f - sigmoid);
    const float dot = g1.x * qn.x + g1.y * qn.y + g1.z * qn.z + g1.w * qn.w;
    const float inv = 1.0f / sc.w;
    g1 = make_float4((g1.x - qn.x * dot) * inv, (g1.y - qn.y * dot) * inv, (g1.z - qn.z * dot) * inv, (g1.w - qn.w * dot) * inv);
    g2.x *= sc.x; g2.y *= sc.y; g2.z *= sc.z;
    Row12 raw;
    raw.a = g0; raw.q = g1; raw.s = g2;
    return raw;
}

// real SH basis up to degree 3 (gaussianParticles.cuh:57-96)
__device__ __forceinline__ void sh_basis(int deg, float x, float y, float z, float Y[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) Y[i] = 0.0f;
    Y[0] = 0.28209479177387814f;
    if (deg > 0) {
        Y[1] = -0.4886025119029199f * y;
        Y[2] = 0.4886025119029199f * z;
        Y[3] = -0.4886025119029199f * x;
        if (deg > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            Y[4] = 1.0925484305920792f * xy;
            Y[5] = -1.0925484305920792f * yz;
            Y[6] = 0.31539156525252005f * (2.0f * zz - xx - yy);
            Y[7] = -1.0925484305920792f * xz;
            Y[8] = 0.5462742152960396f * (xx - yy);
            if (deg > 2) {
                Y[9] = -0.5900435899266435f * y * (3.0f * xx - yy);
                Y[10] = 2.890611442640554f * xy * z;
                Y[11] = -0.4570457994644658f * y * (4.0f * zz - xx - yy);
                Y[12] = 0.3731763325901154f * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
                Y[13] = -0.4570457994644658f * x * (4.0f * zz - xx - yy);
                Y[14] = 1.445305721320277f * z * (xx - yy);
                Y[15] = -0.5900435899266435f * x * (xx - 3.0f * yy);
            }
        }
    }
}

}  // namespace gut
