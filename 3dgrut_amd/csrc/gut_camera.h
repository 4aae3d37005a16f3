// gut_camera.h — the camera projection, once: sensor-space point -> pixel, for K1 (gut_project.hip) and the TSDF fusion
// (gut_fuse.hip).  These functions are the numerics contract of DESIGN.md §4: fp32 in the order written here, IEEE-exact
// +,-,*,/,sqrt, det_atan2f_pos instead of the device math library.  EVERY UNIT THAT INCLUDES THIS HEADER MUST BE BUILT WITH
// -ffp-contract=off: an FMA in any of these expressions moves a pixel, and with it an integer buffer.
//
// A `View` is any record with these fields (ViewParams and FuseView are the two; the field names are the contract):
//     int32_t width, height;
//     float principal_point[2], focal_length[2];
//     float radial[6], tangential[2], thin_prism[4];
//     float max_angle;
#pragma once
#include "gut_internal.h"

namespace gut {

// atan2(y, x), y > 0: Cephes atanf reduction + polynomial
__device__ inline float det_atan2f_pos(float y, float x) {
    const float ax = fabsf(x);
    const float lo = y < ax ? y : ax;
    const float hi = y < ax ? ax : y;
    float t = lo / hi;
    float base = 0.0f;
    if (t > 0.4142135679721832f) {
        base = 0.7853981852531433f;
        t = (t - 1.0f) / (t + 1.0f);
    }
    const float z = t * t;
    float a = (((8.05374449538e-2f * z - 1.38776856032e-1f) * z + 1.99777106478e-1f) * z - 3.33329491539e-1f) * z * t + t;
    a = base + a;
    if (y > ax) a = 1.5707963705062866f - a;
    if (x < 0.0f) a = 3.1415927410125732f - a;
    return a;
}

__device__ __forceinline__ bool within_resolution(float rx, float ry, float tol, float px, float py) {
    const float mx = rx * tol, my = ry * tol;
    return (px > -mx) && (py > -my) && (px < rx + mx) && (py < ry + my);
}

// OpenCV pinhole with rational radial / tangential / thin-prism distortion (cameraProjections.cuh:57-103)
template <bool kDistorted, class View>
__device__ __forceinline__ bool project_pinhole(const View& v, float px, float py, float pz, float tol, float& ox, float& oy) {
    if (pz <= 0.0f) {
        ox = 0.0f;
        oy = 0.0f;
        return false;
    }
    // xy / z as multiplication by one IEEE reciprocal (numerics contract, mirrored by the oracle)
    const float rz = 1.0f / pz;
    const float un = px * rz, vn = py * rz;
    if (!kDistorted) {  // all distortion coefficients are zero: icd == 1, delta == 0 exactly
        ox = un * v.focal_length[0] + v.principal_point[0];
        oy = vn * v.focal_length[1] + v.principal_point[1];
        return within_resolution((float)v.width, (float)v.height, tol, ox, oy);
    }
    const float u2 = un * un, v2 = vn * vn;
    const float r2 = u2 + v2;
    const float a1 = 2.0f * un * vn;
    const float a2 = r2 + 2.0f * u2;
    const float a3 = r2 + 2.0f * v2;
    const float num = 1.0f + r2 * (v.radial[0] + r2 * (v.radial[1] + r2 * v.radial[2]));
    const float den = 1.0f + r2 * (v.radial[3] + r2 * (v.radial[4] + r2 * v.radial[5]));
    const float icd = num / den;
    const float dx = v.tangential[0] * a1 + v.tangential[1] * a2 + r2 * (v.thin_prism[0] + r2 * v.thin_prism[1]);
    const float dy = v.tangential[0] * a3 + v.tangential[1] * a1 + r2 * (v.thin_prism[2] + r2 * v.thin_prism[3]);
    const float xd = icd * un + dx, yd = icd * vn + dy;
    const bool radial_ok = (icd > 0.8f) && (icd < 1.2f);
    if (radial_ok) {
        ox = xd * v.focal_length[0] + v.principal_point[0];
        oy = yd * v.focal_length[1] + v.principal_point[1];
    } else {
        const float fw = (float)v.width, fh = (float)v.height;
        const float clip = sqrtf(fw * fw + fh * fh);
        const float k = clip / sqrtf(r2);
        ox = k * un + v.principal_point[0];
        oy = k * vn + v.principal_point[1];
    }
    return radial_ok && within_resolution((float)v.width, (float)v.height, tol, ox, oy);
}

// OpenCV fisheye, theta clamped to max_angle (cameraProjections.cuh:105-128)
template <class View>
__device__ __forceinline__ bool project_fisheye(const View& v, float px, float py, float pz, float tol, float& ox, float& oy) {
    const float eps = 1.1920929e-07f;
    float rho = sqrtf(px * px + py * py);
    rho = rho > eps ? rho : eps;
    const float theta_full = det_atan2f_pos(rho, pz);
    const float theta = theta_full < v.max_angle ? theta_full : v.max_angle;
    const float t2 = theta * theta;
    float poly = v.radial[3];
    poly = t2 * poly + v.radial[2];
    poly = t2 * poly + v.radial[1];
    poly = t2 * poly + v.radial[0];
    const float delta = (theta * (poly * t2 + 1.0f)) / rho;
    ox = v.focal_length[0] * px * delta + v.principal_point[0];
    oy = v.focal_length[1] * py * delta + v.principal_point[1];
    return (theta < v.max_angle) && within_resolution((float)v.width, (float)v.height, tol, ox, oy);
}

// kVariant: 0 = pinhole without distortion, 1 = pinhole with distortion, 2 = fisheye (compile-time specialisation of
// the reference's run-time camera-model switch, cameraProjections.cuh:130-144)
template <int kVariant, class View>
__device__ __forceinline__ int project_camera(const View& v, float cx, float cy, float cz, float tol, float& ox, float& oy) {
    if (kVariant == 0) return project_pinhole<false>(v, cx, cy, cz, tol, ox, oy) ? 1 : 0;
    if (kVariant == 1) return project_pinhole<true>(v, cx, cy, cz, tol, ox, oy) ? 1 : 0;
    return project_fisheye(v, cx, cy, cz, tol, ox, oy) ? 1 : 0;
}

// which kVariant a camera of `model` (GUT_CAMERA_*) with v's coefficients is; host side
template <class View>
inline int camera_variant(int model, const View& v) {
    bool distorted = false;
    for (float k : v.radial) distorted |= (k != 0.0f);
    for (float k : v.tangential) distorted |= (k != 0.0f);
    for (float k : v.thin_prism) distorted |= (k != 0.0f);
    return model == GUT_CAMERA_OPENCV_FISHEYE ? 2 : (distorted ? 1 : 0);
}

}  // namespace gut
