// gut_ssim.hip — the image losses and metrics for gfx950: fused SSIM (forward + backward), the fused photometric loss, the
// evaluation metrics.
//
// The model.  The reference's loss calls the external CUDA-only `fused_ssim` package (threedgrut/model/losses.py:17-33,
// requirements.txt:23) right after every render (trainer.py:425-430): mean SSIM with an 11x11 Gaussian window
// (sigma 1.5), C1 = 0.01^2, C2 = 0.03^2, padding="valid" (the 5-pixel border of the SSIM map is excluded from the mean).  Two kernels
// do all of it.  k_ssim_fwd: one 256-thread workgroup per 16x16 output tile and channel stages the (16+10)^2 patch of the PREDICTION
// and of the ground truth in LDS once, runs the separable window horizontally into LDS and vertically in registers, and writes its
// partial sums (SSIM, L1, for the metrics the squared error) and the three derivative maps d(ssim)/d(mu1), d(ssim)/d(sigma1^2),
// d(ssim)/d(sigma12) (the scheme of fused-ssim).  k_ssim_bwd convolves those maps with the window and writes the gradient.  Images are
// addressed through (channel, row, pixel) element strides (ImgView), so the tracer's [1,H,W,3] / [H,W,4] tensors are consumed in place.
//
// Operands.  What the prediction IS is decided where a pixel is loaded (load_pred) and by nothing else:
//     comp_k = rgb_k + B_k (1 - alpha)      B: the view's constant background, or the pixel's own colour in the plane `bg` (kBgImage:
//                                           the reference's `random` background, model/background.py:83-89, a colour, an environment image)
//     pred_c = E [comp; 1]                  kExposure: E = [A | b], a row-major 3x4 array in device memory
//     pred_c, gt_c times mask[y,x]          kMasked (trainer.py:397-404): both images, a halo pixel with ITS OWN mask value
// An operand is one pointer of LossOperands and one template flag of both kernels; an instantiation reads exactly the operands its
// flags name (the others may be null), so a combination without an operand runs code that has never heard of it.  loss_kernels() maps
// the operands a call brings to the instantiation pair.
//
// Post-passes of the fused loss, per pixel on the float4 gradient:
//     k_alpha_grad<kBgImage>     d loss / d alpha = -sum_k B_k g_k, for a background other than constant black (there the backward's 0 stands)
//     k_exposure_grad<kBgImage>  with an exposure the channels mix: the backward leaves g_c = d loss / d pred_c, this turns the three into
//                                A^T g, writes the alpha slot and reduces the 12 sums of dL/dE (k_exposure_finish adds the rows)
// The loss value itself has no pass: workgroup 0 of the backward finishes it (photometric_finish).  The metrics run the forward alone
// (kMetrics: no maps), then k_metrics_finish; the colour-corrected metrics first fit E (k_cc_moments, k_cc_solve) and
// run the same forward with kExposure on it.
#include <array>
#include <cmath>
#include <utility>

#include "gut_internal.h"
#include "gut_fixed.h"

namespace gut {

constexpr int kWin = 11;
constexpr int kHalo = 5;
constexpr int kSTile = 16;
constexpr int kPatch = kSTile + 2 * kHalo;  // 26
constexpr int kRowStride = 48;              // LDS row stride of a patch, see k_ssim_fwd

// Tile of workgroup b: the eight XCDs take workgroups round-robin (b % 8), so neighbouring tiles — whose 26x26 input patches
// overlap by 10 pixels — would sit in eight different L2s and every halo would be fetched from memory again (measured: 2.5x the
// algorithmic bytes).  Each XCD gets one contiguous band of tile rows instead.
__device__ __forceinline__ void xcd_tile(uint32_t b, uint32_t gx, uint32_t gy, int* tx, int* ty) {
    const uint32_t n = gx * gy, full = n >> 3;            // tiles per band; the up to seven tiles beyond 8 * full keep t = b
    const uint32_t t = b < 8u * full ? (b & 7u) * full + (b >> 3) : b;
    *tx = (int)(t % gx); *ty = (int)(t / gx);
}

__constant__ float c_gauss[kWin] = {0.001028380123898387f, 0.0075987582094967365f, 0.036000773310661316f,
                                    0.10936068743467331f,  0.21300552785396576f,   0.26601171493530273f,
                                    0.21300552785396576f,  0.10936068743467331f,   0.036000773310661316f,
                                    0.0075987582094967365f, 0.001028380123898387f};

struct ImgView {
    int H, W, C;
    long long sc, sh, sw;  // element strides: channel, row, pixel
    // fused photometric loss only: img1 is the tracer's [H,W,4] rgba and the compared image is
    // rgb + background * (1 - alpha) (BackgroundColor.forward, model/background.py:78-93); alpha_offset < 0 = plain image
    long long alpha_offset;  // element offset of alpha relative to channel 0 of the same pixel
    float background;        // constant background colour (0 black, 1 white)
};

__device__ __forceinline__ float load_px(const float* __restrict__ img, const ImgView& v, int c, int y, int x) {
    if (x < 0 || y < 0 || x >= v.W || y >= v.H) return 0.0f;
    const long long o = (long long)y * v.sh + (long long)x * v.sw;
    float p = img[o + (long long)c * v.sc];
    if (v.alpha_offset >= 0 && v.background != 0.0f) p += v.background * (1.0f - img[o + v.alpha_offset]);
    return p;
}

// kMasked: the pixel of either image times mask[y,x] ([H,W] floats; the reference multiplies prediction and ground truth by the
// batch's mask before its losses, trainer.py:397-404).  A halo pixel takes ITS OWN mask value, whichever tile it belongs to.
__device__ __forceinline__ float mask_px(const float* __restrict__ mask, const ImgView& v, int y, int x) {
    if (x < 0 || y < 0 || x >= v.W || y >= v.H) return 0.0f;   // (load_px is 0 there: the mask is not read outside the image)
    return mask[(size_t)y * v.W + x];
}

// The optional operands of the fused loss, device pointers: mask [H,W], bg [H,W,3] (interleaved like the ground truth), exposure
// (E, 12 floats).  A kernel instantiation reads only those its template flags name; the others may be null.
struct LossOperands {
    const float* __restrict__ mask = nullptr;
    const float* __restrict__ bg = nullptr;
    const float* __restrict__ exposure = nullptr;
    static constexpr int kCount = 3;
    unsigned present() const { return (mask ? 1u : 0u) | (bg ? 2u : 0u) | (exposure ? 4u : 0u); }   // bit i: operand i is there
};

// kExposure: the three composited channels of a pixel, comp_k = rgb_k + B_k (1 - alpha), B the pixel's own background colour
// (kBgImage) or the constant v.background — one definition for the forward, the backward and the per-pixel pass.
template <bool kBgImage>
__device__ __forceinline__ void composite3(const float* __restrict__ px /* the pixel's rgba */, long long sc, long long alpha_offset,
                                           float background, const float* __restrict__ b3 /* the pixel's B, kBgImage only */,
                                           float* __restrict__ comp) {
    const float oma = 1.0f - px[alpha_offset];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float p = px[(long long)k * sc];
        if constexpr (kBgImage) comp[k] = fmaf(b3[k], oma, p);
        else comp[k] = background != 0.0f ? p + background * oma : p;
    }
}

// kExposure: row c of E, the four floats a workgroup holds in registers (zeros, and nothing read, without an exposure)
template <bool kExposure>
__device__ __forceinline__ void exposure_row(const LossOperands& ops, int c, float (&e4)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) e4[k] = kExposure ? ops.exposure[4 * c + k] : 0.0f;
}

// Channel c of the prediction at (y, x), before the mask factor — the one place that knows what the prediction is, for the forward
// and the backward alike.  Outside the image 0, and nothing is read.
//   neither flag: the rgba pixel over the constant v.background (load_px)
//   kBgImage:     over ITS OWN background colour bg[y,x,c]: rgb + B * (1 - alpha) as one fma (v.background is not used)
//   kExposure:    A[c][0] comp_0 + A[c][1] comp_1 + A[c][2] comp_2 + b_c of the composited pixel, e4 = row c of E
template <bool kBgImage, bool kExposure>
__device__ __forceinline__ float load_pred(const float* __restrict__ img, const ImgView& v, const LossOperands& ops, const float (&e4)[4],
                                           int c, int y, int x) {
    if constexpr (!kBgImage && !kExposure) return load_px(img, v, c, y, x);
    else {
        if (x < 0 || y < 0 || x >= v.W || y >= v.H) return 0.0f;
        const long long o = (long long)y * v.sh + (long long)x * v.sw;
        if constexpr (kExposure) {
            float comp[3];
            composite3<kBgImage>(img + o, v.sc, v.alpha_offset, v.background, kBgImage ? ops.bg + ((size_t)y * v.W + x) * 3 : nullptr, comp);
            return fmaf(e4[0], comp[0], fmaf(e4[1], comp[1], fmaf(e4[2], comp[2], e4[3])));
        } else return fmaf(ops.bg[((size_t)y * v.W + x) * 3 + c], 1.0f - img[o + v.alpha_offset], img[o + (long long)c * v.sc]);
    }
}

// forward: partial sums of the valid-region SSIM map per workgroup + derivative maps (planar [C,H,W])
// kMetrics (gut_image_metrics, no backward follows): the three derivative maps are not stored (their pointers may be null) and the
// workgroup's sum of squared errors goes to partial_sq, next to the L1 partials.
// kBgImage / kExposure: img1 is staged through load_pred<kBgImage, kExposure>, channel c with row c of E.
// kMasked: both patches are staged times the mask, so the SSIM statistics, the L1 partials and the derivative maps are those of the
// two masked images.  The three flags combine freely.
template <bool kMetrics, bool kMasked = false, bool kBgImage = false, bool kExposure = false>
__global__ __launch_bounds__(256) void k_ssim_fwd(ImgView v, ImgView v2, const float* __restrict__ img1,
                                                 const float* __restrict__ img2, float* __restrict__ partial,
                                                 float* __restrict__ partial_l1, float* __restrict__ dm_dmu1,
                                                 float* __restrict__ dm_dsigma1_sq, float* __restrict__ dm_dsigma12,
                                                 uint32_t gx, uint32_t gy, float* __restrict__ partial_sq, LossOperands ops) {
    // row strides chosen for the two 16-lane rows a 32-lane LDS access group covers: 48 = 16 mod 32 for the patches (row r and
    // r + 1 fall on disjoint halves of the 32 banks while the 11-tap window slides), 16 for the filtered rows (ditto for the
    // column pass).  With the earlier 27 / 17 the window passes lost 46 % of their LDS cycles to 2-way conflicts.
    __shared__ float s1[kPatch][kRowStride], s2[kPatch][kRowStride];
    __shared__ float h[5][kPatch][kSTile];  // horizontally filtered: mu1, mu2, x^2, y^2, xy
    __shared__ float red[4];
    const int c = blockIdx.z;
    int tx, ty;
    xcd_tile(blockIdx.x, gx, gy, &tx, &ty);
    const int x0 = tx * kSTile, y0 = ty * kSTile;
    const int tid = threadIdx.x;
    float e4[4];
    exposure_row<kExposure>(ops, c, e4);
    for (int i = tid; i < kPatch * kPatch; i += 256) {
        const int py = i / kPatch, pxx = i - py * kPatch;
        const int y = y0 + py - kHalo, x = x0 + pxx - kHalo;
        float mk = 1.0f;
        if constexpr (kMasked) mk = mask_px(ops.mask, v, y, x);
        s1[py][pxx] = load_pred<kBgImage, kExposure>(img1, v, ops, e4, c, y, x) * mk;
        s2[py][pxx] = load_px(img2, v2, c, y, x) * mk;
    }
    __syncthreads();
    for (int i = tid; i < kPatch * kSTile; i += 256) {
        const int py = i / kSTile, ox = i - py * kSTile;
        float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const float w = c_gauss[k];
            const float p = s1[py][ox + k], q = s2[py][ox + k];
            a += w * p; b += w * q; aa += w * p * p; bb += w * q * q; ab += w * p * q;
        }
        h[0][py][ox] = a; h[1][py][ox] = b; h[2][py][ox] = aa; h[3][py][ox] = bb; h[4][py][ox] = ab;
    }
    __syncthreads();
    const int ox = tid & 15, oy = tid >> 4;
    float mu1 = 0.f, mu2 = 0.f, e11 = 0.f, e22 = 0.f, e12 = 0.f;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
        const float w = c_gauss[k];
        mu1 += w * h[0][oy + k][ox]; mu2 += w * h[1][oy + k][ox];
        e11 += w * h[2][oy + k][ox]; e22 += w * h[3][oy + k][ox]; e12 += w * h[4][oy + k][ox];
    }
    const int x = x0 + ox, y = y0 + oy;
    float val = 0.0f, l1 = 0.0f, sq = 0.0f;
    if (x < v.W && y < v.H) {
        const float d = s1[oy + kHalo][ox + kHalo] - s2[oy + kHalo][ox + kHalo];
        l1 = fabsf(d);
        if constexpr (kMetrics) sq = d * d;
        const float C1 = 0.0001f, C2 = 0.0009f;
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
        const float sg1 = e11 - mu1_sq, sg2 = e22 - mu2_sq, sg12 = e12 - mu12;
        const float A = mu1_sq + mu2_sq + C1, B = sg1 + sg2 + C2, Cc = 2.0f * mu12 + C1, D = 2.0f * sg12 + C2;
        const float m = (Cc * D) / (A * B);
        if constexpr (!kMetrics) {
            const size_t o = ((size_t)c * v.H + y) * v.W + x;
            dm_dmu1[o] = (mu2 * 2.0f * D) / (A * B) - (mu2 * 2.0f * Cc) / (A * B) - (mu1 * 2.0f * Cc * D) / (A * A * B) +
                         (mu1 * 2.0f * Cc * D) / (A * B * B);
            dm_dsigma1_sq[o] = (-Cc * D) / (A * B * B);
            dm_dsigma12[o] = (2.0f * Cc) / (A * B);
        }
        const bool valid = x >= kHalo && y >= kHalo && x < v.W - kHalo && y < v.H - kHalo;
        val = valid ? m : 0.0f;
    }
    for (int mk = 32; mk >= 1; mk >>= 1) val += __shfl_xor(val, mk);
    if ((tid & 63) == 0) red[tid >> 6] = val;
    __syncthreads();
    const int slot = blockIdx.z * gridDim.x + blockIdx.x;
    if (tid == 0) partial[slot] = red[0] + red[1] + red[2] + red[3];
    if (partial_l1) {  // block-uniform
        __syncthreads();
        for (int mk = 32; mk >= 1; mk >>= 1) l1 += __shfl_xor(l1, mk);
        if ((tid & 63) == 0) red[tid >> 6] = l1;
        __syncthreads();
        if (tid == 0) partial_l1[slot] = red[0] + red[1] + red[2] + red[3];
    }
    if constexpr (kMetrics) {
        __syncthreads();
        for (int mk = 32; mk >= 1; mk >>= 1) sq += __shfl_xor(sq, mk);
        if ((tid & 63) == 0) red[tid >> 6] = sq;
        __syncthreads();
        if (tid == 0) partial_sq[slot] = red[0] + red[1] + red[2] + red[3];
    }
}

// deterministic final sum of the per-workgroup partials -> mean SSIM
__global__ __launch_bounds__(256) void k_ssim_finish(const float* __restrict__ partial, int n, float inv_count,
                                                    float* __restrict__ out) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += (double)partial[i];
    for (int mk = 32; mk >= 1; mk >>= 1) acc += __shfl_xor(acc, mk);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (float)((red[0] + red[1] + red[2] + red[3]) * (double)inv_count);
}

// fused photometric loss: out3 = { lambda_l1 * L1 + lambda_ssim * (1 - SSIM), L1, SSIM } from the forward kernel's per-workgroup
// partial sums (fixed summation order: the value does not depend on which workgroup finished when).  Not a launch of its own:
// workgroup 0 of the BACKWARD kernel does it (the partials are complete when that kernel starts, and its other 12 k workgroups
// run meanwhile) — a 16 us single-workgroup launch less on the step's critical path.
struct FinishArgs {
    const float* partial = nullptr;
    const float* partial_l1 = nullptr;
    int n = 0;
    float inv_count_ssim = 0.f, inv_count_l1 = 0.f, lambda_l1 = 0.f, lambda_ssim = 0.f;
    float* out3 = nullptr;   // nullptr: nothing to finish (gut_ssim_backward)
};

// kMetrics (k_metrics_finish): the squared-error partials are summed as well, in the same order, and the output is the four
// floats { MSE, PSNR, SSIM, L1 } (MSE over the same numel as L1); lambda_l1 / lambda_ssim are not used then.
template <bool kMetrics>
__device__ __forceinline__ void photometric_finish(const FinishArgs& fin, const float* __restrict__ partial_sq = nullptr) {
    __shared__ double red[kMetrics ? 3 : 2][4];
    double a = 0.0, b = 0.0, q = 0.0;
    for (int i = threadIdx.x; i < fin.n; i += 256) {
        a += (double)fin.partial[i];
        b += (double)fin.partial_l1[i];
        if constexpr (kMetrics) q += (double)partial_sq[i];
    }
    for (int mk = 32; mk >= 1; mk >>= 1) {
        a += __shfl_xor(a, mk);
        b += __shfl_xor(b, mk);
        if constexpr (kMetrics) q += __shfl_xor(q, mk);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = b;
        if constexpr (kMetrics) red[2][threadIdx.x >> 6] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float ssim = (float)((red[0][0] + red[0][1] + red[0][2] + red[0][3]) * (double)fin.inv_count_ssim);
        const float l1 = (float)((red[1][0] + red[1][1] + red[1][2] + red[1][3]) * (double)fin.inv_count_l1);
        if constexpr (kMetrics) {
            const double mse = (red[2][0] + red[2][1] + red[2][2] + red[2][3]) * (double)fin.inv_count_l1;
            fin.out3[0] = (float)mse;
            fin.out3[1] = mse > 0.0 ? (float)(10.0 * log10(1.0 / mse)) : __builtin_huge_valf();   // PSNR for a data range of 1
            fin.out3[2] = ssim;
            fin.out3[3] = l1;
        } else {
            fin.out3[0] = fin.lambda_l1 * l1 + fin.lambda_ssim * (1.0f - ssim);
            fin.out3[1] = l1;
            fin.out3[2] = ssim;
        }
    }
}

__global__ __launch_bounds__(256) void k_metrics_finish(FinishArgs fin /* out3: the four floats */, const float* __restrict__ partial_sq) {
    photometric_finish<true>(fin, partial_sq);
}

// backward: d(mean ssim)/d(img1) * upstream, written through the same strides as img1
// fused photometric loss (upstream == nullptr): grad = -lambda_ssim * d(mean ssim) + lambda_l1 * sign(p - q) / numel, and
// channel 0's workgroups also write the alpha gradient slot (-background * sum of the colour gradients is added by
// k_alpha_grad for a non-black background; zero for black).
// kMasked (fused photometric loss of a masked view): p and q are the masked pixels the forward saw, and the finished gradient, L1
// term included, is multiplied by mask[y,x] (d image_masked / d rgb); where the mask is 0 it is written as 0.0f whatever g is.
// kBgImage: p is the pixel over its own background colour, as the forward staged it; the alpha slot is written by k_alpha_grad<true>.
// kExposure: p is channel c of the affine image, as the forward staged it, and slot c receives g_c = d loss / d image_c (mask factor
// included), NOT yet the rgb gradient: k_exposure_grad turns the three into A^T g and writes the alpha slot of every pixel.
template <bool kMasked, bool kBgImage = false, bool kExposure = false>
__global__ __launch_bounds__(256) void k_ssim_bwd(ImgView v, ImgView v2, const float* __restrict__ img1,
                                                 const float* __restrict__ img2, const float* __restrict__ dm_dmu1,
                                                 const float* __restrict__ dm_dsigma1_sq, const float* __restrict__ dm_dsigma12,
                                                 const float* __restrict__ upstream, float inv_count, float ssim_weight,
                                                 float l1_weight, float* __restrict__ grad, uint32_t gx, uint32_t gy, FinishArgs fin,
                                                 LossOperands ops) {
    __shared__ float s[3][kPatch][kRowStride];
    __shared__ float h[3][kPatch][kSTile];
    const int c = blockIdx.z;
    float e4[4];
    exposure_row<kExposure>(ops, c, e4);   // before the finish's stores: a load the compiler can prove unclobbered stays scalar
    if (fin.out3 && blockIdx.x == 0 && blockIdx.z == 0) photometric_finish<false>(fin);   // (block-uniform)
    int tx, ty;
    xcd_tile(blockIdx.x, gx, gy, &tx, &ty);
    const int x0 = tx * kSTile, y0 = ty * kSTile;
    const int tid = threadIdx.x;
    const float scale = (upstream ? upstream[0] : ssim_weight) * inv_count;
    for (int i = tid; i < kPatch * kPatch; i += 256) {
        const int py = i / kPatch, pxx = i - py * kPatch;
        const int x = x0 + pxx - kHalo, y = y0 + py - kHalo;
        float a = 0.f, b = 0.f, d = 0.f;
        if (x >= kHalo && y >= kHalo && x < v.W - kHalo && y < v.H - kHalo) {  // d(mean)/d(map) is zero on the border
            const size_t o = ((size_t)c * v.H + y) * v.W + x;
            a = dm_dmu1[o]; b = dm_dsigma1_sq[o]; d = dm_dsigma12[o];
        }
        s[0][py][pxx] = a; s[1][py][pxx] = b; s[2][py][pxx] = d;
    }
    __syncthreads();
    for (int i = tid; i < kPatch * kSTile; i += 256) {
        const int py = i / kSTile, ox = i - py * kSTile;
        float a = 0.f, b = 0.f, d = 0.f;
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const float w = c_gauss[k];
            a += w * s[0][py][ox + k]; b += w * s[1][py][ox + k]; d += w * s[2][py][ox + k];
        }
        h[0][py][ox] = a; h[1][py][ox] = b; h[2][py][ox] = d;
    }
    __syncthreads();
    const int ox = tid & 15, oy = tid >> 4;
    float a = 0.f, b = 0.f, d = 0.f;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
        const float w = c_gauss[k];
        a += w * h[0][oy + k][ox]; b += w * h[1][oy + k][ox]; d += w * h[2][oy + k][ox];
    }
    const int x = x0 + ox, y = y0 + oy;
    if (x < v.W && y < v.H) {
        const long long o = (long long)c * v.sc + (long long)y * v.sh + (long long)x * v.sw;
        float p = load_pred<kBgImage, kExposure>(img1, v, ops, e4, c, y, x), q = load_px(img2, v2, c, y, x);
        float mk = 1.0f;
        if constexpr (kMasked) {
            mk = mask_px(ops.mask, v, y, x);
            p *= mk; q *= mk;
        }
        float g = scale * (a + 2.0f * p * b + q * d);
        if (l1_weight != 0.0f) g += l1_weight * (float)((p > q) - (p < q));
        if constexpr (kMasked) g = mk == 0.0f ? 0.0f : g * mk;
        grad[o] = g;
        if constexpr (!kExposure)
            if (v.alpha_offset >= 0 && c == 0) grad[o + v.alpha_offset] = 0.0f;
    }
}

// d(loss)/d(alpha) for rgb_out = rgb + B * (1 - alpha): -background * (g_r + g_g + g_b) over a constant colour, and with kBgImage
// -(B_r g_r + B_g g_g + B_b g_b), B = bg[pixel] ([H,W,3]; `background` is not used).  The colour gradients of a masked view are
// already multiplied by the mask.
template <bool kBgImage>
__global__ __launch_bounds__(256) void k_alpha_grad(int pixels, float background, const float* __restrict__ bg,
                                                   float* __restrict__ rgba_grad) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < pixels) {
        float4* g = reinterpret_cast<float4*>(rgba_grad) + i;
        float4 t = *g;
        if constexpr (kBgImage) {
            const float* b = bg + (size_t)i * 3;
            t.w = -(b[0] * t.x + b[1] * t.y + b[2] * t.z);
        } else t.w = -background * (t.x + t.y + t.z);
        *g = t;
    }
}

// Exposure, the per-pixel pass behind k_ssim_bwd<.., kExposure>: the pixel's float4 holds g = (g_r, g_g, g_b, unwritten).  Writes
//     d loss / d rgb_k = sum_c A[c][k] g_c,      d loss / d alpha = -sum_k B_k d loss / d rgb_k     (exactly 0.0f for constant black)
// into all four slots and, with `partials`, reduces the 12 sums of dL/dE = [sum g_c comp_k | sum g_c]: kExpPixels pixels per lane, a
// wave butterfly, the four waves added in order, one row of 12 partials per workgroup.  A pixel whose mask is 0 gets four times
// 0.0f and is left out of the sums (its rgba and background are not read).
constexpr int kExpPixels = 4;   // pixels per lane: 1024 per workgroup, 12 partials per 1024 pixels

template <bool kBgImage>
__global__ __launch_bounds__(256) void k_exposure_grad(uint32_t pixels, const float* __restrict__ rgba, const float* __restrict__ bg,
                                                      float background, const float* __restrict__ mask,
                                                      const float* __restrict__ exposure, float* __restrict__ rgba_grad,
                                                      float* __restrict__ partials) {
    __shared__ float red[4][12];
    float E[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) E[k] = exposure[k];
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.0f;
#pragma unroll
    for (int j = 0; j < kExpPixels; ++j) {
        const uint32_t i = (blockIdx.x * kExpPixels + j) * 256u + threadIdx.x;
        if (i >= pixels) break;
        float4* gp = reinterpret_cast<float4*>(rgba_grad) + i;
        if (mask && mask[i] == 0.0f) {   // (g is 0.0f there already; the alpha slot is not: every element is written)
            *gp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            continue;
        }
        const float4 t = *gp;
        const float g[3] = {t.x, t.y, t.z};
        float d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = E[k] * g[0] + E[4 + k] * g[1] + E[8 + k] * g[2];
        const float* b3 = kBgImage ? bg + (size_t)i * 3 : nullptr;
        float da = 0.0f;
        if constexpr (kBgImage) da = -(b3[0] * d[0] + b3[1] * d[1] + b3[2] * d[2]);
        else if (background != 0.0f) da = -background * (d[0] + d[1] + d[2]);
        *gp = make_float4(d[0], d[1], d[2], da);
        if (partials) {   // (block-uniform)
            float comp[3];
            composite3<kBgImage>(rgba + (size_t)i * 4, 1, 3, background, b3, comp);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int k = 0; k < 3; ++k) acc[4 * c + k] += g[c] * comp[k];
                acc[4 * c + 3] += g[c];
            }
        }
    }
    if (!partials) return;
#pragma unroll
    for (int k = 0; k < 12; ++k)
        for (int mk = 32; mk >= 1; mk >>= 1) acc[k] += __shfl_xor(acc[k], mk);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) red[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 12)
        partials[(size_t)blockIdx.x * 12 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// deterministic final sum of the per-workgroup rows of 12 partials, in double: lane = component + 16 * slice; slice s adds the rows
// s, s + 16, ... in order, then component k adds its 16 slices in order
__global__ __launch_bounds__(256) void k_exposure_finish(uint32_t rows, const float* __restrict__ partials, float* __restrict__ out12) {
    __shared__ double red[16][12];
    const uint32_t k = threadIdx.x & 15u, slice = threadIdx.x >> 4;
    if (k < 12) {
        double acc = 0.0;
        for (uint32_t j = slice; j < rows; j += 16u) acc += (double)partials[(size_t)j * 12 + k];
        red[slice][k] = acc;
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        double acc = red[0][threadIdx.x];
        for (int s = 1; s < 16; ++s) acc += red[s][threadIdx.x];
        out12[threadIdx.x] = (float)acc;
    }
}

// The per-pixel rendering error of a view (gut_pixel_error), one lane per pixel: the mean absolute difference of the
// three channels of the prediction — composite3 and the fma chain of load_pred, so the image is the fused loss's — and the ground
// truth, clamped to [0, 1], times the mask.  A pixel whose mask is 0 gets 0.0f and reads nothing else.
template <bool kBgImage, bool kExposure>
__global__ __launch_bounds__(256) void k_pixel_error(size_t pixels, const float* __restrict__ rgba, const float* __restrict__ gt,
                                                    const float* __restrict__ mask, const float* __restrict__ bg, float background,
                                                    const float* __restrict__ exposure, float* __restrict__ error) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= pixels) return;
    const float m = mask ? mask[i] : 1.0f;
    if (m == 0.0f) {
        error[i] = 0.0f;
        return;
    }
    float comp[3];
    composite3<kBgImage>(rgba + i * 4, 1, 3, background, kBgImage ? bg + i * 3 : nullptr, comp);
    float sum = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float img = comp[c];
        if constexpr (kExposure)
            img = fmaf(exposure[4 * c + 0], comp[0], fmaf(exposure[4 * c + 1], comp[1], fmaf(exposure[4 * c + 2], comp[2], exposure[4 * c + 3])));
        sum += fabsf(img - gt[i * 3 + c]);
    }
    const float e = fminf(fmaxf(sum / 3.0f, 0.0f), 1.0f);
    error[i] = mask ? e * m : e;
}

// Adam on the 12 exposure values of ONE view (3dgrut_amd/exposure.py): the view's own moments and visit count, which is advanced
// first and gives the bias correction; betas held in float32, 1 - beta^t formed in double from them and rounded once (the host form
// of ExposureCompensation.end does the same).  One launch of one wave; no contraction, so that the host form can follow it.
__global__ __launch_bounds__(64) void k_exposure_adam(const float* __restrict__ grad12, float* __restrict__ e12, float* __restrict__ m12,
                                                      float* __restrict__ v12, int32_t* __restrict__ count, float lr, float beta1,
                                                      float beta2, float eps) {
#pragma clang fp contract(off)
    const uint32_t k = threadIdx.x;
    const int32_t t = count[0] + 1;   // every lane reads the count before lane 0 stores it (one wave: the barrier below orders them)
    __syncthreads();
    if (k == 0) count[0] = t;
    if (k >= 12) return;
    view_adam_element(grad12[k], e12 + k, m12 + k, v12 + k, t, lr, beta1, beta2, eps);   // gut_fixed.h: shared with the bilateral grids
}

// Colour-corrected metrics (gut_image_metrics_cc), pass 1: the 22 moments of the ridge-regularised affine fit of the
// composited image to the ground truth.  With x = (comp_0, comp_1, comp_2, 1) and y = gt: the 10 distinct sums of x x^T (row-major
// upper triangle: 00 01 02 03 11 12 13 22 23 33) and the 12 sums of x y^T ([4][3], row-major).  The partition of k_exposure_grad
// (kExpPixels pixels per lane, 1024 per workgroup), accumulated in DOUBLE from the first product: fp32 sums move an entry of the
// fitted E by up to 6e-4 on images whose channels correlate.  A wave butterfly, the four waves added in order, one row of 22
// doubles per workgroup; every row is written and nothing is atomic: the sums are a pure function of the inputs.
constexpr int kCcTerms = 22;
constexpr uint32_t kCcBatch = 16;   // k_cc_solve: rows a lane fetches before it adds them, so that the loads overlap

__global__ __launch_bounds__(256) void k_cc_moments(uint32_t pixels, const float* __restrict__ rgba, const float* __restrict__ gt,
                                                   float background, double* __restrict__ partials) {
    __shared__ double red[4][kCcTerms];
    double acc[kCcTerms];
#pragma unroll
    for (int k = 0; k < kCcTerms; ++k) acc[k] = 0.0;
#pragma unroll
    for (int j = 0; j < kExpPixels; ++j) {
        const uint32_t i = (blockIdx.x * kExpPixels + j) * 256u + threadIdx.x;
        if (i >= pixels) break;
        const float4 t = reinterpret_cast<const float4*>(rgba)[i];
        const float px[4] = {t.x, t.y, t.z, t.w};
        float comp[3];
        composite3<false>(px, 1, 3, background, nullptr, comp);
        const double x[4] = {(double)comp[0], (double)comp[1], (double)comp[2], 1.0};
        const float* g = gt + (size_t)i * 3;
        const double y[3] = {(double)g[0], (double)g[1], (double)g[2]};
        int n = 0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int b = a; b < 4; ++b) acc[n++] += x[a] * x[b];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[10 + 3 * a + c] += x[a] * y[c];
        }
    }
#pragma unroll
    for (int k = 0; k < kCcTerms; ++k)
        for (int mk = 32; mk >= 1; mk >>= 1) acc[k] += __shfl_xor(acc[k], mk);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kCcTerms; ++k) red[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < kCcTerms)
        partials[(size_t)blockIdx.x * kCcTerms + threadIdx.x] =
            red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// ... pass 2, one workgroup: the rows are summed in a fixed order (lane = term + 32 * slice; slice s adds the rows s, s + 8, ... in
// order, then term k adds its 8 slices in order, as k_exposure_finish does), then one lane adds the ridge, ridge_p = ridge * pixels on
// the diagonal of G = sum x x^T and on the identity part of C = sum x y^T, factors G = L L^T and solves the three right-hand sides, all
// in double: E^T = G^-1 C, written as 12 floats (row-major 3x4) to e_ws and, if given, to e_out.  With finite inputs and ridge > 0 G is
// positive definite and no pivot can be <= 0; non-finite inputs give non-finite outputs.
__global__ __launch_bounds__(256) void k_cc_solve(uint32_t rows, const double* __restrict__ partials, double ridge_p,
                                                 float* __restrict__ e_ws, float* __restrict__ e_out) {
    __shared__ double red[8][32];
    __shared__ double sum[kCcTerms];
    const uint32_t k = threadIdx.x & 31u, slice = threadIdx.x >> 5;
    if (k < (uint32_t)kCcTerms) {
        double acc = 0.0;
        for (uint32_t j = slice; j < rows; j += 8u * kCcBatch) {   // kCcBatch loads in flight, added in row order (+ 0.0 past the end)
            double v[kCcBatch];
#pragma unroll
            for (uint32_t u = 0; u < kCcBatch; ++u) {
                const uint32_t r = j + 8u * u;
                v[u] = r < rows ? partials[(size_t)r * kCcTerms + k] : 0.0;
            }
#pragma unroll
            for (uint32_t u = 0; u < kCcBatch; ++u) acc += v[u];
        }
        red[slice][k] = acc;
    }
    __syncthreads();
    if (threadIdx.x < kCcTerms) {
        double acc = red[0][threadIdx.x];
        for (int s = 1; s < 8; ++s) acc += red[s][threadIdx.x];
        sum[threadIdx.x] = acc;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double G[4][4], C[4][3], L[4][4];
    int n = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int b = a; b < 4; ++b) {
            G[a][b] = G[b][a] = sum[n++] + (a == b ? ridge_p : 0.0);
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) C[a][c] = sum[10 + 3 * a + c] + (a == c ? ridge_p : 0.0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double d = G[j][j];
#pragma unroll
        for (int m = 0; m < j; ++m) d -= L[j][m] * L[j][m];
        L[j][j] = sqrt(d);
#pragma unroll
        for (int i = j + 1; i < 4; ++i) {
            double s = G[i][j];
#pragma unroll
            for (int m = 0; m < j; ++m) s -= L[i][m] * L[j][m];
            L[i][j] = s / L[j][j];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double z[4], w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {   // L z = C[:, c]
            double s = C[i][c];
#pragma unroll
            for (int m = 0; m < i; ++m) s -= L[i][m] * z[m];
            z[i] = s / L[i][i];
        }
#pragma unroll
        for (int i = 3; i >= 0; --i) {  // L^T w = z
            double s = z[i];
#pragma unroll
            for (int m = i + 1; m < 4; ++m) s -= L[m][i] * w[m];
            w[i] = s / L[i][i];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const float e = (float)w[a];
            e_ws[4 * c + a] = e;
            if (e_out) e_out[4 * c + a] = e;
        }
    }
}

// The fused loss's instantiation pair for every set of operands, indexed by LossOperands::present().  One more operand is one more
// flag in loss_pair (and its field and bit in LossOperands).
struct LossKernels {
    decltype(&k_ssim_fwd<false>) fwd;
    decltype(&k_ssim_bwd<false>) bwd;
};
template <size_t B>
constexpr LossKernels loss_pair = {k_ssim_fwd<false, (B & 1) != 0, (B & 2) != 0, (B & 4) != 0>, k_ssim_bwd<(B & 1) != 0, (B & 2) != 0, (B & 4) != 0>};
template <size_t... B>
constexpr std::array<LossKernels, sizeof...(B)> loss_table(std::index_sequence<B...>) { return {{loss_pair<B>...}}; }

static LossKernels loss_kernels(const LossOperands& ops) {
    static constexpr auto table = loss_table(std::make_index_sequence<(1 << LossOperands::kCount)>());
    return table[ops.present()];
}

// What every entry point derives from (channels, height, width): the tile grid, the two interleaved views of the fused loss, the
// means' denominators and where the partial arrays lie (nblocks floats each, 64 floats of slack after the first two).
struct LossGeometry {
    int32_t C, H, W;
    uint32_t gx, gy;
    dim3 grid;
    int nblocks;
    size_t plane;          // elements of one derivative map
    double count, numel;   // valid-region SSIM values, image elements
    LossGeometry(int32_t channels, int32_t height, int32_t width)
        : C(channels), H(height), W(width), gx((width + 15) / 16), gy((height + 15) / 16), grid(gx * gy, 1, channels),
          nblocks((int)(grid.x * grid.z)), plane((size_t)channels * height * width),
          count((double)channels * (height - 2 * kHalo) * (width - 2 * kHalo)), numel((double)channels * height * width) {}
    static bool too_small(int32_t height, int32_t width) { return height <= 2 * kHalo || width <= 2 * kHalo; }
    ImgView view(int64_t sc, int64_t sh, int64_t sw, long long alpha_offset = -1, float background = 0.0f) const {
        ImgView v;
        v.C = C; v.H = H; v.W = W; v.sc = sc; v.sh = sh; v.sw = sw;
        v.alpha_offset = alpha_offset;
        v.background = background;
        return v;
    }
    ImgView rgba(float background) const { return view(1, 4 * (int64_t)W, 4, 3, background); }   // the tracer's [H,W,4], interleaved
    ImgView rgb() const { return view(1, 3 * (int64_t)W, 3); }                                    // ground truth [H,W,3], interleaved
    float* partial_l1(float* partial) const { return partial + nblocks + 64; }
    float* partial_sq(float* partial) const { return partial_l1(partial) + nblocks + 64; }
    FinishArgs finish(float* partial, float lambda_l1, float lambda_ssim, float* out) const {
        FinishArgs fin;
        fin.partial = partial; fin.partial_l1 = partial_l1(partial); fin.n = nblocks;
        fin.inv_count_ssim = (float)(1.0 / count); fin.inv_count_l1 = (float)(1.0 / numel);
        fin.lambda_l1 = lambda_l1; fin.lambda_ssim = lambda_ssim; fin.out3 = out;
        return fin;
    }
};

}  // namespace gut

extern "C" {

size_t gut_ssim_workspace_bytes(int32_t channels, int32_t height, int32_t width) {
    const size_t maps = (size_t)3 * channels * height * width * sizeof(float);
    const size_t tiles = (size_t)((width + 15) / 16) * ((height + 15) / 16) * channels * sizeof(float);
    return maps + tiles + 256;
}

int gut_ssim_forward(void* stream, int32_t channels, int32_t height, int32_t width, int64_t stride_c, int64_t stride_h,
                     int64_t stride_w, const float* d_img1, const float* d_img2, void* d_workspace, float* d_mean_ssim) {
    if (!d_img1 || !d_img2 || !d_workspace || !d_mean_ssim || channels <= 0) return 1;
    if (gut::LossGeometry::too_small(height, width)) return 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const gut::LossGeometry geo(channels, height, width);
    float* maps = static_cast<float*>(d_workspace);
    float* partial = maps + 3 * geo.plane;
    const gut::ImgView v = geo.view(stride_c, stride_h, stride_w);
    hipLaunchKernelGGL(gut::k_ssim_fwd<false>, geo.grid, dim3(256), 0, s, v, v, d_img1, d_img2, partial, (float*)nullptr, maps,
                       maps + geo.plane, maps + 2 * geo.plane, geo.gx, geo.gy, (float*)nullptr, gut::LossOperands{});
    hipLaunchKernelGGL(gut::k_ssim_finish, dim3(1), dim3(256), 0, s, partial, geo.nblocks, (float)(1.0 / geo.count), d_mean_ssim);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

int gut_ssim_backward(void* stream, int32_t channels, int32_t height, int32_t width, int64_t stride_c, int64_t stride_h,
                      int64_t stride_w, const float* d_img1, const float* d_img2, const void* d_workspace,
                      const float* d_upstream /* 1 float */, float* d_grad_img1) {
    if (!d_img1 || !d_img2 || !d_workspace || !d_upstream || !d_grad_img1) return 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const gut::LossGeometry geo(channels, height, width);
    const float* maps = static_cast<const float*>(d_workspace);
    const gut::ImgView v = geo.view(stride_c, stride_h, stride_w);
    hipLaunchKernelGGL(gut::k_ssim_bwd<false>, geo.grid, dim3(256), 0, s, v, v, d_img1, d_img2, maps, maps + geo.plane, maps + 2 * geo.plane,
                       d_upstream, (float)(1.0 / geo.count), 0.0f, 0.0f, d_grad_img1, geo.gx, geo.gy, gut::FinishArgs(), gut::LossOperands{});
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

size_t gut_photometric_workspace_bytes(int32_t height, int32_t width) {
    const size_t tiles = (size_t)((width + 15) / 16) * ((height + 15) / 16) * 3 * sizeof(float);
    return gut_ssim_workspace_bytes(3, height, width) + tiles;
}

size_t gut_photometric_exposure_workspace_bytes(int32_t height, int32_t width) {
    const size_t rows = ((size_t)height * width + 256 * gut::kExpPixels - 1) / (256 * gut::kExpPixels);
    return gut_photometric_workspace_bytes(height, width) + rows * 12 * sizeof(float) + 256;
}

// The fused loss of one view.  The operands the descriptor brings choose the instantiation pair (loss_kernels) and the post-pass:
// with an exposure k_exposure_grad for every background (the channels mix) and, if the 12 sums are wanted, k_exposure_finish on the
// rows of partials, which follow everything gut_photometric_workspace_bytes covers (partial_l1 ends exactly there); without one
// k_alpha_grad, unless the background is constant black.  The loss value is finished in the backward (FinishArgs).
int gut_photometric_loss_run(void* stream, int32_t height, int32_t width, const GutPhotometricLoss* d) {
    static_assert(sizeof(GutPhotometricLoss) == 88, "GutPhotometricLoss: nine pointers, three floats (include/gut_hip.h)");
    if (!d || !d->d_rgba || !d->d_gt_rgb || !d->d_workspace || !d->d_loss3 || !d->d_rgba_grad) return 1;
    if (d->d_exposure_grad12 && !d->d_exposure12) return 1;
    if (gut::LossGeometry::too_small(height, width)) return 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const gut::LossGeometry geo(3, height, width);
    const gut::LossOperands ops{d->d_mask, d->d_background, d->d_exposure12};
    const float background = ops.bg ? 0.0f : d->background;   // (not used with a plane)
    float* maps = static_cast<float*>(d->d_workspace);
    float* partial = maps + 3 * geo.plane;
    const gut::ImgView v = geo.rgba(background), g = geo.rgb();
    const gut::LossKernels k = gut::loss_kernels(ops);
    hipLaunchKernelGGL(k.fwd, geo.grid, dim3(256), 0, s, v, g, d->d_rgba, d->d_gt_rgb, partial, geo.partial_l1(partial), maps,
                       maps + geo.plane, maps + 2 * geo.plane, geo.gx, geo.gy, (float*)nullptr, ops);
    const float* no_upstream = nullptr;   // the fused loss has no upstream gradient: the weights below
    hipLaunchKernelGGL(k.bwd, geo.grid, dim3(256), 0, s, v, g, d->d_rgba, d->d_gt_rgb, maps, maps + geo.plane, maps + 2 * geo.plane, no_upstream,
                       (float)(1.0 / geo.count), -d->lambda_ssim, (float)(d->lambda_l1 / geo.numel), d->d_rgba_grad, geo.gx, geo.gy,
                       geo.finish(partial, d->lambda_l1, d->lambda_ssim, d->d_loss3), ops);
    const int pixels = height * width;
    if (ops.exposure) {
        float* partial_e = d->d_exposure_grad12 ? geo.partial_l1(partial) + geo.nblocks : nullptr;
        const uint32_t rows = ((uint32_t)pixels + 256 * gut::kExpPixels - 1) / (256 * gut::kExpPixels);
        hipLaunchKernelGGL(ops.bg ? gut::k_exposure_grad<true> : gut::k_exposure_grad<false>, dim3(rows), dim3(256), 0, s, (uint32_t)pixels,
                           d->d_rgba, ops.bg, background, ops.mask, ops.exposure, d->d_rgba_grad, partial_e);
        if (partial_e) hipLaunchKernelGGL(gut::k_exposure_finish, dim3(1), dim3(256), 0, s, rows, partial_e, d->d_exposure_grad12);
    } else if (ops.bg || background != 0.0f)
        hipLaunchKernelGGL(ops.bg ? gut::k_alpha_grad<true> : gut::k_alpha_grad<false>, dim3((pixels + 255) / 256), dim3(256), 0, s, pixels,
                           background, ops.bg, d->d_rgba_grad);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// The four positional forms: each fills the descriptor with what it has.
int gut_photometric_loss(void* stream, int32_t height, int32_t width, const float* d_rgba, const float* d_gt_rgb, float background,
                         float lambda_l1, float lambda_ssim, void* d_workspace, float* d_loss3, float* d_rgba_grad) {
    const GutPhotometricLoss d{d_rgba, d_gt_rgb, nullptr, nullptr, nullptr, d_workspace, d_loss3, d_rgba_grad, nullptr, background, lambda_l1, lambda_ssim};
    return gut_photometric_loss_run(stream, height, width, &d);
}

int gut_photometric_loss_masked(void* stream, int32_t height, int32_t width, const float* d_rgba, const float* d_gt_rgb,
                                const float* d_mask, float background, float lambda_l1, float lambda_ssim, void* d_workspace,
                                float* d_loss3, float* d_rgba_grad) {
    const GutPhotometricLoss d{d_rgba, d_gt_rgb, d_mask, nullptr, nullptr, d_workspace, d_loss3, d_rgba_grad, nullptr, background, lambda_l1, lambda_ssim};
    return gut_photometric_loss_run(stream, height, width, &d);
}

int gut_photometric_loss_background(void* stream, int32_t height, int32_t width, const float* d_rgba, const float* d_gt_rgb,
                                    const float* d_mask, const float* d_background, float lambda_l1, float lambda_ssim,
                                    void* d_workspace, float* d_loss3, float* d_rgba_grad) {
    if (!d_background) return 1;
    const GutPhotometricLoss d{d_rgba, d_gt_rgb, d_mask, d_background, nullptr, d_workspace, d_loss3, d_rgba_grad, nullptr, 0.0f, lambda_l1, lambda_ssim};
    return gut_photometric_loss_run(stream, height, width, &d);
}

int gut_photometric_loss_exposure(void* stream, int32_t height, int32_t width, const float* d_rgba, const float* d_gt_rgb,
                                  const float* d_mask, const float* d_background, float background, const float* d_exposure12,
                                  float lambda_l1, float lambda_ssim, void* d_workspace, float* d_loss3, float* d_rgba_grad,
                                  float* d_exposure_grad12) {
    if (!d_exposure12) return 1;
    const GutPhotometricLoss d{d_rgba, d_gt_rgb, d_mask, d_background, d_exposure12, d_workspace, d_loss3, d_rgba_grad, d_exposure_grad12,
                               background, lambda_l1, lambda_ssim};
    return gut_photometric_loss_run(stream, height, width, &d);
}

int gut_exposure_adam_step(void* stream, const float* d_grad12, float* d_exposure12, float* d_m12, float* d_v12, int32_t* d_count,
                           float lr, float beta1, float beta2, float eps) {
    if (!d_grad12 || !d_exposure12 || !d_m12 || !d_v12 || !d_count) return 1;
    hipLaunchKernelGGL(gut::k_exposure_adam, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), d_grad12, d_exposure12, d_m12,
                       d_v12, d_count, lr, beta1, beta2, eps);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// One elementwise launch, no workspace; the optional operands as in the fused loss.
int gut_pixel_error(void* stream, int32_t height, int32_t width, const float* d_rgba, const float* d_gt_rgb, const float* d_mask,
                    const float* d_background, float background, const float* d_exposure12, float* d_error) {
    if (!d_rgba || !d_gt_rgb || !d_error || height < 1 || width < 1) return 1;
    const size_t pixels = (size_t)height * (size_t)width;
    const auto kernel = d_background ? (d_exposure12 ? gut::k_pixel_error<true, true> : gut::k_pixel_error<true, false>)
                                     : (d_exposure12 ? gut::k_pixel_error<false, true> : gut::k_pixel_error<false, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pixels, d_rgba,
                       d_gt_rgb, d_mask, d_background, background, d_exposure12, d_error);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// three arrays of per-workgroup partials (SSIM, L1, squared error; 3 channels x tiles entries, 64 floats of slack after each)
size_t gut_image_metrics_workspace_bytes(int32_t height, int32_t width) {
    const size_t blocks = (size_t)((width + 15) / 16) * ((height + 15) / 16) * 3;
    return 3 * (blocks + 64) * sizeof(float) + 256;
}

// The metrics forward and its finish: the three partial arrays lie at the start of the workspace.  d_exposure: null, or the E the
// image is mapped through first (the kExposure instantiation).
static int metrics_forward_finish(hipStream_t s, int32_t height, int32_t width, const float* d_rgba, const float* d_gt_rgb, float background,
                                  const float* d_exposure, void* d_workspace, float* d_out4) {
    const gut::LossGeometry geo(3, height, width);
    float* partial = static_cast<float*>(d_workspace);
    gut::LossOperands ops;
    ops.exposure = d_exposure;
    hipLaunchKernelGGL((d_exposure ? gut::k_ssim_fwd<true, false, false, true> : gut::k_ssim_fwd<true>), geo.grid, dim3(256), 0, s,
                       geo.rgba(background), geo.rgb(), d_rgba, d_gt_rgb, partial, geo.partial_l1(partial), (float*)nullptr, (float*)nullptr,
                       (float*)nullptr, geo.gx, geo.gy, geo.partial_sq(partial), ops);
    hipLaunchKernelGGL(gut::k_metrics_finish, dim3(1), dim3(256), 0, s, geo.finish(partial, 0.f, 0.f, d_out4),
                       (const float*)geo.partial_sq(partial));
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

int gut_image_metrics(void* stream, int32_t height, int32_t width, const float* d_rgba, const float* d_gt_rgb, float background,
                      void* d_workspace, float* d_out4) {
    if (!d_rgba || !d_gt_rgb || !d_workspace || !d_out4) return 1;
    if (gut::LossGeometry::too_small(height, width)) return 1;
    return metrics_forward_finish(static_cast<hipStream_t>(stream), height, width, d_rgba, d_gt_rgb, background, nullptr, d_workspace, d_out4);
}

// the workspace of gut_image_metrics (rounded up to 16 bytes), then one row of 22 doubles per 1024 pixels, then the fitted E (12 floats)
static size_t cc_rows(int32_t height, int32_t width) {
    return ((size_t)height * width + 256 * gut::kExpPixels - 1) / (256 * gut::kExpPixels);
}
static size_t cc_moments_offset(int32_t height, int32_t width) {
    return (gut_image_metrics_workspace_bytes(height, width) + 15) / 16 * 16;
}

size_t gut_image_metrics_cc_workspace_bytes(int32_t height, int32_t width) {
    if (height <= 0 || width <= 0) return 0;
    return cc_moments_offset(height, width) + cc_rows(height, width) * gut::kCcTerms * sizeof(double) + 64;
}

int gut_image_metrics_cc(void* stream, int32_t height, int32_t width, const float* d_rgba, const float* d_gt_rgb, float background,
                         float ridge, void* d_workspace, float* d_out4, float* d_exposure12) {
    if (!d_rgba || !d_gt_rgb || !d_workspace || !d_out4) return 1;
    if (gut::LossGeometry::too_small(height, width)) return 1;
    if (!(ridge > 0.0f) || !std::isfinite(ridge)) return 1;
    if (reinterpret_cast<uintptr_t>(d_workspace) % 8 != 0) return 1;   // (the rows of doubles)
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t rows = (uint32_t)cc_rows(height, width);
    double* moments = reinterpret_cast<double*>(static_cast<char*>(d_workspace) + cc_moments_offset(height, width));
    float* fitted = reinterpret_cast<float*>(moments + (size_t)rows * gut::kCcTerms);
    const uint32_t pixels = (uint32_t)height * (uint32_t)width;
    hipLaunchKernelGGL(gut::k_cc_moments, dim3(rows), dim3(256), 0, s, pixels, d_rgba, d_gt_rgb, background, moments);
    hipLaunchKernelGGL(gut::k_cc_solve, dim3(1), dim3(256), 0, s, rows, (const double*)moments, (double)ridge * (double)pixels, fitted,
                       d_exposure12);
    return metrics_forward_finish(s, height, width, d_rgba, d_gt_rgb, background, fitted, d_workspace, d_out4);
}

}  // extern "C"
