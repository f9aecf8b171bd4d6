// CIEDE2000 colour difference per pixel and its mean per image, gfx950: the third number of the NTIRE dehazing
// tables beside PSNR and SSIM (csrc/train_io.hip).  One pass over the six planes of two dense fp32 [N,3,H,W] batches.
//
// Definition.  With lab_input == 0 each channel value v of both images becomes
//   c = v > 0 ? min(v, 1) : 0                                    (NaN gives 0: the expression of adh_image_to_u8)
//   l = c <= 0.04045 ? c / 12.92 : ((c + 0.055) / 1.055)^2.4     (sRGB decoding)
//   X = 0.412453 lr + 0.357580 lg + 0.180423 lb
//   Y = 0.212671 lr + 0.715160 lg + 0.072169 lb
//   Z = 0.019334 lr + 0.119193 lg + 0.950227 lb                  then X / 0.95047, Y / 1, Z / 1.08883 (D65 white)
//   f(t) = t > (6/29)^3 ? cbrt(t) : t / (3 (6/29)^2) + 4/29
//   L = 116 f(Y) - 16,  a = 500 (f(X) - f(Y)),  b = 200 (f(Y) - f(Z))
// which are the constants of skimage's rgb2lab.  With lab_input == 1 the three planes hold L, a, b already.  Then the
// Delta E 00 of Sharma, Wu and Dalal (2005), kL = kC = kH = 1, between pixel 1 (pred) and pixel 2 (target):
//   Ci = sqrt(ai^2 + bi^2), Cm = (C1 + C2) / 2, G = (1 - sqrt(Cm^7 / (Cm^7 + 25^7))) / 2, a'i = (1 + G) ai,
//   C'i = sqrt(a'i^2 + bi^2), h'i = atan2(bi, a'i) in degrees in [0, 360), 0 where a'i = bi = 0
//   dL = L2 - L1, dC = C'2 - C'1
//   dh = 0 where C'1 C'2 = 0, else h'2 - h'1 brought into [-180, 180] by -+360 where |h'2 - h'1| > 180
//   dH = 2 sqrt(C'1 C'2) sin(dh / 2)
//   Lm = (L1 + L2) / 2, C'm = (C'1 + C'2) / 2
//   hm = h'1 + h'2 where C'1 C'2 = 0, else (h'1 + h'2) / 2 where |h'1 - h'2| <= 180, else (h'1 + h'2 + 360) / 2 where
//        h'1 + h'2 < 360, else (h'1 + h'2 - 360) / 2
//   T = 1 - 0.17 cos(hm - 30) + 0.24 cos(2 hm) + 0.32 cos(3 hm + 6) - 0.20 cos(4 hm - 63)
//   SL = 1 + 0.015 (Lm - 50)^2 / sqrt(20 + (Lm - 50)^2), SC = 1 + 0.045 C'm, SH = 1 + 0.015 C'm T
//   RT = -sin(2 * 30 exp(-((hm - 275) / 25)^2)) * 2 sqrt(C'm^7 / (C'm^7 + 25^7))
//   dE = sqrt((dL/SL)^2 + (dC/SC)^2 + (dH/SH)^2 + RT (dC/SC) (dH/SH))
// map[n][y][x] = dE, mean[n] = its mean over the image.
//
// Everything from the clamp to the stores is float64, one rounding to fp32 at each store: dE jumps by tenths of a unit where
// two hues are 180 degrees apart, and an fp32 hue takes the other branch there about once per million pixel pairs.  A lane
// owns four neighbouring pixels of a plane: one 16-byte access per plane where both inputs (and map) are 16-byte aligned and
// H * W % 4 == 0, decided once on the host, single floats otherwise; the pixels a lane takes and the order of every sum are the
// same on both paths.  The mean is a two-stage float64 reduction in a fixed order (lane, workgroup tree in LDS, then the
// workgroups' partials), no atomics; the grid's y is the image, so the result for an image does not depend on N.
#include "common.h"

#define CIE_QUAD 4
#define CIE_THREADS 256
#define CIE_PX_PER_BLOCK (CIE_THREADS * CIE_QUAD)
#define CIE_MAX_BLOCKS 2048
#define CIE_DEG 57.295779513082320877    // 180 / pi
#define CIE_RAD 0.017453292519943295769  // pi / 180
#define CIE_25_7 6103515625.0            // 25^7

__device__ __forceinline__ double cie_srgb_linear(float v) {
    const double c = v > 0.0f ? (double)fminf(v, 1.0f) : 0.0;
    return c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4);
}

__device__ __forceinline__ double cie_lab_f(double t) {
    const double d = 6.0 / 29.0;
    return t > d * d * d ? cbrt(t) : t / (3.0 * d * d) + 4.0 / 29.0;
}

template <int LAB>
__device__ __forceinline__ void cie_to_lab(float c0, float c1, float c2, double& L, double& a, double& b) {
    if (LAB) {
        L = c0; a = c1; b = c2;
        return;
    }
    const double r = cie_srgb_linear(c0), g = cie_srgb_linear(c1), bl = cie_srgb_linear(c2);
    const double fx = cie_lab_f((0.412453 * r + 0.357580 * g + 0.180423 * bl) / 0.95047);
    const double fy = cie_lab_f(0.212671 * r + 0.715160 * g + 0.072169 * bl);
    const double fz = cie_lab_f((0.019334 * r + 0.119193 * g + 0.950227 * bl) / 1.08883);
    L = 116.0 * fy - 16.0;
    a = 500.0 * (fx - fy);
    b = 200.0 * (fy - fz);
}

__device__ __forceinline__ double cie_pow7(double c) {
    const double c2 = c * c, c4 = c2 * c2;
    return c4 * c2 * c;
}

__device__ __forceinline__ double cie_hue(double b, double ap) {
    if (ap == 0.0 && b == 0.0) return 0.0;
    const double h = atan2(b, ap) * CIE_DEG;
    return h < 0.0 ? h + 360.0 : h;
}

__device__ __forceinline__ double cie_de00(double L1, double a1, double b1, double L2, double a2, double b2) {
    const double Cm = 0.5 * (sqrt(a1 * a1 + b1 * b1) + sqrt(a2 * a2 + b2 * b2));
    const double Cm7 = cie_pow7(Cm);
    const double G = 0.5 * (1.0 - sqrt(Cm7 / (Cm7 + CIE_25_7)));
    const double ap1 = (1.0 + G) * a1, ap2 = (1.0 + G) * a2;
    const double Cp1 = sqrt(ap1 * ap1 + b1 * b1), Cp2 = sqrt(ap2 * ap2 + b2 * b2);
    const double h1 = cie_hue(b1, ap1), h2 = cie_hue(b2, ap2);
    const double dL = L2 - L1, dC = Cp2 - Cp1;
    const double CC = Cp1 * Cp2;
    const bool grey = CC == 0.0;
    const double hd = h2 - h1, hs = h1 + h2;
    const double dh = grey ? 0.0 : (hd > 180.0 ? hd - 360.0 : (hd < -180.0 ? hd + 360.0 : hd));
    const double dH = 2.0 * sqrt(CC) * sin(0.5 * dh * CIE_RAD);
    const double Lm = 0.5 * (L1 + L2), Cpm = 0.5 * (Cp1 + Cp2);
    const double hm = grey ? hs : (fabs(h1 - h2) <= 180.0 ? 0.5 * hs : (hs < 360.0 ? 0.5 * (hs + 360.0) : 0.5 * (hs - 360.0)));
    const double T = 1.0 - 0.17 * cos((hm - 30.0) * CIE_RAD) + 0.24 * cos(2.0 * hm * CIE_RAD) +
                     0.32 * cos((3.0 * hm + 6.0) * CIE_RAD) - 0.20 * cos((4.0 * hm - 63.0) * CIE_RAD);
    const double l50 = (Lm - 50.0) * (Lm - 50.0);
    const double SL = 1.0 + 0.015 * l50 / sqrt(20.0 + l50);
    const double SC = 1.0 + 0.045 * Cpm;
    const double SH = 1.0 + 0.015 * Cpm * T;
    const double hq = (hm - 275.0) / 25.0;
    const double Cpm7 = cie_pow7(Cpm);
    const double RT = -sin(2.0 * (30.0 * exp(-hq * hq)) * CIE_RAD) * (2.0 * sqrt(Cpm7 / (Cpm7 + CIE_25_7)));
    const double tL = dL / SL, tC = dC / SC, tH = dH / SH;
    // |RT| < 2, so the form is positive semi-definite; the guard only keeps a rounding residue of -1e-30 from becoming a NaN
    return sqrt(fmax(tL * tL + tC * tC + tH * tH + RT * tC * tH, 0.0));
}

// grid (nblk, N): the workgroups of an image walk its quads with a stride of the whole row of workgroups
template <int LAB>
__global__ __launch_bounds__(CIE_THREADS) void ciede2000_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                int64_t HW, int wide, double* __restrict__ partial,
                                                                float* __restrict__ map) {
    __shared__ double red[CIE_THREADS];
    const int n = blockIdx.y;
    const int tid = threadIdx.x;
    const float* __restrict__ pp = pred + (int64_t)n * 3 * HW;
    const float* __restrict__ pt = target + (int64_t)n * 3 * HW;
    float* __restrict__ pm = map ? map + (int64_t)n * HW : nullptr;
    const int64_t nq = (HW + CIE_QUAD - 1) / CIE_QUAD;
    double acc = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * CIE_THREADS + tid; q < nq; q += (int64_t)gridDim.x * CIE_THREADS) {
        const int64_t px = q * CIE_QUAD;
        const int npx = (HW - px) < CIE_QUAD ? (int)(HW - px) : CIE_QUAD;
        float u[3][CIE_QUAD], v[3][CIE_QUAD];
        if (wide) {                      // HW % 4 == 0: every quad is whole
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(pp + c * HW + px);
                const f32x4 b = *reinterpret_cast<const f32x4*>(pt + c * HW + px);
#pragma unroll
                for (int j = 0; j < CIE_QUAD; ++j) { u[c][j] = a[j]; v[c][j] = b[j]; }
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < CIE_QUAD; ++j) {
                    u[c][j] = j < npx ? pp[c * HW + px + j] : 0.0f;
                    v[c][j] = j < npx ? pt[c * HW + px + j] : 0.0f;
                }
        }
        double e[CIE_QUAD];
#pragma unroll
        for (int j = 0; j < CIE_QUAD; ++j) {
            double L1, a1, b1, L2, a2, b2;
            cie_to_lab<LAB>(u[0][j], u[1][j], u[2][j], L1, a1, b1);
            cie_to_lab<LAB>(v[0][j], v[1][j], v[2][j], L2, a2, b2);
            e[j] = j < npx ? cie_de00(L1, a1, b1, L2, a2, b2) : 0.0;
        }
        acc += (e[0] + e[1]) + (e[2] + e[3]);
        if (pm) {
            if (wide) {
                f32x4 o;
#pragma unroll
                for (int j = 0; j < CIE_QUAD; ++j) o[j] = (float)e[j];
                *reinterpret_cast<f32x4*>(pm + px) = o;
            } else {
#pragma unroll
                for (int j = 0; j < CIE_QUAD; ++j)
                    if (j < npx) pm[px + j] = (float)e[j];
            }
        }
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = CIE_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) partial[(int64_t)n * gridDim.x + blockIdx.x] = red[0];
}

__global__ __launch_bounds__(64) void ciede2000_finalize_kernel(const double* __restrict__ partial, int nblk, double inv_count,
                                                                float* __restrict__ mean) {
    __shared__ double red[64];
    const int n = blockIdx.x;
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < nblk; i += 64) acc += partial[(int64_t)n * nblk + i];
    red[tid] = acc;
    __syncthreads();
    for (int s = 32; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) mean[n] = (float)(red[0] * inv_count);
}

extern "C" int adh_ciede2000_num_blocks(int64_t pixels) {
    if (pixels < 1) return ADH_E_ARG;
    const int64_t b = (pixels + CIE_PX_PER_BLOCK - 1) / CIE_PX_PER_BLOCK;
    return b < CIE_MAX_BLOCKS ? (int)b : CIE_MAX_BLOCKS;
}

extern "C" int adh_ciede2000(void* stream, const float* pred_nchw, const float* target_nchw, int N, int H, int W, int lab_input,
                             double* partial, int nblk, float* map, float* mean) {
    if (!pred_nchw || !target_nchw || !partial || !mean || N < 1 || N > 65535 || H < 1 || W < 1) return ADH_E_ARG;
    if (lab_input != 0 && lab_input != 1) return ADH_E_ARG;
    const int64_t HW = (int64_t)H * W;
    if (nblk != adh_ciede2000_num_blocks(HW)) return ADH_E_ARG;
    const uintptr_t p0 = (uintptr_t)pred_nchw, t0 = (uintptr_t)target_nchw, m0 = (uintptr_t)map;
    const uintptr_t map_bytes = (uintptr_t)N * (uintptr_t)HW * sizeof(float), in_bytes = 3 * map_bytes;
    // a lane stores its quad of the map before its neighbours have read theirs: the map may not overlap either image
    if (map && ((m0 < p0 + in_bytes && p0 < m0 + map_bytes) || (m0 < t0 + in_bytes && t0 < m0 + map_bytes))) return ADH_E_ARG;
    const int wide = ((p0 | t0 | m0) & 15) == 0 && (HW & 3) == 0;
    if (lab_input)
        hipLaunchKernelGGL(ciede2000_kernel<1>, dim3(nblk, N), dim3(CIE_THREADS), 0, (hipStream_t)stream, pred_nchw, target_nchw,
                           HW, wide, partial, map);
    else
        hipLaunchKernelGGL(ciede2000_kernel<0>, dim3(nblk, N), dim3(CIE_THREADS), 0, (hipStream_t)stream, pred_nchw, target_nchw,
                           HW, wide, partial, map);
    hipLaunchKernelGGL(ciede2000_finalize_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, partial, nblk, 1.0 / (double)HW,
                       mean);
    return adh_check_launch();
}
