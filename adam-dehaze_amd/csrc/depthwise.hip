// Depthwise convolution (Conv2d(C, C, k, stride, (k-1)/2, groups=C, bias=False)) and the squeeze-excitation channel
// scale of torchvision's MobileNetV2 / V3, gfx950.
//
// 2 k^2 FLOP per 8 bytes moved: no MFMA form is worth having, so these are streaming kernels judged against HBM like the
// BatchNorm ones in bn_act.hip.  Layout shared by every kernel here: a block of 256 threads covers up to 64 channel quads
// (CQB; wider layers take several channel chunks in blockIdx.y) times R = 256 / CQB pixel lanes, channel quads fastest, so
// a wave reads contiguous 16-byte runs of one or more pixels; a thread keeps its channel quad -- and its k^2 x 4 weights in
// registers -- for the whole sweep over the block's `ppb` pixels.  The k^2 taps of neighbouring output pixels overlap and
// are served by L1 / L2: HBM sees each input element about once.  Every reduction (BatchNorm statistics, weight gradient,
// squeeze-excitation gradient) goes through per-block partial rows summed in a fixed order: bit-reproducible, no atomics.
#include "common.h"

#define DW_MAXCQB 64   // channel quads per block

struct DwSplit {
    int CQ, CQB, R, chunks;
};

static inline DwSplit dw_split(int C) {
    DwSplit s;
    s.CQ = C / 4;
    s.CQB = s.CQ < DW_MAXCQB ? s.CQ : DW_MAXCQB;
    s.R = 256 / s.CQB;
    s.chunks = (s.CQ + s.CQB - 1) / s.CQB;
    return s;
}

// pixels per block: about `target` blocks over all channel chunks, between min_ppt and max_ppt pixels per lane
static inline int dw_ppb(int64_t P, const DwSplit& s, int target, int min_ppt, int max_ppt) {
    int64_t want = target / s.chunks;
    if (want < 1) want = 1;
    int64_t ppt = (P + want * s.R - 1) / (want * s.R);
    if (ppt < min_ppt) ppt = min_ppt;
    if (ppt > max_ppt) ppt = max_ppt;
    return (int)(ppt * s.R);
}

static inline int dw_ppb_fwd(int64_t P, const DwSplit& s) { return dw_ppb(P, s, 2048, 2, 16); }
static inline int dw_ppb_wgrad(int64_t P, const DwSplit& s) { return dw_ppb(P, s, 1024, 16, 64); }
static inline int dw_ppb_se(int64_t HW, const DwSplit& s) { return dw_ppb(HW, s, 64, 4, 64); }

__device__ __forceinline__ void dw_lane(int C, int& cq, int& pr, int& R, int& CQB) {
    const int CQ = C >> 2;
    CQB = CQ < DW_MAXCQB ? CQ : DW_MAXCQB;
    R = 256 / CQB;
    cq = blockIdx.y * CQB + (int)(threadIdx.x % CQB);
    pr = (int)(threadIdx.x / CQB);
}

__device__ __forceinline__ f32x4 fma4(const f32x4& a, const f32x4& b, const f32x4& c) {
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = fmaf(a[j], b[j], c[j]);
    return r;
}

// ---------------------------------------------------------------------------------------------------------------------
// weights: w[C][1][k][k] -> wp[k*k][C]
// ---------------------------------------------------------------------------------------------------------------------
__global__ void dwconv_pack_kernel(const float* __restrict__ w, int C, int KK, float* __restrict__ wp) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= C * KK) return;
    const int t = e / C, c = e - t * C;
    wp[e] = w[c * KK + t];
}

extern "C" int adh_dwconv_pack_weights(void* stream, const float* w, const adh_wlayout* L, float* wp) {
    if (!w || !L || !wp || L->Nc < 1 || L->KHt != L->KWt || (L->KHt != 3 && L->KHt != 5)) return ADH_E_ARG;
    const int KK = L->KHt * L->KWt;
    hipLaunchKernelGGL(dwconv_pack_kernel, dim3(adh_ceil_div((int64_t)L->Nc * KK, 256)), dim3(256), 0, (hipStream_t)stream, w,
                       L->Nc, KK, wp);
    return adh_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------
// forward: raw y + BatchNorm partial sums (train) or act(y * scale + shift) (eval)
// ---------------------------------------------------------------------------------------------------------------------
template <int K, int S>
__global__ __launch_bounds__(256) void dwconv_fwd_kernel(const float* __restrict__ x, int x_cs, int IH, int IW, int C,
                                                         const float* __restrict__ wp, float* __restrict__ out, int out_cs,
                                                         int OH, int OW, int64_t P, int ppb, const float* __restrict__ scale,
                                                         const float* __restrict__ shift, int act, float* __restrict__ stats) {
    constexpr int PAD = (K - 1) / 2;
    __shared__ f32x4 red[2][256];
    int cq, pr, R, CQB;
    dw_lane(C, cq, pr, R, CQB);
    const bool active = pr < R && cq < (C >> 2);
    const int c = cq * 4;
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = s1;
    if (active) {
        f32x4 wr[K * K];
#pragma unroll
        for (int t = 0; t < K * K; ++t) wr[t] = *reinterpret_cast<const f32x4*>(wp + (size_t)t * C + c);
        f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
        if (scale) sc = *reinterpret_cast<const f32x4*>(scale + c);
        if (shift) sh = *reinterpret_cast<const f32x4*>(shift + c);
        const int OHW = OH * OW;
        const int64_t p0 = (int64_t)blockIdx.x * ppb;
        const int64_t p1 = p0 + ppb < P ? p0 + ppb : P;
        for (int64_t p = p0 + pr; p < p1; p += R) {
            const int pi = (int)p;
            const int n = pi / OHW;
            const int rem = pi - n * OHW;
            const int oy = rem / OW;
            const int ox = rem - oy * OW;
            const int iy0 = oy * S - PAD, ix0 = ox * S - PAD;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ky = 0; ky < K; ++ky) {
                const int iy = iy0 + ky;
                if ((unsigned)iy >= (unsigned)IH) continue;
                const float* row = x + (int64_t)(n * IH + iy) * IW * x_cs + c;
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const int ix = ix0 + kx;
                    if ((unsigned)ix >= (unsigned)IW) continue;
                    acc = fma4(*reinterpret_cast<const f32x4*>(row + (int64_t)ix * x_cs), wr[ky * K + kx], acc);
                }
            }
            f32x4 o;
            if (stats) {
                s1 += acc;
                s2 = fma4(acc, acc, s2);
                o = acc;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = adh_act_fwd(act, fmaf(acc[j], sc[j], sh[j]));
            }
            __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(out + p * out_cs + c));
        }
    }
    if (stats) {   // uniform over the block
        red[0][threadIdx.x] = s1;
        red[1][threadIdx.x] = s2;
        __syncthreads();
        if ((int)threadIdx.x < CQB && cq < (C >> 2)) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
            for (int r = 0; r < R; ++r) {
                a += red[0][r * CQB + threadIdx.x];
                b += red[1][r * CQB + threadIdx.x];
            }
            *reinterpret_cast<f32x4*>(stats + ((size_t)blockIdx.x * 2 + 0) * C + c) = a;
            *reinterpret_cast<f32x4*>(stats + ((size_t)blockIdx.x * 2 + 1) * C + c) = b;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// data gradient: gather over the output positions that reach each input pixel (stride 1: the flipped correlation; stride
// 2: the <= ceil(k/2)^2 taps of matching parity)
// ---------------------------------------------------------------------------------------------------------------------
template <int K, int S>
__global__ __launch_bounds__(256) void dwconv_dgrad_kernel(const float* __restrict__ g, int g_cs, int OH, int OW, int C,
                                                           const float* __restrict__ wp, float* __restrict__ gx, int gx_cs,
                                                           int IH, int IW, int64_t P, int ppb, int accumulate) {
    constexpr int PAD = (K - 1) / 2;
    int cq, pr, R, CQB;
    dw_lane(C, cq, pr, R, CQB);
    if (pr >= R || cq >= (C >> 2)) return;
    const int c = cq * 4;
    f32x4 wr[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) wr[t] = *reinterpret_cast<const f32x4*>(wp + (size_t)t * C + c);
    const int IHW = IH * IW;
    const int64_t p0 = (int64_t)blockIdx.x * ppb;
    const int64_t p1 = p0 + ppb < P ? p0 + ppb : P;
    for (int64_t p = p0 + pr; p < p1; p += R) {
        const int pi = (int)p;
        const int n = pi / IHW;
        const int rem = pi - n * IHW;
        const int iy = rem / IW;
        const int ix = rem - iy * IW;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int ty = iy + PAD - ky;
            if (ty < 0 || (S == 2 && (ty & 1))) continue;
            const int oy = ty / S;
            if (oy >= OH) continue;
            const float* row = g + (int64_t)(n * OH + oy) * OW * g_cs + c;
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const int tx = ix + PAD - kx;
                if (tx < 0 || (S == 2 && (tx & 1))) continue;
                const int ox = tx / S;
                if (ox >= OW) continue;
                acc = fma4(*reinterpret_cast<const f32x4*>(row + (int64_t)ox * g_cs), wr[ky * K + kx], acc);
            }
        }
        f32x4* dst = reinterpret_cast<f32x4*>(gx + p * gx_cs + c);
        if (accumulate) acc += *dst;
        __builtin_nontemporal_store(acc, dst);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// weight gradient: per-block partials[b][k*k][C], then a fixed-order reduce into dw[C][k*k]
// ---------------------------------------------------------------------------------------------------------------------
template <int K, int S>
__global__ __launch_bounds__(256) void dwconv_wgrad_kernel(const float* __restrict__ x, int x_cs, int IH, int IW, int C,
                                                           const float* __restrict__ g, int g_cs, int OH, int OW, int64_t P,
                                                           int ppb, float* __restrict__ partials) {
    constexpr int PAD = (K - 1) / 2;
    __shared__ f32x4 red[256];
    int cq, pr, R, CQB;
    dw_lane(C, cq, pr, R, CQB);
    const bool active = pr < R && cq < (C >> 2);
    const int c = cq * 4;
    f32x4 acc[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (active) {
        const int OHW = OH * OW;
        const int64_t p0 = (int64_t)blockIdx.x * ppb;
        const int64_t p1 = p0 + ppb < P ? p0 + ppb : P;
        for (int64_t p = p0 + pr; p < p1; p += R) {
            const int pi = (int)p;
            const int n = pi / OHW;
            const int rem = pi - n * OHW;
            const int oy = rem / OW;
            const int ox = rem - oy * OW;
            const int iy0 = oy * S - PAD, ix0 = ox * S - PAD;
            const f32x4 gv = *reinterpret_cast<const f32x4*>(g + p * g_cs + c);
#pragma unroll
            for (int ky = 0; ky < K; ++ky) {
                const int iy = iy0 + ky;
                if ((unsigned)iy >= (unsigned)IH) continue;
                const float* row = x + (int64_t)(n * IH + iy) * IW * x_cs + c;
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const int ix = ix0 + kx;
                    if ((unsigned)ix >= (unsigned)IW) continue;
                    acc[ky * K + kx] = fma4(*reinterpret_cast<const f32x4*>(row + (int64_t)ix * x_cs), gv, acc[ky * K + kx]);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < K * K; ++t) {
        red[threadIdx.x] = acc[t];
        __syncthreads();
        if ((int)threadIdx.x < CQB && cq < (C >> 2)) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            for (int r = 0; r < R; ++r) a += red[r * CQB + threadIdx.x];
            *reinterpret_cast<f32x4*>(partials + ((size_t)blockIdx.x * (K * K) + t) * C + c) = a;
        }
        __syncthreads();
    }
}

__global__ void dwconv_wgrad_reduce_kernel(const float* __restrict__ partials, int nblk, int C, int KK, float* __restrict__ dw,
                                           int accumulate) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;   // e = t * C + c: neighbouring lanes read neighbouring channels
    if (e >= C * KK) return;
    const int t = e / C, c = e - t * C;
    double s0 = 0.0, s1 = 0.0;
    int b = 0;
    for (; b + 1 < nblk; b += 2) {
        s0 += (double)partials[(size_t)b * KK * C + e];
        s1 += (double)partials[(size_t)(b + 1) * KK * C + e];
    }
    if (b < nblk) s0 += (double)partials[(size_t)b * KK * C + e];
    const float v = (float)(s0 + s1);
    dw[c * KK + t] = accumulate ? dw[c * KK + t] + v : v;
}

// ---------------------------------------------------------------------------------------------------------------------
// host entry points
// ---------------------------------------------------------------------------------------------------------------------
static bool dw_args_ok(int C, int k, int stride, int IH, int IW, int OH, int OW, int64_t P, int cs_a, int cs_b) {
    if (C < 4 || (C & 3) || C > 4096 || (k != 3 && k != 5) || (stride != 1 && stride != 2)) return false;
    if (IH < 1 || IW < 1 || OH < 1 || OW < 1 || P < 1 || P > INT32_MAX) return false;
    if (cs_a < C || cs_b < C || (cs_a & 3) || (cs_b & 3)) return false;
    const int pad = (k - 1) / 2;
    return OH == (IH + 2 * pad - k) / stride + 1 && OW == (IW + 2 * pad - k) / stride + 1;
}

#define DW_DISPATCH(KERNEL, GRID, STREAM, ...)                                                                            \
    do {                                                                                                                \
        if (k == 3 && stride == 1) hipLaunchKernelGGL((KERNEL<3, 1>), GRID, dim3(256), 0, STREAM, __VA_ARGS__);          \
        else if (k == 3) hipLaunchKernelGGL((KERNEL<3, 2>), GRID, dim3(256), 0, STREAM, __VA_ARGS__);                    \
        else if (stride == 1) hipLaunchKernelGGL((KERNEL<5, 1>), GRID, dim3(256), 0, STREAM, __VA_ARGS__);               \
        else hipLaunchKernelGGL((KERNEL<5, 2>), GRID, dim3(256), 0, STREAM, __VA_ARGS__);                                \
    } while (0)

extern "C" int adh_dwconv_num_blocks(int64_t P, int C) {
    if (P < 1 || C < 4 || (C & 3)) return ADH_E_ARG;
    const DwSplit s = dw_split(C);
    return adh_ceil_div(P, dw_ppb_fwd(P, s));
}

extern "C" int adh_dwconv_fwd(void* stream, const float* x, int x_cs, int N, int IH, int IW, int C, int k, int stride,
                              const float* wp, float* out, int out_cs, int OH, int OW, const float* scale, const float* shift,
                              int act, float* stats) {
    const int64_t P = (int64_t)N * OH * OW;
    if (!x || !wp || !out || N < 1 || !dw_args_ok(C, k, stride, IH, IW, OH, OW, P, x_cs, out_cs)) return ADH_E_ARG;
    if ((int64_t)N * IH * IW > INT32_MAX || !adh_act_host_valid(act)) return ADH_E_ARG;
    if (stats && (scale || shift || act != ADH_ACT_NONE)) return ADH_E_ARG;   // train mode stores y raw
    const DwSplit s = dw_split(C);
    const int ppb = dw_ppb_fwd(P, s);
    const dim3 grid(adh_ceil_div(P, ppb), s.chunks);
    DW_DISPATCH(dwconv_fwd_kernel, grid, (hipStream_t)stream, x, x_cs, IH, IW, C, wp, out, out_cs, OH, OW, P, ppb, scale, shift,
                act, stats);
    return adh_check_launch();
}

extern "C" int adh_dwconv_dgrad(void* stream, const float* g, int g_cs, int N, int OH, int OW, int C, int k, int stride,
                                const float* wp, float* gx, int gx_cs, int IH, int IW, int accumulate) {
    const int64_t P = (int64_t)N * IH * IW;
    if (!g || !wp || !gx || N < 1 || !dw_args_ok(C, k, stride, IH, IW, OH, OW, P, g_cs, gx_cs)) return ADH_E_ARG;
    const DwSplit s = dw_split(C);
    const int ppb = dw_ppb_fwd(P, s);
    const dim3 grid(adh_ceil_div(P, ppb), s.chunks);
    DW_DISPATCH(dwconv_dgrad_kernel, grid, (hipStream_t)stream, g, g_cs, OH, OW, C, wp, gx, gx_cs, IH, IW, P, ppb, accumulate);
    return adh_check_launch();
}

extern "C" int adh_dwconv_wgrad_num_blocks(int64_t P, int C) {
    if (P < 1 || C < 4 || (C & 3)) return ADH_E_ARG;
    const DwSplit s = dw_split(C);
    return adh_ceil_div(P, dw_ppb_wgrad(P, s));
}

extern "C" int adh_dwconv_wgrad(void* stream, const float* x, int x_cs, int N, int IH, int IW, int C, int k, int stride,
                                const float* g, int g_cs, int OH, int OW, float* partials, int nblk, float* dw, int accumulate) {
    const int64_t P = (int64_t)N * OH * OW;
    if (!x || !g || !partials || !dw || N < 1 || !dw_args_ok(C, k, stride, IH, IW, OH, OW, P, x_cs, g_cs)) return ADH_E_ARG;
    if ((int64_t)N * IH * IW > INT32_MAX) return ADH_E_ARG;
    const DwSplit s = dw_split(C);
    const int ppb = dw_ppb_wgrad(P, s);
    if (nblk != adh_ceil_div(P, ppb)) return ADH_E_ARG;
    const dim3 grid(nblk, s.chunks);
    DW_DISPATCH(dwconv_wgrad_kernel, grid, (hipStream_t)stream, x, x_cs, IH, IW, C, g, g_cs, OH, OW, P, ppb, partials);
    const int KK = k * k;
    hipLaunchKernelGGL(dwconv_wgrad_reduce_kernel, dim3(adh_ceil_div((int64_t)C * KK, 256)), dim3(256), 0, (hipStream_t)stream,
                       partials, nblk, C, KK, dw, accumulate);
    return adh_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------
// squeeze-excitation channel scale and its backward
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void channel_scale_kernel(const float* __restrict__ x, int x_cs, const float* __restrict__ s,
                                                            int HW, int C, float* __restrict__ out, int out_cs) {
    const int CQ = C >> 2;
    const int n = blockIdx.y;
    const int64_t total = (int64_t)HW * CQ;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t p = e / CQ;
        const int c = (int)(e - p * CQ) * 4;
        const int64_t q = (int64_t)n * HW + p;
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + q * x_cs + c);
        const f32x4 sv = *reinterpret_cast<const f32x4*>(s + (size_t)n * C + c);
        *reinterpret_cast<f32x4*>(out + q * out_cs + c) = v * sv;
    }
}

extern "C" int adh_channel_scale(void* stream, const float* x, int x_cs, const float* s, int N, int HW, int C, float* out,
                                 int out_cs) {
    if (!x || !s || !out || N < 1 || HW < 1 || C < 4 || (C & 3) || x_cs < C || out_cs < C || (x_cs & 3) || (out_cs & 3))
        return ADH_E_ARG;
    const int64_t total = (int64_t)HW * (C / 4);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(channel_scale_kernel, dim3((int)blocks, N), dim3(256), 0, (hipStream_t)stream, x, x_cs, s, HW, C, out,
                       out_cs);
    return adh_check_launch();
}

__global__ __launch_bounds__(256) void channel_scale_bwd_kernel(const float* __restrict__ g, int g_cs, const float* __restrict__ x,
                                                                int x_cs, const float* __restrict__ s, int HW, int C, int ppb,
                                                                float* __restrict__ gx, int gx_cs, float* __restrict__ partials) {
    __shared__ f32x4 red[256];
    int cq, pr, R, CQB;
    dw_lane(C, cq, pr, R, CQB);
    const bool active = pr < R && cq < (C >> 2);
    const int c = cq * 4;
    const int n = blockIdx.z;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (active) {
        const f32x4 sv = *reinterpret_cast<const f32x4*>(s + (size_t)n * C + c);
        const int p0 = blockIdx.x * ppb;
        const int p1 = p0 + ppb < HW ? p0 + ppb : HW;
        for (int p = p0 + pr; p < p1; p += R) {
            const int64_t q = (int64_t)n * HW + p;
            const f32x4 gv = *reinterpret_cast<const f32x4*>(g + q * g_cs + c);
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + q * x_cs + c);
            acc = fma4(gv, xv, acc);
            if (gx) *reinterpret_cast<f32x4*>(gx + q * gx_cs + c) = gv * sv;
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if ((int)threadIdx.x < CQB && cq < (C >> 2)) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        for (int r = 0; r < R; ++r) a += red[r * CQB + threadIdx.x];
        *reinterpret_cast<f32x4*>(partials + ((size_t)n * gridDim.x + blockIdx.x) * C + c) = a;
    }
}

__global__ void channel_scale_bwd_reduce_kernel(const float* __restrict__ partials, int nblk, int N, int C, float* __restrict__ gs) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;   // e = n * C + c
    if (e >= N * C) return;
    const int n = e / C, c = e - n * C;
    float a = 0.f;
    for (int b = 0; b < nblk; ++b) a += partials[((size_t)n * nblk + b) * C + c];
    gs[e] = a;
}

extern "C" int adh_channel_scale_bwd_num_blocks(int HW, int C) {
    if (HW < 1 || C < 4 || (C & 3)) return ADH_E_ARG;
    const DwSplit s = dw_split(C);
    return adh_ceil_div(HW, dw_ppb_se(HW, s));
}

extern "C" int adh_channel_scale_bwd(void* stream, const float* g, int g_cs, const float* x, int x_cs, const float* s, int N,
                                     int HW, int C, float* gx, int gx_cs, float* partials, int nblk, float* gs) {
    if (!g || !x || !s || !partials || !gs || N < 1 || HW < 1 || C < 4 || (C & 3) || C > 4096) return ADH_E_ARG;
    if (g_cs < C || x_cs < C || (g_cs & 3) || (x_cs & 3) || (gx && (gx_cs < C || (gx_cs & 3)))) return ADH_E_ARG;
    const DwSplit sp = dw_split(C);
    const int ppb = dw_ppb_se(HW, sp);
    if (nblk != adh_ceil_div(HW, ppb)) return ADH_E_ARG;
    hipLaunchKernelGGL(channel_scale_bwd_kernel, dim3(nblk, sp.chunks, N), dim3(256), 0, (hipStream_t)stream, g, g_cs, x, x_cs, s,
                       HW, C, ppb, gx, gx_cs, partials);
    hipLaunchKernelGGL(channel_scale_bwd_reduce_kernel, dim3(adh_ceil_div((int64_t)N * C, 256)), dim3(256), 0, (hipStream_t)stream,
                       partials, nblk, N, C, gs);
    return adh_check_launch();
}
