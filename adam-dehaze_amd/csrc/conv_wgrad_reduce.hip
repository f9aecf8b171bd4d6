// Reduce stage of every weight gradient: the accumulating kernels (conv_wgrad.hip, conv_wgrad_small.hip, conv_wgrad32.hip,
// conv_wgrad43.hip, conv_stem.hip) write partial slabs, one per pixel split or workgroup; the kernels here add them in a fixed
// order (deterministic, no atomics) and scatter the result through the layout `L` into the weight-gradient tensor,
//     dst[adh_wlayout_off(L, ty, tx, k, n)] (+)= value            (`accumulate`: add to what dst holds)
//   * slabs in the tap domain, slab[s][tap][KP][NcP]: three summation orders, kept as they are because their results are pinned
//     bit for bit -- four accumulators per thread (adh_wgrad_reduce), one wave per element (adh_wgrad_reduce_small: hundreds of
//     slabs, few elements), two accumulators over the packed 7x7-stem slabs (adh_wgrad_reduce_packed, its own index decode);
//   * slabs in a Winograd domain, slab[s][class][plane][KP][NcP]: the splits are first stream-summed into split 0
//     (adh_wgrad_sum_splits), then one kernel template applies the domain's inverse transform per (class, k, n).
// The real sizes L.K x L.Nc may be smaller than the padded KP x NcP of the slabs; only the real elements are read and written.
#include "common.h"

// flat element index -> (t, k, n), n fastest; t is the tap of the tap-domain kernels, the class of the Winograd-domain ones
struct WrElem {
    int t, k, n;
};
__host__ __device__ static inline WrElem wr_elem(int64_t idx, const adh_wlayout& L) {
    const int n = (int)(idx % L.Nc);
    const int64_t r = idx / L.Nc;
    return {(int)(r / L.K), (int)(r % L.K), n};
}
__host__ __device__ static inline void wr_store(float* dst, const adh_wlayout& L, int ty, int tx, int k, int n, float v,
                                                int accumulate) {
    const int64_t off = adh_wlayout_off(L, ty, tx, k, n);
    dst[off] = accumulate ? dst[off] + v : v;
}

// dst(layout L) (+)= sum over splits, fixed order
__global__ void wgrad_reduce_kernel(const float* __restrict__ slab, int nsplit, int KP, int NcP, const adh_wlayout L,
                                    float* __restrict__ dst, int accumulate) {
    const int T = L.KHt * L.KWt;
    const int64_t total = (int64_t)T * L.K * L.Nc;
    const int64_t split_stride = (int64_t)T * KP * NcP;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const WrElem e = wr_elem(idx, L);
        const float* p = slab + ((int64_t)e.t * KP + e.k) * NcP + e.n;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int s = 0;
        for (; s + 4 <= nsplit; s += 4) {
            s0 += p[(int64_t)(s + 0) * split_stride];
            s1 += p[(int64_t)(s + 1) * split_stride];
            s2 += p[(int64_t)(s + 2) * split_stride];
            s3 += p[(int64_t)(s + 3) * split_stride];
        }
        for (; s < nsplit; ++s) s0 += p[(int64_t)s * split_stride];
        wr_store(dst, L, e.t / L.KWt, e.t % L.KWt, e.k, e.n, (s0 + s1) + (s2 + s3), accumulate);
    }
}

extern "C" int adh_wgrad_reduce(void* stream, const float* slab, int nsplit, int KP, int NcP, const adh_wlayout* L,
                                float* dst, int accumulate) {
    if (!slab || !L || !dst || nsplit < 1) return ADH_E_ARG;
    const int64_t total = (int64_t)L->KHt * L->KWt * L->K * L->Nc;
    const int blocks = adh_min_i(adh_ceil_div(total, 256), 8192);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, slab, nsplit, KP, NcP, *L,
                       dst, accumulate);
    return adh_check_launch();
}

// dst(layout L) (+)= sum over slabs[s][tap][k][n]: one wave per output element (few outputs, hundreds of slabs: the
// thread-per-output kernel above would run one long dependent chain per thread)
__global__ __launch_bounds__(256) void wgrad_reduce_wave_kernel(const float* __restrict__ slab, int nslabs, int KP, int NcP,
                                                                const adh_wlayout L, float* __restrict__ dst, int accumulate) {
    const int T = L.KHt * L.KWt;
    const int64_t total = (int64_t)T * L.K * L.Nc;
    const int64_t split_stride = (int64_t)T * KP * NcP;
    const int lane = threadIdx.x & 63;
    for (int64_t idx = blockIdx.x * 4 + (threadIdx.x >> 6); idx < total; idx += (int64_t)gridDim.x * 4) {
        const WrElem e = wr_elem(idx, L);
        const float* p = slab + ((int64_t)e.t * KP + e.k) * NcP + e.n;
        float s = 0.f;
        for (int i = lane; i < nslabs; i += 64) s += p[(int64_t)i * split_stride];
        s = wave_sum(s);
        if (lane == 0) wr_store(dst, L, e.t / L.KWt, e.t % L.KWt, e.k, e.n, s, accumulate);
    }
}

extern "C" int adh_wgrad_reduce_small(void* stream, const float* slab, int nslabs, int KP, int NcP, const adh_wlayout* L,
                                      float* dst, int accumulate) {
    if (!slab || !L || !dst || nslabs < 1) return ADH_E_ARG;
    const int64_t total = (int64_t)L->KHt * L->KWt * L->K * L->Nc;
    hipLaunchKernelGGL(wgrad_reduce_wave_kernel, dim3(adh_min_i(adh_ceil_div(total, 4), 4096)), dim3(256), 0, (hipStream_t)stream,
                       slab, nslabs, KP, NcP, *L, dst, accumulate);
    return adh_check_launch();
}

// Packed small-Cin slabs: slab[s][tap=(ky*KWg+kxg)][i=(kxl*8+ci)][NcP] -> dst OIHW [Cout][Cin][KH][KW]
__global__ void wgrad_reduce_packed_kernel(const float* __restrict__ slab, int nsplit, int NcP, int Cin, int KH, int KW,
                                           int Cout, float* __restrict__ dst, int accumulate) {
    const adh_wlayout oihw = {Cin, Cout, KH, KW, 0, KW, 1, KH * KW, Cin * KH * KW};
    const int KWg = (KW + 3) / 4;
    const int64_t total = (int64_t)Cout * Cin * KH * KW;
    const int64_t split_stride = (int64_t)KH * KWg * 32 * NcP;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int kx = (int)(idx % KW);
        int64_t r = idx / KW;
        const int ky = (int)(r % KH);
        r /= KH;
        const int ci = (int)(r % Cin);
        const int co = (int)(r / Cin);
        const int tap = ky * KWg + (kx >> 2);
        const int i = (kx & 3) * 8 + ci;
        const float* p = slab + ((int64_t)tap * 32 + i) * NcP + co;
        float s0 = 0.f, s1 = 0.f;
        int s = 0;
        for (; s + 2 <= nsplit; s += 2) {
            s0 += p[(int64_t)s * split_stride];
            s1 += p[(int64_t)(s + 1) * split_stride];
        }
        if (s < nsplit) s0 += p[(int64_t)s * split_stride];
        wr_store(dst, oihw, ky, kx, ci, co, s0 + s1, accumulate);
    }
}

extern "C" int adh_wgrad_reduce_packed(void* stream, const float* slab, int nsplit, int NcP, int Cin, int KH, int KW, int Cout,
                                       float* dst, int accumulate) {
    if (!slab || !dst || nsplit < 1 || Cin < 1 || Cin > 8) return ADH_E_ARG;
    const int64_t total = (int64_t)Cout * Cin * KH * KW;
    hipLaunchKernelGGL(wgrad_reduce_packed_kernel, dim3(adh_min_i(adh_ceil_div(total, 256), 4096)), dim3(256), 0,
                       (hipStream_t)stream, slab, nsplit, NcP, Cin, KH, KW, Cout, dst, accumulate);
    return adh_check_launch();
}

// slab[0] = sum over splits, in a fixed order (deterministic).  Block = 64 elements (16 bytes each) x 4 split groups: group y
// adds splits y, y + 4, .. with eight independent loads in flight, the four partial sums meet in LDS.  (One thread per
// element walking all the splits left the 96-channel layers -- 36,864 elements, 144 blocks -- latency-bound: 42 us.)
__global__ __launch_bounds__(256) void wgrad_sum_splits_kernel(float* __restrict__ slab, int nsplit, int64_t n4) {
    __shared__ f32x4 part[3][64];
    f32x4* s4 = reinterpret_cast<f32x4*>(slab);
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    for (int64_t i0 = blockIdx.x * (int64_t)64; i0 < n4; i0 += (int64_t)gridDim.x * 64) {
        const int64_t i = i0 + x;
        f32x4 a[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (i < n4) {
            int sp = y;
            for (; sp + 28 < nsplit; sp += 32) {
#pragma unroll
                for (int u = 0; u < 8; ++u) a[u] += s4[(int64_t)(sp + 4 * u) * n4 + i];
            }
            for (; sp < nsplit; sp += 4) a[0] += s4[(int64_t)sp * n4 + i];
        }
        const f32x4 t = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
        if (y) part[y - 1][x] = t;
        __syncthreads();
        if (y == 0 && i < n4) s4[i] = ((t + part[0][x]) + (part[1][x] + part[2][x]));
        __syncthreads();
    }
}

void adh_wgrad_sum_splits(hipStream_t s, float* slab, int nsplit, int64_t n4) {
    hipLaunchKernelGGL(wgrad_sum_splits_kernel, dim3(adh_min_i(adh_ceil_div(n4, 64), 4096)), dim3(256), 0, s, slab, nsplit, n4);
}

// ---- Winograd-domain slabs ------------------------------------------------------------------------------------------------
// A domain gives PLANES frequency planes per class, the TH x TW output taps inverse(u, w) makes of them, the number of classes
// and the layout tap (ty, tx) of output tap (i, j) of class c.

// F(2x2,3x3), conv_wgrad_rows_kernel in Winograd mode: G^T u G with G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]; the two minus
// signs of A's last row / column were left out by the accumulating kernel (u[a][b] *= s_a s_b, s_3 = -1)
struct WinoF23 {
    static constexpr int PLANES = 16, TH = 3, TW = 3;
    __host__ __device__ int classes() const { return 1; }
    __host__ __device__ void tap(const adh_wlayout&, int, int i, int j, int& ty, int& tx) const { ty = i, tx = j; }
    __host__ __device__ static void inverse(const float (&s)[16], float (&w)[3][3]) {
        float u[4][4];
#pragma unroll
        for (int f = 0; f < 16; ++f) {
            const float sign = ((f >> 2) == 3) != ((f & 3) == 3) ? -1.f : 1.f;
            u[f >> 2][f & 3] = sign * s[f];
        }
        float t[3][4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            t[0][b] = u[0][b] + 0.5f * (u[1][b] + u[2][b]);
            t[1][b] = 0.5f * (u[1][b] - u[2][b]);
            t[2][b] = 0.5f * (u[1][b] + u[2][b]) + u[3][b];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            w[i][0] = t[i][0] + 0.5f * (t[i][1] + t[i][2]);
            w[i][1] = 0.5f * (t[i][1] - t[i][2]);
            w[i][2] = 0.5f * (t[i][1] + t[i][2]) + t[i][3];
        }
    }
};

// F(3x3,2x2) per kernel-parity class, conv_wgrad32_kernel / conv_wgrad32v2*_kernel: A^T u A with A = [[1,0],[1,1],[1,-1],[0,-1]];
// rows / columns 1, 2 of the slab carry the deferred factor 1/2 of G.  The class's 2x2 taps go to d's taps through `tp`.
struct WinoF32 {
    static constexpr int PLANES = 16, TH = 2, TW = 2;
    adh_wg32_taps tp;
    __host__ __device__ int classes() const { return tp.ncls; }
    __host__ __device__ void tap(const adh_wlayout& L, int c, int hy, int hx, int& ty, int& tx) const {
        const int t = tp.tap0[c] + (tp.rev[c] ? 1 - hy : hy) * tp.tap_sy[c] + (tp.rev[c] ? 1 - hx : hx) * tp.tap_sx[c];
        ty = t / L.KWt, tx = t - ty * L.KWt;
    }
    __host__ __device__ static void inverse(const float (&s)[16], float (&w)[2][2]) {
        float u[4][4];
#pragma unroll
        for (int f = 0; f < 16; ++f) {
            const int a = f >> 2, b = f & 3;
            const float sc = ((a == 1 || a == 2) ? 0.5f : 1.f) * ((b == 1 || b == 2) ? 0.5f : 1.f);
            u[a][b] = sc * s[f];
        }
        float t[2][4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            t[0][b] = u[0][b] + u[1][b] + u[2][b];
            t[1][b] = u[1][b] - u[2][b] - u[3][b];
        }
#pragma unroll
        for (int hy = 0; hy < 2; ++hy) {
            w[hy][0] = t[hy][0] + t[hy][1] + t[hy][2];
            w[hy][1] = t[hy][1] - t[hy][2] - t[hy][3];
        }
    }
};

// F(4x4,3x3), conv_wgrad_wino43_kernel: A'^T (u[a][b] / (N_a N_b)) A' at the points 0, +-a, +-b, infinity, in float64 and rounded
// once (the 1 / N factors are not dyadic)
struct WinoF43 {
    static constexpr int PLANES = 36, TH = 3, TW = 3;
    __host__ __device__ int classes() const { return 1; }
    __host__ __device__ void tap(const adh_wlayout&, int, int i, int j, int& ty, int& tx) const { ty = i, tx = j; }
    __host__ __device__ static void inverse(const float (&u)[36], float (&w)[3][3]) {
        const double a = G4_A, b = G4_B;
        const double n0 = a * a * b * b, na = 2.0 * a * a * (a * a - b * b), nb = 2.0 * b * b * (b * b - a * a);
        const double inv[6] = {1.0 / n0, 1.0 / na, 1.0 / na, 1.0 / nb, 1.0 / nb, 1.0};
        const double AT[3][6] = {{1, 1, 1, 1, 1, 0}, {0, a, -a, b, -b, 0}, {0, a * a, a * a, b * b, b * b, 1}};
        double t[3][6];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int bb = 0; bb < 6; ++bb) {
                double acc = 0.0;
#pragma unroll
                for (int aa = 0; aa < 6; ++aa) acc += AT[i][aa] * inv[aa] * (double)u[aa * 6 + bb];
                t[i][bb] = acc * inv[bb];
            }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                double v = 0.0;
#pragma unroll
                for (int bb = 0; bb < 6; ++bb) v += t[i][bb] * AT[j][bb];
                w[i][j] = (float)v;
            }
    }
};

// dst(layout L) (+)= inverse transform of slab[0][class][plane][KP][NcP] (split 0 holds the sum over splits), one thread per
// (class, k, n): PLANES independent loads in flight
template <class Dom>
__global__ void wgrad_reduce_winograd_kernel(const float* __restrict__ slab, int KP, int NcP, const adh_wlayout L, const Dom dom,
                                             float* __restrict__ dst, int accumulate) {
    const int64_t total = (int64_t)dom.classes() * L.K * L.Nc;
    const int64_t fstride = (int64_t)KP * NcP;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const WrElem e = wr_elem(idx, L);
        const float* p = slab + e.t * Dom::PLANES * fstride + (int64_t)e.k * NcP + e.n;
        float u[Dom::PLANES], w[Dom::TH][Dom::TW];
#pragma unroll
        for (int f = 0; f < Dom::PLANES; ++f) u[f] = p[f * fstride];
        Dom::inverse(u, w);
#pragma unroll
        for (int i = 0; i < Dom::TH; ++i)
#pragma unroll
            for (int j = 0; j < Dom::TW; ++j) {
                int ty, tx;
                dom.tap(L, e.t, i, j, ty, tx);
                wr_store(dst, L, ty, tx, e.k, e.n, w[i][j], accumulate);
            }
    }
}

// many splits x few (k, n) pairs would leave the transform kernel latency-bound: the splits are stream-summed first
template <class Dom>
static int wgrad_reduce_winograd(void* stream, float* slab, int nsplit, int KP, int NcP, const adh_wlayout* L, const Dom& dom,
                                 float* dst, int accumulate) {
    hipStream_t s = (hipStream_t)stream;
    if (nsplit > 1) adh_wgrad_sum_splits(s, slab, nsplit, (int64_t)dom.classes() * Dom::PLANES * KP * NcP / 4);
    const int64_t total = (int64_t)dom.classes() * L->K * L->Nc;
    hipLaunchKernelGGL(wgrad_reduce_winograd_kernel<Dom>, dim3(adh_min_i(adh_ceil_div(total, 64), 16384)), dim3(64), 0, s, slab,
                       KP, NcP, *L, dom, dst, accumulate);
    return adh_check_launch();
}

extern "C" int adh_wgrad_reduce_wino(void* stream, float* slab, int nsplit, int KP, int NcP, const adh_wlayout* L,
                                     float* dst, int accumulate) {
    if (!slab || !L || !dst || nsplit < 1 || L->KHt != 3 || L->KWt != 3 || (NcP & 3)) return ADH_E_ARG;
    return wgrad_reduce_winograd(stream, slab, nsplit, KP, NcP, L, WinoF23{}, dst, accumulate);
}

extern "C" int adh_wgrad_reduce_wino43(void* stream, float* slab, int nsplit, int KP, int NcP, const adh_wlayout* L,
                                       float* dst, int accumulate) {
    if (!slab || !L || !dst || nsplit < 1 || L->KHt != 3 || L->KWt != 3 || (NcP & 3)) return ADH_E_ARG;
    return wgrad_reduce_winograd(stream, slab, nsplit, KP, NcP, L, WinoF43{}, dst, accumulate);
}

extern "C" int adh_wgrad_reduce_wino32(void* stream, float* slab, int nsplit, const adh_conv_desc* d, int KP, int NcP,
                                       const adh_wlayout* L, float* dst, int accumulate) {
    if (!slab || !L || !dst || !d || nsplit < 1 || (NcP & 3)) return ADH_E_ARG;
    WinoF32 dom;
    if (!adh_wgrad32_class_taps(d, &dom.tp)) return ADH_E_UNSUPPORTED;
    if (L->KHt * L->KWt != d->KH * d->KW) return ADH_E_ARG;
    return wgrad_reduce_winograd(stream, slab, nsplit, KP, NcP, L, dom, dst, accumulate);
}
