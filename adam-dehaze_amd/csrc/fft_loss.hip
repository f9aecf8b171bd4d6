// Frequency-domain L1 loss term, gfx950: for d = pred - target [N,3,H,W] and D = fft2(d) over the last two dims,
//   L = sum over (n, c, u, v) of (|Re D| + |Im D|) / (2 N 3 H W)        (divided by sqrt(H W) once more for norm = "ortho")
//   dL/dpred = Re(F^H s) / (2 N 3 H W),  s = sign(Re D) + i sign(Im D), sign(0) = 0
// H and W powers of two in [8, 4096].  No FFT library: the transforms are written here.
//
// One transform, used four times: an in-place radix-2 decimation-in-frequency FFT in LDS (natural order in, bit-reversed order
// out), two stages at a time in registers (a radix-4 unit on elements i, i+q, i+2q, i+3q is the stages with half sizes 2q and q;
// an odd stage count leaves one radix-2 stage), and its stage-by-stage Hermitian transpose, the decimation-in-time FFT with
// conjugate twiddles (bit-reversed in, natural out).  |.| and sign(.) act per bin, so nothing is ever put back in order: the
// spectrum lives in bit-reversed order from the first pass to the last, and the adjoint undoes the scrambling by construction.
// Twiddles come from sincospif on j / h, which is exact in fp32 (h a power of two): correct to fp32 rounding at every size.
//
// d is real, so D and s are Hermitian and half the columns suffice in both directions.  The workspace holds, per image-channel
// and row, W/2 complex "slots": slot k >= 1 is column v = bitrev(k) in (0, W/2); slot 0 packs the two real columns v = 0 (.x) and
// v = W/2 (.y).  That is H * W/2 complex = the bytes of one image, with no ragged last column.
//   fft_rows_fwd   one workgroup per (image-channel, pair of rows): z = d[y0] + i d[y1], one complex transform, split into the two
//                  rows' half spectra by Z[v] +- conj Z[W-v], written to the workspace.
//   fft_cols       one workgroup per (image-channel, tile of TC adjacent slots; TC * 8 bytes per row and global access): column
//                  transform in LDS; float64 sum of |Re| + |Im| (weight 2 for slots >= 1, which stand for v and W - v; slot 0 is
//                  first split into its two Hermitian columns, weight 1 each) into one partial per workgroup; with GRAD, D is
//                  overwritten by s, the adjoint column transform runs on the same LDS image and the tile goes back in place.
//                  The four self-conjugate bins come out with an imaginary part of exactly 0 (x - x), so their sign is 0.
//   fft_rows_adj   one workgroup per (image-channel, pair of rows): rebuilds the full Hermitian rows of the pair as one complex
//                  spectrum, adjoint transform, scaled real parts -> grad row y0, imaginary parts -> grad row y1.
//   fft_finalize   one workgroup: the partials summed in a fixed order in float64, scaled, rounded once to the fp32 loss.
// No atomics, fixed summation order: bit-reproducible.  LDS image index a is stored at a ^ (((a >> 5) & 3) << log2 TC): see
// fft_lidx.
#include "common.h"

struct __attribute__((aligned(8))) fftc {
    float x, y;
};

#define FFT_MIN 8
#define FFT_MAX 4096
#define FFT_THREADS_MAX 256

// Power-of-two strides put every lane of a wave on the same few of the 64 LDS banks.  A radix-4 unit of the column pass touches
// rows i + k q, element (row, c) at row * TC + c: for q = 1, 2 the 32 lanes of one 8-byte access would cover only bits 0..log2 TC-1
// and >= 5 of the index.  XOR-ing index bits 5, 6 into bits log2 TC, log2 TC + 1 makes those accesses conflict-free at TC = 8 at
// no cost in space (padding would not fit H = 4096); the row passes (TC = 1) use the same map, which frees the q = 1 unit and
// leaves two- to four-way conflicts at q = 2..8.
__device__ __forceinline__ int fft_lidx(int a, int sh) { return a ^ (((a >> 5) & 3) << sh); }

__device__ __forceinline__ fftc fft_mul(fftc a, float wr, float wi) { return fftc{a.x * wr - a.y * wi, a.x * wi + a.y * wr}; }
__device__ __forceinline__ fftc fft_add(fftc a, fftc b) { return fftc{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ fftc fft_sub(fftc a, fftc b) { return fftc{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ float fft_sign(float v) { return (float)(v > 0.f) - (float)(v < 0.f); }
__device__ __forceinline__ int fft_brev(int v, int bits) { return (int)(__brev((unsigned)v) >> (32 - bits)); }

// The transform of `1 << csh` interleaved sequences of n = 1 << logn elements: element (pos, c) at fft_lidx((pos << csh) + c, csh).
// INV = false: decimation in frequency, e^{-2 pi i jk/n}, natural -> bit-reversed.  INV = true: its Hermitian transpose.
// Ends with a barrier; the caller places one before it.
template <bool INV>
__device__ __forceinline__ void fft_lds(fftc* s, int logn, int csh, int tid, int nthr) {
    const int n = 1 << logn, cmask = (1 << csh) - 1;
    const int qmin_log = logn & 1;                       // smallest q of a radix-4 unit: 1, or 2 when a radix-2 stage is left over
    const int npairs = logn >> 1;
    if (INV && (logn & 1)) {                             // the left-over stage (h = 1, twiddle 1) comes first on the way back
        for (int w = tid; w < (n >> 1) << csh; w += nthr) {
            const int c = w & cmask, i = (w >> csh) << 1;
            const int a0 = fft_lidx((i << csh) + c, csh), a1 = fft_lidx(((i + 1) << csh) + c, csh);
            const fftc x0 = s[a0], x1 = s[a1];
            s[a0] = fft_add(x0, x1);
            s[a1] = fft_sub(x0, x1);
        }
        __syncthreads();
    }
    for (int p = 0; p < npairs; ++p) {
        const int logq = INV ? qmin_log + 2 * p : logn - 2 - 2 * p;
        const int q = 1 << logq;
        for (int w = tid; w < (n >> 2) << csh; w += nthr) {
            const int c = w & cmask, b = w >> csh;
            const int j = b & (q - 1), i = ((b >> logq) << (logq + 2)) + j;
            const int a0 = fft_lidx((i << csh) + c, csh), a1 = fft_lidx(((i + q) << csh) + c, csh);
            const int a2 = fft_lidx(((i + 2 * q) << csh) + c, csh), a3 = fft_lidx(((i + 3 * q) << csh) + c, csh);
            // wa = e^{-i pi j / 2q} (half size 2q, index j; index j + q is wa * -i), wb = e^{-i pi j / q} (half size q)
            float sa, ca, sb, cb;
            sincospif((float)j / (float)(2 * q), &sa, &ca);
            sincospif((float)j / (float)q, &sb, &cb);
            const fftc x0 = s[a0], x1 = s[a1], x2 = s[a2], x3 = s[a3];
            if (!INV) {
                const fftc t0 = fft_add(x0, x2), t2 = fft_mul(fft_sub(x0, x2), ca, -sa);
                const fftc t1 = fft_add(x1, x3), t3 = fft_mul(fft_sub(x1, x3), -sa, -ca);
                s[a0] = fft_add(t0, t1);
                s[a1] = fft_mul(fft_sub(t0, t1), cb, -sb);
                s[a2] = fft_add(t2, t3);
                s[a3] = fft_mul(fft_sub(t2, t3), cb, -sb);
            } else {
                const fftc b1 = fft_mul(x1, cb, sb), b3 = fft_mul(x3, cb, sb);
                const fftc t0 = fft_add(x0, b1), t1 = fft_sub(x0, b1), t2 = fft_add(x2, b3), t3 = fft_sub(x2, b3);
                const fftc c2 = fft_mul(t2, ca, sa), c3 = fft_mul(t3, -sa, ca);
                s[a0] = fft_add(t0, c2);
                s[a2] = fft_sub(t0, c2);
                s[a1] = fft_add(t1, c3);
                s[a3] = fft_sub(t1, c3);
            }
        }
        __syncthreads();
    }
    if (!INV && (logn & 1)) {
        for (int w = tid; w < (n >> 1) << csh; w += nthr) {
            const int c = w & cmask, i = (w >> csh) << 1;
            const int a0 = fft_lidx((i << csh) + c, csh), a1 = fft_lidx(((i + 1) << csh) + c, csh);
            const fftc x0 = s[a0], x1 = s[a1];
            s[a0] = fft_add(x0, x1);
            s[a1] = fft_sub(x0, x1);
        }
        __syncthreads();
    }
}

// LDS position of the bin W - v that mirrors slot k >= 1 (v = bitrev(k) over logW - 1 bits, itself at position 2k)
__device__ __forceinline__ int fft_mirror_pos(int k, int logW) {
    const int v = fft_brev(k, logW - 1);
    return fft_brev((1 << logW) - v, logW);
}

__global__ __launch_bounds__(FFT_THREADS_MAX) void fft_rows_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                       int H, int logW, fftc* __restrict__ ws) {
    ADH_DYN_LDS(fftc, s);                                // W complex
    const int W = 1 << logW, Wh = W >> 1, tid = threadIdx.x, nthr = blockDim.x;
    const int64_t row0 = ((int64_t)blockIdx.y * H + 2 * (int64_t)blockIdx.x);
    const float* p0 = pred + row0 * W;
    const float* t0 = target + row0 * W;
    for (int x = tid; x < W; x += nthr) s[fft_lidx(x, 0)] = fftc{p0[x] - t0[x], p0[W + x] - t0[W + x]};
    __syncthreads();
    fft_lds<false>(s, logW, 0, tid, nthr);
    fftc* o0 = ws + row0 * Wh;
    fftc* o1 = o0 + Wh;
    for (int k = tid; k < Wh; k += nthr) {
        if (k == 0) {                                    // v = 0 at position 0, v = W/2 at position 1: both real per row
            const fftc z0 = s[fft_lidx(0, 0)], zh = s[fft_lidx(1, 0)];
            o0[0] = fftc{z0.x, zh.x};
            o1[0] = fftc{z0.y, zh.y};
        } else {
            const fftc z1 = s[fft_lidx(2 * k, 0)], z2 = s[fft_lidx(fft_mirror_pos(k, logW), 0)];
            o0[k] = fftc{0.5f * (z1.x + z2.x), 0.5f * (z1.y - z2.y)};      // (Z[v] + conj Z[W-v]) / 2
            o1[k] = fftc{0.5f * (z1.y + z2.y), 0.5f * (z2.x - z1.x)};      // (Z[v] - conj Z[W-v]) / 2i
        }
    }
}

template <bool GRAD>
__global__ __launch_bounds__(FFT_THREADS_MAX) void fft_cols_kernel(fftc* __restrict__ ws, int logH, int Wh, int csh,
                                                                   double* __restrict__ partial) {
    ADH_DYN_LDS(fftc, s);                                // H rows of TC complex
    __shared__ double red[FFT_THREADS_MAX];
    const int H = 1 << logH, TC = 1 << csh, tid = threadIdx.x, nthr = blockDim.x;
    const int k0 = blockIdx.x << csh;
    fftc* g = ws + (int64_t)blockIdx.y * H * Wh + k0;
    for (int a = tid; a < H << csh; a += nthr) s[fft_lidx(a, csh)] = g[(int64_t)(a >> csh) * Wh + (a & (TC - 1))];
    __syncthreads();
    fft_lds<false>(s, logH, csh, tid, nthr);
    double acc = 0.0;
    for (int a = tid; a < H << csh; a += nthr) {
        if (k0 + (a & (TC - 1)) == 0) continue;          // the packed slot 0: below
        const int l = fft_lidx(a, csh);
        const fftc d = s[l];
        acc += 2.0 * ((double)fabsf(d.x) + (double)fabsf(d.y));
        if (GRAD) s[l] = fftc{fft_sign(d.x), fft_sign(d.y)};
    }
    if (k0 == 0) {
        // column 0 holds Z = FFT(R0 + i Rh), R0 / Rh the real columns v = 0 / W/2 after the row pass:
        // D0[u] = (Z[u] + conj Z[H-u]) / 2, Dh[u] = (Z[u] - conj Z[H-u]) / 2i, D[H-u] = conj D[u]; s goes back as s0 + i sh
        for (int u = tid; u <= H >> 1; u += nthr) {
            const int l1 = fft_lidx(fft_brev(u, logH) << csh, csh);
            const fftc z1 = s[l1];
            if (u == 0 || u == H >> 1) {
                acc += (double)fabsf(z1.x) + (double)fabsf(z1.y);
                if (GRAD) s[l1] = fftc{fft_sign(z1.x), fft_sign(z1.y)};
            } else {
                const int l2 = fft_lidx(fft_brev(H - u, logH) << csh, csh);
                const fftc z2 = s[l2];
                const fftc d0 = fftc{0.5f * (z1.x + z2.x), 0.5f * (z1.y - z2.y)};
                const fftc dh = fftc{0.5f * (z1.y + z2.y), 0.5f * (z2.x - z1.x)};
                acc += 2.0 * (((double)fabsf(d0.x) + (double)fabsf(d0.y)) + ((double)fabsf(dh.x) + (double)fabsf(dh.y)));
                if (GRAD) {
                    const float ar = fft_sign(d0.x), ai = fft_sign(d0.y), br = fft_sign(dh.x), bi = fft_sign(dh.y);
                    s[l1] = fftc{ar - bi, ai + br};      // s0[u] + i sh[u]
                    s[l2] = fftc{ar + bi, br - ai};      // conj s0[u] + i conj sh[u]
                }
            }
        }
    }
    red[tid] = acc;
    __syncthreads();
    for (int o = FFT_THREADS_MAX >> 1; o > 0; o >>= 1) {
        if (tid < o && tid + o < nthr) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
    if (GRAD) {
        fft_lds<true>(s, logH, csh, tid, nthr);
        for (int a = tid; a < H << csh; a += nthr) g[(int64_t)(a >> csh) * Wh + (a & (TC - 1))] = s[fft_lidx(a, csh)];
    }
}

__global__ __launch_bounds__(FFT_THREADS_MAX) void fft_rows_adj_kernel(const fftc* __restrict__ ws, int H, int logW, float scale,
                                                                       float* __restrict__ grad) {
    ADH_DYN_LDS(fftc, s);
    const int W = 1 << logW, Wh = W >> 1, tid = threadIdx.x, nthr = blockDim.x;
    const int64_t row0 = ((int64_t)blockIdx.y * H + 2 * (int64_t)blockIdx.x);
    const fftc* i0 = ws + row0 * Wh;
    const fftc* i1 = i0 + Wh;
    for (int k = tid; k < Wh; k += nthr) {
        const fftc a = i0[k], b = i1[k];                 // X[v] = G0[v] + i G1[v], X[W-v] = conj G0[v] + i conj G1[v]
        if (k == 0) {
            s[fft_lidx(0, 0)] = fftc{a.x, b.x};
            s[fft_lidx(1, 0)] = fftc{a.y, b.y};
        } else {
            s[fft_lidx(2 * k, 0)] = fftc{a.x - b.y, a.y + b.x};
            s[fft_lidx(fft_mirror_pos(k, logW), 0)] = fftc{a.x + b.y, b.x - a.y};
        }
    }
    __syncthreads();
    fft_lds<true>(s, logW, 0, tid, nthr);
    float* o0 = grad + row0 * W;
    for (int x = tid; x < W; x += nthr) {
        const fftc v = s[fft_lidx(x, 0)];
        o0[x] = v.x * scale;
        o0[W + x] = v.y * scale;
    }
}

__global__ __launch_bounds__(FFT_THREADS_MAX) void fft_finalize_kernel(const double* __restrict__ partial, int n, double scale,
                                                                       float* __restrict__ loss) {
    __shared__ double red[FFT_THREADS_MAX];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < n; i += FFT_THREADS_MAX) acc += partial[i];
    red[tid] = acc;
    __syncthreads();
    for (int o = FFT_THREADS_MAX >> 1; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) *loss = (float)(red[0] * scale);
}

static int fft_log2(int v) {
    if (v < FFT_MIN || v > FFT_MAX || (v & (v - 1))) return -1;
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}
// slots per column tile: 8 (64-byte runs), 4 where 8 columns of H = 4096 would not fit the LDS or the image has only 4 slots
static int fft_col_shift(int H, int W) { return (H > 2048 || W < 16) ? 2 : 3; }
static int fft_threads(int64_t units) { return units >= FFT_THREADS_MAX ? FFT_THREADS_MAX : (units <= 64 ? 64 : (int)units); }
static bool fft_sizes_ok(int N, int H, int W) {
    return N >= 1 && fft_log2(H) >= 0 && fft_log2(W) >= 0 && 3 * (int64_t)N <= 65535 &&
           3 * (int64_t)N * H * W * (int64_t)sizeof(float) <= 0x7fffffff;
}

extern "C" int adh_fft_l1_workspace_bytes(int N, int H, int W) {
    if (N < 1) return ADH_E_ARG;
    if (!fft_sizes_ok(N, H, W)) return ADH_E_UNSUPPORTED;
    return (int)(3 * (int64_t)N * H * (W / 2) * (int64_t)sizeof(fftc));
}

extern "C" int adh_fft_l1_num_partials(int N, int H, int W) {
    if (N < 1) return ADH_E_ARG;
    if (!fft_sizes_ok(N, H, W)) return ADH_E_UNSUPPORTED;
    return 3 * N * ((W / 2) >> fft_col_shift(H, W));
}

extern "C" int adh_fft_l1(void* stream, const float* pred_nchw, const float* target_nchw, int N, int H, int W, int ortho,
                          void* workspace, double* partial, float* loss, float* g_pred_nchw) {
    if (!pred_nchw || !target_nchw || !workspace || !partial || !loss || N < 1 || (ortho != 0 && ortho != 1)) return ADH_E_ARG;
    if (((uintptr_t)workspace & 7) || ((uintptr_t)partial & 7)) return ADH_E_ARG;
    if (!fft_sizes_ok(N, H, W)) return ADH_E_UNSUPPORTED;
    const int logH = fft_log2(H), logW = fft_log2(W), Wh = W / 2, csh = fft_col_shift(H, W);
    const int ntiles = Wh >> csh, nparts = 3 * N * ntiles;
    hipStream_t st = (hipStream_t)stream;
    fftc* ws = (fftc*)workspace;
    const dim3 grows(H / 2, 3 * N), gcols(ntiles, 3 * N);
    const int trows = fft_threads(W / 4), tcols = fft_threads(((int64_t)H / 4) << csh);
    const size_t lrows = (size_t)W * sizeof(fftc), lcols = ((size_t)H << csh) * sizeof(fftc);
    const double count = 2.0 * 3.0 * (double)N * (double)H * (double)W;
    const double scale = (ortho ? 1.0 / sqrt((double)H * (double)W) : 1.0) / count;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fft_cols_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lcols);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fft_cols_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lcols);
    hipLaunchKernelGGL(fft_rows_fwd_kernel, grows, dim3(trows), lrows, st, pred_nchw, target_nchw, H, logW, ws);
    if (g_pred_nchw) {
        hipLaunchKernelGGL(fft_cols_kernel<true>, gcols, dim3(tcols), lcols, st, ws, logH, Wh, csh, partial);
        hipLaunchKernelGGL(fft_rows_adj_kernel, grows, dim3(trows), lrows, st, (const fftc*)ws, H, logW, (float)scale, g_pred_nchw);
    } else {
        hipLaunchKernelGGL(fft_cols_kernel<false>, gcols, dim3(tcols), lcols, st, ws, logH, Wh, csh, partial);
    }
    hipLaunchKernelGGL(fft_finalize_kernel, dim3(1), dim3(FFT_THREADS_MAX), 0, st, (const double*)partial, nparts, scale, loss);
    return adh_check_launch();
}
