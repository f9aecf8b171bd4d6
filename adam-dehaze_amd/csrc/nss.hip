// Natural-scene statistics for the no-reference scores NIQE (Mittal, Soundararajan, Bovik 2013) and BRISQUE (Mittal, Moorthy,
// Bovik 2012), gfx950: the mean-subtracted contrast-normalised (MSCN) coefficients of a grey plane, the products
// of torus neighbours inside a region, and the handful of sums per region both scores fit their features to.
//   grey plane   Y = 255 ((0.299 R + 0.587 G) + 0.114 B), float64 from the fp32 planes, over the top-left Hc x Wc crop
//   window       g[i] = exp(-(i-3)^2 / (2 (7/6)^2)), i = 0..6, normalised to sum 1 in float64; w = g (x) g; window positions
//                outside the cropped plane take the nearest in-plane pixel
//   per pixel p  d = sum_q w_q (Y_q - Y_p),  v = sum_q w_q (Y_q - Y_p)^2 - d^2,  s = sqrt|v|,  M_p = -d / (s + 1)
//                (centred on the pixel: an exactly flat window gives exact zeros whatever the order of the sum)
//   region       an rh x rw block of the crop; M comes from the plane, so windows cross region borders, while the neighbour
//                products wrap inside the region: direction k pairs (i, j) with ((i + di) mod rh, (j + dj) mod rw),
//                (di, dj) = (0,1), (1,0), (1,1), (1,-1)
//   per region   24 doubles: [0] sum|M|, [1] sum M^2, [2] sum s; for direction k at 3 + 5k: the count of products < 0, the sum
//                of their squares, the count of products > 0, the sum of their squares, sum|p| over all; [23] = 0.  A product
//                equal to 0 (or NaN) is in neither set.
//   second scale the grey plane halved by the antialiased bicubic (a = -0.5): output j reads inputs 2j-3 .. 2j+4, indices clamped
//                to the plane, weights [-3, -9, 29, 111, 111, 29, -9, -3] / 256, along W first, then along H.
// Nothing is contracted by the compiler (the pragma below): the grey value of a pixel is the same double wherever it is formed
// -- staged in LDS or read again for a wrapped neighbour -- and Y_q - Y_p of two equal pixels is exactly 0.  The sums use
// explicit fma.
//
// Moments: a workgroup owns an NSS_TH x NSS_TW tile of one region.  It needs M on the tile, on the row below and on the columns
// left and right (the four directions look right, down, down-right and down-left), so it stages those (NSS_TH + 1) x (NSS_TW + 2)
// positions plus the window's ring of 3 as float64 in LDS, clamped to the crop.  A position that leaves the region stands for
// the wrapped pixel on the region's other side, whose window lies elsewhere in the plane: its 49 taps are read from memory
// directly (the perimeter of a region only).  LDS is float64 and consecutive lanes read consecutive columns of a row, so by
// the ds_read_b64 bank rule (32 lanes x 2 words = 64 banks) no pass has a conflict beyond the turn of a row.
// No atomics: a tile reduces its 23 sums over a fixed tree to one partial, and a second launch adds a region's partials in a
// fixed order (a region of more than NSS_LAST tiles -- a whole photograph as one BRISQUE region -- first adds them NSS_CHUNK at a
// time, in place, so that no workgroup walks thousands of partials alone), so two runs are bit-equal and the numbers of image
// i do not depend on N.
#include "common.h"
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define NSS_WIN 7
#define NSS_R 3
#define NSS_THREADS 256
#define NSS_GROUPS (NSS_THREADS / 32)
#define NSS_TH 16                             // tile sides: adh_nss_moments' ntiles counts tiles of these (the header names them)
#define NSS_TW 32
#define NSS_MH (NSS_TH + 1)                   // M: the tile and the row below
#define NSS_MW (NSS_TW + 2)                   // the column left of it, the tile, the column right of it
#define NSS_YH (NSS_MH + 2 * NSS_R)           // 23 staged rows
#define NSS_YW (NSS_MW + 2 * NSS_R)           // 40 staged columns
#define NSS_OUT 24
#define NSS_SLICES 10                         // the finalize kernel adds a region's partials in 10 interleaved slices
#ifndef NSS_LAST
#define NSS_LAST 160                          // the last level adds up to this many partials per region; more go through levels
#endif                                        // of NSS_CHUNK first (the host-emulation test sets both small, so the levels run)
#ifndef NSS_CHUNK
#define NSS_CHUNK 64
#endif
#ifndef NSS_MAX_GRID
#define NSS_MAX_GRID 65535                    // regions (and blocks of the halving) beyond it are looped over
#endif

struct nss_window {
    double w[NSS_WIN * NSS_WIN];
};

static nss_window nss_make_window() {
    double g[NSS_WIN], s = 0.0;
    const double sigma = 7.0 / 6.0;
    for (int i = 0; i < NSS_WIN; ++i) {
        const double d = (double)(i - NSS_R);
        g[i] = exp(-(d * d) / (2.0 * sigma * sigma));
        s += g[i];
    }
    for (int i = 0; i < NSS_WIN; ++i) g[i] /= s;
    nss_window win;
    for (int a = 0; a < NSS_WIN; ++a)
        for (int b = 0; b < NSS_WIN; ++b) win.w[a * NSS_WIN + b] = g[a] * g[b];
    return win;
}

struct nss_halve_taps {
    double t[8];
};

// pixel o of image `img`: the grey value of three fp32 planes HW apart, or the double itself
template <bool RGB>
__device__ __forceinline__ double nss_pixel(const void* __restrict__ img, int64_t HW, int64_t o) {
    if (RGB) {
        const float* __restrict__ p = (const float*)img;
        const double r = (double)p[o], g = (double)p[HW + o], b = (double)p[2 * HW + o];
        return 255.0 * ((0.299 * r + 0.587 * g) + 0.114 * b);
    }
    return ((const double*)img)[o];
}

__device__ __forceinline__ int nss_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// grid (tiles of a region, min(N * regions, NSS_MAX_GRID)); partial: [N * regions][tiles][24]
template <bool RGB>
__global__ __launch_bounds__(NSS_THREADS) void nss_moments_kernel(const void* __restrict__ src, int H, int W, int Hc, int Wc,
                                                                  int rh, int rw, int tiles_x, int regions_y, int regions_x,
                                                                  int64_t nregions, nss_window win, double* __restrict__ partial) {
    __shared__ double Ys[NSS_YH][NSS_YW];
    __shared__ double Ms[NSS_MH][NSS_MW];
    __shared__ double red[8][NSS_THREADS];
    const int tid = threadIdx.x, lane = tid & 31, grp = tid >> 5;
    const int tile = blockIdx.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * NSS_TH, x0 = tx * NSS_TW;       // first pixel of the tile, in region coordinates
    const int64_t HW = (int64_t)H * W;
    const int64_t per_image = (int64_t)regions_y * regions_x;
    for (int64_t rg = blockIdx.y; rg < nregions; rg += gridDim.y) {
        const int64_t n = rg / per_image, rr = rg - n * per_image;
        const int by = (int)(rr / regions_x), bx = (int)(rr - (int64_t)by * regions_x);
        const int R0 = by * rh, C0 = bx * rw;           // first pixel of the region, in plane coordinates
        const void* __restrict__ img = RGB ? (const void*)((const float*)src + n * 3 * HW) : (const void*)((const double*)src + n * HW);
        for (int i = tid; i < NSS_YH * NSS_YW; i += NSS_THREADS) {
            const int a = i / NSS_YW, b = i - a * NSS_YW;
            const int py = nss_clamp(R0 + y0 - NSS_R + a, Hc - 1), px = nss_clamp(C0 + x0 - NSS_R - 1 + b, Wc - 1);
            Ys[a][b] = nss_pixel<RGB>(img, HW, (int64_t)py * W + px);
        }
        __syncthreads();
        double vals[NSS_OUT];
#pragma unroll
        for (int k = 0; k < NSS_OUT; ++k) vals[k] = 0.0;
        for (int i = tid; i < NSS_MH * NSS_MW; i += NSS_THREADS) {
            const int r = i / NSS_MW, c = i - r * NSS_MW;
            const int ri = y0 + r, rj = x0 - 1 + c;     // region coordinates before wrapping: ri >= 0, rj >= -1
            double m = 0.0;
            if (ri <= rh && rj <= rw) {                 // the tile's own pixels and every neighbour one of them pairs with
                const int wi = ri % rh, wj = ((rj % rw) + rw) % rw;
                double d = 0.0, v = 0.0;
                if (wi == ri && wj == rj) {             // inside the region: the staged window
                    const double yp = Ys[r + NSS_R][c + NSS_R];
#pragma unroll
                    for (int a = 0; a < NSS_WIN; ++a)
#pragma unroll
                        for (int b = 0; b < NSS_WIN; ++b) {
                            const double t = Ys[r + a][c + b] - yp, wt = win.w[a * NSS_WIN + b];
                            d = fma(wt, t, d);
                            v = fma(wt * t, t, v);
                        }
                } else {                                // the wrapped pixel, with its own window
                    const int cy = R0 + wi, cx = C0 + wj;
                    const double yp = nss_pixel<RGB>(img, HW, (int64_t)cy * W + cx);
                    for (int a = 0; a < NSS_WIN; ++a) {
                        const int qy = nss_clamp(cy - NSS_R + a, Hc - 1);
#pragma unroll                                          // a row's loads are issued together: 7 round trips, not 49
                        for (int b = 0; b < NSS_WIN; ++b) {
                            const int qx = nss_clamp(cx - NSS_R + b, Wc - 1);
                            const double t = nss_pixel<RGB>(img, HW, (int64_t)qy * W + qx) - yp, wt = win.w[a * NSS_WIN + b];
                            d = fma(wt, t, d);
                            v = fma(wt * t, t, v);
                        }
                    }
                }
                v = v - d * d;
                const double s = sqrt(fabs(v));
                m = -d / (s + 1.0);
                if (r < NSS_TH && c >= 1 && c <= NSS_TW && ri < rh && rj < rw) {
                    vals[0] += fabs(m);
                    vals[1] += m * m;
                    vals[2] += s;
                }
            }
            Ms[r][c] = m;
        }
        __syncthreads();
        for (int r = grp; r < NSS_TH; r += NSS_GROUPS) {
            if (y0 + r < rh && x0 + lane < rw) {
                const double m0 = Ms[r][lane + 1];
                const double nb[4] = {Ms[r][lane + 2], Ms[r + 1][lane + 1], Ms[r + 1][lane + 2], Ms[r + 1][lane]};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double p = m0 * nb[k];
                    if (p < 0.0) {
                        vals[3 + 5 * k] += 1.0;
                        vals[4 + 5 * k] += p * p;
                    } else if (p > 0.0) {
                        vals[5 + 5 * k] += 1.0;
                        vals[6 + 5 * k] += p * p;
                    }
                    vals[7 + 5 * k] += fabs(p);
                }
            }
        }
        double* __restrict__ q = partial + (rg * gridDim.x + tile) * NSS_OUT;
#pragma unroll
        for (int round = 0; round < NSS_OUT / 8; ++round) {
#pragma unroll
            for (int k = 0; k < 8; ++k) red[k][tid] = vals[round * 8 + k];
            __syncthreads();
            for (int s = NSS_THREADS / 2; s > 0; s >>= 1) {
                if (tid < s) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) red[k][tid] += red[k][tid + s];
                }
                __syncthreads();
            }
            if (tid < 8) q[round * 8 + tid] = red[tid][0];
            __syncthreads();                            // the next round, or the next region's stage, writes over what was just read
        }
    }
}

// Adds partials of a region in a fixed order.  The live partials of a level are those of the tiles 0, step, 2 step, ... (`count`
// of them); workgroup (c, region) adds the `chunk` of them that starts at c * chunk -- 10 interleaved slices per value, then the
// slices -- and writes the sum over the first of its own partials, which no other workgroup reads, or, in the last level
// (one chunk), to out with [23] = 0.  grid (chunks, min(N * regions, NSS_MAX_GRID)).
__global__ __launch_bounds__(NSS_THREADS) void nss_finalize_kernel(double* __restrict__ partial, int ntiles, int64_t nregions,
                                                                   int step, int count, int chunk, double* __restrict__ out) {
    __shared__ double red[NSS_SLICES][NSS_OUT];
    const int tid = threadIdx.x, k = tid % NSS_OUT, j = tid / NSS_OUT;
    const int first = blockIdx.x * chunk, last = first + chunk < count ? first + chunk : count;
    for (int64_t rg = blockIdx.y; rg < nregions; rg += gridDim.y) {
        double* __restrict__ q = partial + rg * ntiles * NSS_OUT;
        if (j < NSS_SLICES) {
            double a = 0.0;
            for (int i = first + j; i < last; i += NSS_SLICES) a += q[(int64_t)i * step * NSS_OUT + k];
            red[j][k] = a;
        }
        __syncthreads();                                // every partial of the chunk is read: the first may be written over
        if (tid < NSS_OUT) {
            double a = 0.0;
            for (int s = 0; s < NSS_SLICES; ++s) a += red[s][tid];
            if (out) out[rg * NSS_OUT + tid] = tid == NSS_OUT - 1 ? 0.0 : a;
            else q[(int64_t)first * step * NSS_OUT + tid] = a;
        }
        __syncthreads();
    }
}

// one thread per output pixel, grid-stride over N * OH * OW
template <bool RGB>
__global__ __launch_bounds__(NSS_THREADS) void nss_halve_kernel(const void* __restrict__ src, int H, int W, int Hc, int Wc, int OH,
                                                                int OW, int64_t total, nss_halve_taps taps, double* __restrict__ dst) {
    const int64_t HW = (int64_t)H * W, OHW = (int64_t)OH * OW;
    for (int64_t e = (int64_t)blockIdx.x * NSS_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * NSS_THREADS) {
        const int64_t n = e / OHW, o = e - n * OHW;
        const int oy = (int)(o / OW), ox = (int)(o - (int64_t)oy * OW);
        const void* __restrict__ img = RGB ? (const void*)((const float*)src + n * 3 * HW) : (const void*)((const double*)src + n * HW);
        double acc = 0.0;
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const int qy = nss_clamp(2 * oy - 3 + a, Hc - 1);
            double h = 0.0;
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const int qx = nss_clamp(2 * ox - 3 + b, Wc - 1);
                h = h + taps.t[b] * nss_pixel<RGB>(img, HW, (int64_t)qy * W + qx);
            }
            acc = acc + taps.t[a] * h;
        }
        dst[e] = acc;
    }
}

static bool nss_overlap(uintptr_t a, uintptr_t na, uintptr_t b, uintptr_t nb) { return a < b + nb && b < a + na; }

static bool nss_bad_plane(const void* src, int src_rgb, int N, int H, int W, int Hc, int Wc) {
    return !src || N < 1 || (src_rgb != 0 && src_rgb != 1) || H < 1 || W < 1 || Hc < 1 || Wc < 1 || Hc > H || Wc > W;
}

static uintptr_t nss_src_bytes(int src_rgb, int N, int H, int W) {
    return (uintptr_t)N * (uintptr_t)H * (uintptr_t)W * (src_rgb ? 12 : 8);
}

extern "C" int adh_nss_halve(void* stream, const void* src, int src_rgb, int N, int H, int W, int Hc, int Wc, double* dst) {
    if (nss_bad_plane(src, src_rgb, N, H, W, Hc, Wc) || !dst) return ADH_E_ARG;
    const int OH = (Hc + 1) / 2, OW = (Wc + 1) / 2;
    const int64_t total = (int64_t)N * OH * OW;
    if (nss_overlap((uintptr_t)dst, (uintptr_t)total * 8, (uintptr_t)src, nss_src_bytes(src_rgb, N, H, W))) return ADH_E_ARG;
    static const double t[8] = {-3.0, -9.0, 29.0, 111.0, 111.0, 29.0, -9.0, -3.0};
    nss_halve_taps taps;
    for (int i = 0; i < 8; ++i) taps.t[i] = t[i] / 256.0;
    const int64_t blocks = (total + NSS_THREADS - 1) / NSS_THREADS;
    const dim3 grid((unsigned)(blocks < NSS_MAX_GRID ? blocks : NSS_MAX_GRID));
    if (src_rgb)
        hipLaunchKernelGGL((nss_halve_kernel<true>), grid, dim3(NSS_THREADS), 0, (hipStream_t)stream, src, H, W, Hc, Wc, OH, OW, total,
                           taps, dst);
    else
        hipLaunchKernelGGL((nss_halve_kernel<false>), grid, dim3(NSS_THREADS), 0, (hipStream_t)stream, src, H, W, Hc, Wc, OH, OW,
                           total, taps, dst);
    return adh_check_launch();
}

extern "C" int adh_nss_moments(void* stream, const void* src, int src_rgb, int N, int H, int W, int Hc, int Wc, int rh, int rw,
                               double* partial, int ntiles, double* out) {
    if (nss_bad_plane(src, src_rgb, N, H, W, Hc, Wc) || !partial || !out || rh < 1 || rw < 1) return ADH_E_ARG;
    if (Hc % rh != 0 || Wc % rw != 0) return ADH_E_ARG;
    const int tiles_y = adh_ceil_div(rh, NSS_TH), tiles_x = adh_ceil_div(rw, NSS_TW);
    const int64_t tiles = (int64_t)tiles_y * tiles_x;
    if (tiles > 0x7fffffff) return ADH_E_UNSUPPORTED;
    if (ntiles != (int)tiles) return ADH_E_ARG;
    const int regions_y = Hc / rh, regions_x = Wc / rw;
    const int64_t nregions = (int64_t)N * regions_y * regions_x;
    const uintptr_t src_bytes = nss_src_bytes(src_rgb, N, H, W), out_bytes = (uintptr_t)nregions * NSS_OUT * 8;
    const uintptr_t partial_bytes = out_bytes * (uintptr_t)tiles;
    if (nss_overlap((uintptr_t)out, out_bytes, (uintptr_t)src, src_bytes) ||
        nss_overlap((uintptr_t)partial, partial_bytes, (uintptr_t)src, src_bytes) ||
        nss_overlap((uintptr_t)partial, partial_bytes, (uintptr_t)out, out_bytes))
        return ADH_E_ARG;
    const nss_window win = nss_make_window();
    const unsigned gy = (unsigned)(nregions < NSS_MAX_GRID ? nregions : NSS_MAX_GRID);
    const dim3 grid((unsigned)tiles, gy);
    if (src_rgb)
        hipLaunchKernelGGL((nss_moments_kernel<true>), grid, dim3(NSS_THREADS), 0, (hipStream_t)stream, src, H, W, Hc, Wc, rh, rw,
                           tiles_x, regions_y, regions_x, nregions, win, partial);
    else
        hipLaunchKernelGGL((nss_moments_kernel<false>), grid, dim3(NSS_THREADS), 0, (hipStream_t)stream, src, H, W, Hc, Wc, rh, rw,
                           tiles_x, regions_y, regions_x, nregions, win, partial);
    // levels of NSS_CHUNK partials each, in place, while a region has more than NSS_LAST of them; then one workgroup per region
    int step = 1, count = (int)tiles;
    while (count > NSS_LAST) {
        const int chunks = adh_ceil_div(count, NSS_CHUNK);
        hipLaunchKernelGGL(nss_finalize_kernel, dim3((unsigned)chunks, gy), dim3(NSS_THREADS), 0, (hipStream_t)stream, partial,
                           (int)tiles, nregions, step, count, NSS_CHUNK, (double*)nullptr);
        step *= NSS_CHUNK;
        count = chunks;
    }
    hipLaunchKernelGGL(nss_finalize_kernel, dim3(1, gy), dim3(NSS_THREADS), 0, (hipStream_t)stream, partial, (int)tiles, nregions,
                       step, count, count, out);
    return adh_check_launch();
}
