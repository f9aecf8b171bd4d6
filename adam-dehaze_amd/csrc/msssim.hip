// Gaussian-window SSIM of Wang et al. (2004) per colour plane, and the pieces MS-SSIM (Wang, Simoncelli, Bovik 2003) is put
// together from, gfx950: one pyramid level forward, one pyramid level backward.
//   g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)), i = 0..10, normalised to sum 1 in float64; the window is g (x) g, "valid" filtering, so an
//   H x W plane has OH x OW = (H - 10) x (W - 10) window positions.  Per plane (n, c), x = pred, y = target:
//     mx = G*x, my = G*y, mxx = G*(x x), myy = G*(y y), mxy = G*(x y);  C1 = (0.01 R)^2, C2 = (0.03 R)^2
//     D1 = mx^2 + my^2 + C1, D2 = (mxx - mx^2) + (myy - my^2) + C2
//     l = (2 mx my + C1) / D1,  cs = (2 (mxy - mx my) + C2) / D2;   SSIM[n,c] = mean(l cs),  CS[n,c] = mean(cs)
//   backward of  a[n,c] SSIM[n,c] + b[n,c] CS[n,c]  with respect to x, per window
//     dl = (2 my - 2 mx l) / D1, dcs = (-2 my + 2 mx cs) / D2, A = a (cs dl + l dcs) + b dcs, w = a l + b, B = -w cs / D2, Cc = 2 w / D2
//     g_x[p] = ((G^T*A)[p] + 2 x[p] (G^T*B)[p] + y[p] (G^T*Cc)[p]) / (OH OW)  (+ a quarter of the coarser level's gradient at the
//     pixel's 2x2 block: the adjoint of the pool below)
//   the next level of the pyramid is the 2x2 mean with stride 2 (the last row / column of an odd side is dropped); the forward
//   writes it from the pixels it has staged.
// Level 0 reads fp32 planes; the pooled levels are float64 planes (the mean of four fp32 values is exact in float64, so the
// statistics of every level see the values the definition names, not a second fp32 rounding), and so are the gradients of the
// pooled levels.  Everything behind the loads is float64: D2 cancels against C2 = 9e-4 and the gradient terms cancel near
// pred = target.  Both filters are separable and run rows first, then columns, through LDS.
//
// LDS layout: every array is float64 and every compute pass maps the 32 lanes of a half wave to 32 (or fewer) consecutive
// columns of ONE row.  ds_read_b64 serves a wave as two groups of 32 lanes over 64 banks of 4 bytes: 32 consecutive doubles are
// 64 consecutive words, one per bank, whatever the row pitch, so neither the row pass (columns c + k of a halo row) nor the
// column pass (column c of rows r + k) has a bank conflict and no row needs padding.  Only the pooled output reads every second
// double (two-way): four reads per pooled pixel.
// No atomics; the per-plane means are a fixed-order two-stage float64 reduction (one partial pair per tile, then one workgroup
// per plane), so they are bit-reproducible and those of image i do not depend on N.  Nothing is saved for the backward.
#include "common.h"

#define MSS_WIN 11
#define MSS_R (MSS_WIN - 1)
#define MSS_THREADS 256
#define MSS_GROUPS (MSS_THREADS / 32)         // half waves: each takes whole rows
#ifndef MSS_MAX_GRID_Y
#define MSS_MAX_GRID_Y 65535                  // planes beyond it are looped over (the host-emulation test sets it to 2)
#endif
// forward: a workgroup owns MSF_TH x MSF_TW window positions
#define MSF_TW 32
#define MSF_TH 16
#define MSF_HW (MSF_TW + MSS_R)               // 42 staged pixels per row
#define MSF_HH (MSF_TH + MSS_R)               // 26 staged rows
// backward: a workgroup owns MSB_TH x MSB_TW pixels; they lie in (MSB_TH + 10) x (MSB_TW + 10) windows, which read
// (MSB_TH + 20) x (MSB_TW + 20) pixels.  MSB_TW + 10 = 32: the two wide passes fill their half waves.
#define MSB_TW 22
#define MSB_TH 12
#define MSB_NW (MSB_TW + MSS_R)               // 32 window columns
#define MSB_NH (MSB_TH + MSS_R)               // 22 window rows
#define MSB_HW (MSB_NW + MSS_R)               // 42 staged pixels per row
#define MSB_HH (MSB_NH + MSS_R)               // 32 staged rows

struct mss_window {
    double g[MSS_WIN];
};

static mss_window mss_make_window() {
    mss_window w;
    double s = 0.0;
    for (int i = 0; i < MSS_WIN; ++i) {
        const double d = (double)(i - MSS_WIN / 2);
        w.g[i] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
        s += w.g[i];
    }
    for (int i = 0; i < MSS_WIN; ++i) w.g[i] /= s;
    return w;
}

// Stages the ROWS x COLS pixels of x and y whose first is (oy, ox) as float64, 0 outside the image.  All of a thread's loads are
// issued before the first is used: a loop that loads, converts and stores one pixel at a time pays the memory latency once per
// pass instead of once per tile.
template <class T, int ROWS, int COLS>
__device__ __forceinline__ void mss_stage(const T* __restrict__ px, const T* __restrict__ py, int H, int W, int oy, int ox,
                                          double (*sx)[COLS], double (*sy)[COLS], int tid) {
    constexpr int NLD = (ROWS * COLS + MSS_THREADS - 1) / MSS_THREADS;
    T u[NLD], v[NLD];
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
        const int i = tid + j * MSS_THREADS, r = i / COLS, c = i - r * COLS;
        const int y = oy + r, x = ox + c;
        u[j] = (T)0;
        v[j] = (T)0;
        if (i < ROWS * COLS && y >= 0 && y < H && x >= 0 && x < W) {
            const int64_t o = (int64_t)y * W + x;
            u[j] = px[o];
            v[j] = py[o];
        }
    }
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
        const int i = tid + j * MSS_THREADS, r = i / COLS, c = i - r * COLS;
        if (i < ROWS * COLS) {
            sx[r][c] = (double)u[j];
            sy[r][c] = (double)v[j];
        }
    }
}

// grid (tiles, min(planes, MSS_MAX_GRID_Y)); partial: [planes][tiles][2] = the tile's sums of l cs and of cs
template <class T>
__global__ __launch_bounds__(MSS_THREADS) void msssim_fwd_kernel(const T* __restrict__ pred, const T* __restrict__ target, int H,
                                                                 int W, int64_t planes, int tiles_x, int tiles_y, double C1,
                                                                 double C2, mss_window win, double* __restrict__ partial,
                                                                 double* __restrict__ pool_pred, double* __restrict__ pool_target) {
    __shared__ double hx[MSF_HH][MSF_HW];
    __shared__ double hy[MSF_HH][MSF_HW];
    __shared__ double rm[5][MSF_HH][MSF_TW];       // the five moments after the row pass
    // the reduction tree reuses the moments' space once the column pass is done with them: 50,752 bytes of LDS, three workgroups
    // per CU instead of the two that 4 KiB more would leave
    double (*red)[MSS_THREADS] = (double (*)[MSS_THREADS])&rm[0][0][0];
    const int tid = threadIdx.x, lane = tid & 31, grp = tid >> 5;
    const int tile = blockIdx.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * MSF_TH, x0 = tx * MSF_TW;  // first window position = first staged pixel
    const int OH = H - MSS_R, OW = W - MSS_R;
    const int PH = H >> 1, PW = W >> 1;
    const int64_t HW = (int64_t)H * W, PHW = (int64_t)PH * PW;
    // the pixels this tile pools: its own rows and columns; the last tile of a direction also takes the 10 behind it, which
    // it has staged (y0 + MSF_TH >= OH there, so y0 + MSF_HH >= H)
    const int own_h = (ty == tiles_y - 1 ? H : y0 + MSF_TH) - y0, own_w = (tx == tiles_x - 1 ? W : x0 + MSF_TW) - x0;
    const int nph = own_h >> 1, npw = own_w >> 1;  // y0 and x0 are even: the 2x2 blocks do not straddle tiles
    for (int64_t pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        const T* __restrict__ px = pred + pl * HW;
        const T* __restrict__ py = target + pl * HW;
        mss_stage<T, MSF_HH, MSF_HW>(px, py, H, W, y0, x0, hx, hy, tid);
        __syncthreads();
        for (int r = grp; r < MSF_HH; r += MSS_GROUPS) {
            double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
            for (int k = 0; k < MSS_WIN; ++k) {
                const double u = hx[r][lane + k], v = hy[r][lane + k], gk = win.g[k];
                const double gu = gk * u, gv = gk * v;
                sx += gu; sy += gv; sxx += gu * u; syy += gv * v; sxy += gu * v;
            }
            rm[0][r][lane] = sx; rm[1][r][lane] = sy; rm[2][r][lane] = sxx; rm[3][r][lane] = syy; rm[4][r][lane] = sxy;
        }
        __syncthreads();
        double s_ssim = 0.0, s_cs = 0.0;
        for (int r = grp; r < MSF_TH; r += MSS_GROUPS) {
            if (y0 + r < OH && x0 + lane < OW) {
                double mx = 0, my = 0, mxx = 0, myy = 0, mxy = 0;
#pragma unroll
                for (int k = 0; k < MSS_WIN; ++k) {
                    const double gk = win.g[k];
                    mx += gk * rm[0][r + k][lane]; my += gk * rm[1][r + k][lane]; mxx += gk * rm[2][r + k][lane];
                    myy += gk * rm[3][r + k][lane]; mxy += gk * rm[4][r + k][lane];
                }
                const double D1 = mx * mx + my * my + C1, D2 = (mxx - mx * mx) + (myy - my * my) + C2;
                const double l = (2.0 * mx * my + C1) / D1, cs = (2.0 * (mxy - mx * my) + C2) / D2;
                s_ssim += l * cs;
                s_cs += cs;
            }
        }
        if (pool_pred) {
            double* __restrict__ qx = pool_pred + pl * PHW;
            double* __restrict__ qy = pool_target + pl * PHW;
            for (int i = tid; i < nph * npw; i += MSS_THREADS) {
                const int r = i / npw, c = i - r * npw;
                const int64_t o = (int64_t)((y0 >> 1) + r) * PW + (x0 >> 1) + c;
                qx[o] = 0.25 * ((hx[2 * r][2 * c] + hx[2 * r][2 * c + 1]) + (hx[2 * r + 1][2 * c] + hx[2 * r + 1][2 * c + 1]));
                qy[o] = 0.25 * ((hy[2 * r][2 * c] + hy[2 * r][2 * c + 1]) + (hy[2 * r + 1][2 * c] + hy[2 * r + 1][2 * c + 1]));
            }
        }
        __syncthreads();                               // every lane has taken its column pass: the tree goes over the moments
        red[0][tid] = s_ssim;
        red[1][tid] = s_cs;
        __syncthreads();
        for (int s = MSS_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s) {
                red[0][tid] += red[0][tid + s];
                red[1][tid] += red[1][tid + s];
            }
            __syncthreads();
        }
        if (tid == 0) {
            double* __restrict__ q = partial + (pl * gridDim.x + tile) * 2;
            q[0] = red[0][0];
            q[1] = red[1][0];
        }
        __syncthreads();                               // the next plane overwrites what tid 0 and the pool have just read
    }
}

// grid min(planes, MSS_MAX_GRID_Y): one workgroup sums a plane's tile partials in a fixed order
__global__ __launch_bounds__(64) void msssim_finalize_kernel(const double* __restrict__ partial, int ntiles, int64_t planes,
                                                             double inv_count, double* __restrict__ ssim, double* __restrict__ cs) {
    __shared__ double red[2][64];
    const int tid = threadIdx.x;
    for (int64_t pl = blockIdx.x; pl < planes; pl += gridDim.x) {
        double a = 0.0, b = 0.0;
        for (int i = tid; i < ntiles; i += 64) {
            a += partial[(pl * ntiles + i) * 2];
            b += partial[(pl * ntiles + i) * 2 + 1];
        }
        red[0][tid] = a;
        red[1][tid] = b;
        __syncthreads();
        for (int s = 32; s > 0; s >>= 1) {
            if (tid < s) {
                red[0][tid] += red[0][tid + s];
                red[1][tid] += red[1][tid + s];
            }
            __syncthreads();
        }
        if (tid == 0) {
            ssim[pl] = red[0][0] * inv_count;
            cs[pl] = red[1][0] * inv_count;
        }
        __syncthreads();
    }
}

// grid (tiles, min(planes, MSS_MAX_GRID_Y)).  Two LDS regions, each used twice:
//   ha: the staged pixels of x and y [2][MSB_HH][MSB_HW]       -> the per-window A, B, Cc [3][MSB_NH][MSB_NW]
//   hb: the five moments after the row pass [5][MSB_HH][MSB_NW] -> A, B, Cc after the transposed row pass [3][MSB_NH][MSB_TW]
template <class T, class TO>
__global__ __launch_bounds__(MSS_THREADS) void msssim_bwd_kernel(const T* __restrict__ pred, const T* __restrict__ target, int H,
                                                                 int W, int64_t planes, int tiles_x, double C1, double C2,
                                                                 mss_window win, const double* __restrict__ coef_a,
                                                                 const double* __restrict__ coef_b,
                                                                 const double* __restrict__ g_coarse, TO* __restrict__ g_out) {
    __shared__ double ha[2 * MSB_HH * MSB_HW];
    __shared__ double hb[5 * MSB_HH * MSB_NW];
    const int tid = threadIdx.x, lane = tid & 31, grp = tid >> 5;
    const int tile = blockIdx.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * MSB_TH, x0 = tx * MSB_TW;      // first pixel of the tile
    const int hy0 = y0 - MSS_R, hx0 = x0 - MSS_R;      // first window that holds it = first staged pixel
    const int OH = H - MSS_R, OW = W - MSS_R;
    const int PH = H >> 1, PW = W >> 1;
    const int64_t HW = (int64_t)H * W, PHW = (int64_t)PH * PW;
    const double inv_count = 1.0 / ((double)OH * (double)OW);
    double (*sx)[MSB_HW] = (double (*)[MSB_HW])ha;                       // x, then y behind it
    double (*sy)[MSB_HW] = (double (*)[MSB_HW])(ha + MSB_HH * MSB_HW);
    double (*rm)[MSB_HH][MSB_NW] = (double (*)[MSB_HH][MSB_NW])hb;
    double (*wc)[MSB_NH][MSB_NW] = (double (*)[MSB_NH][MSB_NW])ha;
    double (*tr)[MSB_NH][MSB_TW] = (double (*)[MSB_NH][MSB_TW])hb;
    for (int64_t pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        const T* __restrict__ px = pred + pl * HW;
        const T* __restrict__ py = target + pl * HW;
        TO* __restrict__ go = g_out + pl * HW;
        const double* __restrict__ gc = g_coarse ? g_coarse + pl * PHW : nullptr;
        const double a = coef_a[pl], b = coef_b[pl];
        if (a == 0.0 && b == 0.0) {                    // uniform per workgroup: only the pool adjoint, exact zeros without it
            for (int ly = grp; ly < MSB_TH; ly += MSS_GROUPS) {
                const int y = y0 + ly, x = x0 + lane;
                if (lane < MSB_TW && y < H && x < W) {
                    double g = 0.0;
                    if (gc && (y >> 1) < PH && (x >> 1) < PW) g = 0.25 * gc[(int64_t)(y >> 1) * PW + (x >> 1)];
                    go[(int64_t)y * W + x] = (TO)g;
                }
            }
            continue;
        }
        mss_stage<T, MSB_HH, MSB_HW>(px, py, H, W, hy0, hx0, sx, sy, tid);
        __syncthreads();
        for (int r = grp; r < MSB_HH; r += MSS_GROUPS) {
            double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
            for (int k = 0; k < MSS_WIN; ++k) {
                const double u = sx[r][lane + k], v = sy[r][lane + k], gk = win.g[k];
                const double gu = gk * u, gv = gk * v;
                s0 += gu; s1 += gv; s2 += gu * u; s3 += gv * v; s4 += gu * v;
            }
            rm[0][r][lane] = s0; rm[1][r][lane] = s1; rm[2][r][lane] = s2; rm[3][r][lane] = s3; rm[4][r][lane] = s4;
        }
        __syncthreads();                               // every lane is done with x and y: A, B, Cc go over them
        for (int r = grp; r < MSB_NH; r += MSS_GROUPS) {
            const int wy = hy0 + r, wx = hx0 + lane;   // top-left pixel of this window
            double A = 0.0, B = 0.0, Cc = 0.0;
            if (wy >= 0 && wy < OH && wx >= 0 && wx < OW) {
                double mx = 0, my = 0, mxx = 0, myy = 0, mxy = 0;
#pragma unroll
                for (int k = 0; k < MSS_WIN; ++k) {
                    const double gk = win.g[k];
                    mx += gk * rm[0][r + k][lane]; my += gk * rm[1][r + k][lane]; mxx += gk * rm[2][r + k][lane];
                    myy += gk * rm[3][r + k][lane]; mxy += gk * rm[4][r + k][lane];
                }
                const double D1 = mx * mx + my * my + C1, D2 = (mxx - mx * mx) + (myy - my * my) + C2;
                const double l = (2.0 * mx * my + C1) / D1, cs = (2.0 * (mxy - mx * my) + C2) / D2;
                const double dl = (2.0 * my - 2.0 * mx * l) / D1, dcs = (-2.0 * my + 2.0 * mx * cs) / D2;
                const double w = a * l + b;
                A = a * (cs * dl + l * dcs) + b * dcs;
                B = -w * cs / D2;
                Cc = 2.0 * w / D2;
            }
            wc[0][r][lane] = A; wc[1][r][lane] = B; wc[2][r][lane] = Cc;
        }
        __syncthreads();                               // the moments are spent: the transposed row pass goes over them
        // pixel column lx lies in the windows at columns lx .. lx + 10 of the tile's window grid, at offset 10 - j inside them
        for (int r = grp; r < MSB_NH; r += MSS_GROUPS) {
            if (lane < MSB_TW) {
                double s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
                for (int j = 0; j < MSS_WIN; ++j) {
                    const double gk = win.g[MSS_R - j];
                    s0 += gk * wc[0][r][lane + j]; s1 += gk * wc[1][r][lane + j]; s2 += gk * wc[2][r][lane + j];
                }
                tr[0][r][lane] = s0; tr[1][r][lane] = s1; tr[2][r][lane] = s2;
            }
        }
        __syncthreads();
        for (int ly = grp; ly < MSB_TH; ly += MSS_GROUPS) {
            const int y = y0 + ly, x = x0 + lane;
            if (lane < MSB_TW && y < H && x < W) {
                double s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
                for (int j = 0; j < MSS_WIN; ++j) {
                    const double gk = win.g[MSS_R - j];
                    s0 += gk * tr[0][ly + j][lane]; s1 += gk * tr[1][ly + j][lane]; s2 += gk * tr[2][ly + j][lane];
                }
                const int64_t o = (int64_t)y * W + x;
                const double xv = (double)px[o], yv = (double)py[o];
                double g = inv_count * (s0 + 2.0 * xv * s1 + yv * s2);
                if (gc && (y >> 1) < PH && (x >> 1) < PW) g += 0.25 * gc[(int64_t)(y >> 1) * PW + (x >> 1)];
                go[o] = (TO)g;
            }
        }
        __syncthreads();                               // the next plane stages over what this pass has just read
    }
}

static int64_t mss_tiles(int H, int W, int th, int tw, int by_pixels) {
    const int eh = by_pixels ? H : H - MSS_R, ew = by_pixels ? W : W - MSS_R;
    return (int64_t)adh_ceil_div(eh, th) * adh_ceil_div(ew, tw);
}

static bool mss_overlap(uintptr_t a, uintptr_t na, uintptr_t b, uintptr_t nb) { return a < b + nb && b < a + na; }

extern "C" int adh_msssim_num_tiles(int H, int W) {
    if (H < MSS_WIN || W < MSS_WIN) return ADH_E_UNSUPPORTED;
    const int64_t t = mss_tiles(H, W, MSF_TH, MSF_TW, 0);
    return t > 0x7fffffff ? ADH_E_UNSUPPORTED : (int)t;
}

extern "C" int adh_msssim_level_fwd(void* stream, const void* pred, const void* target, int in_f64, int N, int H, int W,
                                    double data_range, double* partial, int ntiles, double* ssim, double* cs, double* pool_pred,
                                    double* pool_target) {
    if (!pred || !target || !partial || !ssim || !cs || N < 1 || N > 65535) return ADH_E_ARG;
    if ((in_f64 != 0 && in_f64 != 1) || (pool_pred == nullptr) != (pool_target == nullptr) || !(data_range > 0.0)) return ADH_E_ARG;
    if (H < MSS_WIN || W < MSS_WIN) return ADH_E_UNSUPPORTED;
    const int tiles = adh_msssim_num_tiles(H, W);
    if (tiles < 0) return tiles;
    if (ntiles != tiles) return ADH_E_ARG;
    const int64_t planes = (int64_t)N * 3;
    const uintptr_t in_bytes = (uintptr_t)planes * (uintptr_t)H * (uintptr_t)W * (in_f64 ? 8 : 4);
    const uintptr_t pool_bytes = (uintptr_t)planes * (uintptr_t)(H >> 1) * (uintptr_t)(W >> 1) * 8;
    if (pool_pred) {   // a tile writes pooled pixels while its neighbours still stage theirs
        const uintptr_t q[2] = {(uintptr_t)pool_pred, (uintptr_t)pool_target}, p[2] = {(uintptr_t)pred, (uintptr_t)target};
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j)
                if (mss_overlap(q[i], pool_bytes, p[j], in_bytes)) return ADH_E_ARG;
        if (mss_overlap(q[0], pool_bytes, q[1], pool_bytes)) return ADH_E_ARG;
    }
    const double C1 = (0.01 * data_range) * (0.01 * data_range), C2 = (0.03 * data_range) * (0.03 * data_range);
    const mss_window win = mss_make_window();
    const int tiles_x = adh_ceil_div(W - MSS_R, MSF_TW), tiles_y = adh_ceil_div(H - MSS_R, MSF_TH);
    const dim3 grid((unsigned)tiles, (unsigned)(planes < MSS_MAX_GRID_Y ? planes : MSS_MAX_GRID_Y));
    if (in_f64)
        hipLaunchKernelGGL((msssim_fwd_kernel<double>), grid, dim3(MSS_THREADS), 0, (hipStream_t)stream, (const double*)pred,
                           (const double*)target, H, W, planes, tiles_x, tiles_y, C1, C2, win, partial, pool_pred, pool_target);
    else
        hipLaunchKernelGGL((msssim_fwd_kernel<float>), grid, dim3(MSS_THREADS), 0, (hipStream_t)stream, (const float*)pred,
                           (const float*)target, H, W, planes, tiles_x, tiles_y, C1, C2, win, partial, pool_pred, pool_target);
    hipLaunchKernelGGL(msssim_finalize_kernel, dim3(grid.y), dim3(64), 0, (hipStream_t)stream, partial, tiles, planes,
                       1.0 / ((double)(H - MSS_R) * (double)(W - MSS_R)), ssim, cs);
    return adh_check_launch();
}

extern "C" int adh_msssim_level_bwd(void* stream, const void* pred, const void* target, int in_f64, int N, int H, int W,
                                    double data_range, const double* coef_a, const double* coef_b, const double* g_coarse,
                                    void* g_out, int out_f64) {
    if (!pred || !target || !coef_a || !coef_b || !g_out || N < 1 || N > 65535) return ADH_E_ARG;
    if ((in_f64 != 0 && in_f64 != 1) || (out_f64 != 0 && out_f64 != 1) || !(data_range > 0.0)) return ADH_E_ARG;
    if (H < MSS_WIN || W < MSS_WIN) return ADH_E_UNSUPPORTED;
    const int64_t planes = (int64_t)N * 3;
    const uintptr_t px = (uintptr_t)planes * (uintptr_t)H * (uintptr_t)W;
    const uintptr_t in_bytes = px * (in_f64 ? 8 : 4), out_bytes = px * (out_f64 ? 8 : 4);
    // a tile reads pixels that its neighbours write: the gradient may not overlap either image (or the gradient it folds in)
    if (mss_overlap((uintptr_t)g_out, out_bytes, (uintptr_t)pred, in_bytes) ||
        mss_overlap((uintptr_t)g_out, out_bytes, (uintptr_t)target, in_bytes))
        return ADH_E_ARG;
    if (g_coarse && mss_overlap((uintptr_t)g_out, out_bytes, (uintptr_t)g_coarse,
                                (uintptr_t)planes * (uintptr_t)(H >> 1) * (uintptr_t)(W >> 1) * 8))
        return ADH_E_ARG;
    const int64_t tiles = mss_tiles(H, W, MSB_TH, MSB_TW, 1);
    if (tiles > 0x7fffffff) return ADH_E_UNSUPPORTED;
    const double C1 = (0.01 * data_range) * (0.01 * data_range), C2 = (0.03 * data_range) * (0.03 * data_range);
    const mss_window win = mss_make_window();
    const int tiles_x = adh_ceil_div(W, MSB_TW);
    const dim3 grid((unsigned)tiles, (unsigned)(planes < MSS_MAX_GRID_Y ? planes : MSS_MAX_GRID_Y));
#define MSS_BWD(TI, TO)                                                                                                          \
    hipLaunchKernelGGL((msssim_bwd_kernel<TI, TO>), grid, dim3(MSS_THREADS), 0, (hipStream_t)stream, (const TI*)pred,           \
                       (const TI*)target, H, W, planes, tiles_x, C1, C2, win, coef_a, coef_b, g_coarse, (TO*)g_out)
    if (in_f64 && out_f64) MSS_BWD(double, double);
    else if (in_f64) MSS_BWD(double, float);
    else if (out_f64) MSS_BWD(float, double);
    else MSS_BWD(float, float);
#undef MSS_BWD
    return adh_check_launch();
}
