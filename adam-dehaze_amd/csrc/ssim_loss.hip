// Backward of the per-image SSIM of csrc/train_io.hip (adh_ssim_gray), gfx950: the gradient of that number with respect to
// the predicted image, so that SSIM can be a loss term.  One fused pass, nothing saved by the forward:
//   x, y      fp32 channel-mean grayscale of pred / target, ((c0 + c1) + c2) / 3 as the forward forms it
//   per valid 7x7 window w (top-left (wy, wx), 0 <= wy <= H-7, 0 <= wx <= W-7), all in float64:
//     mx, my, mxx, myy, mxy  window means;  vx = cn (mxx - mx^2), vy = cn (myy - my^2), vxy = cn (mxy - mx my), cn = 49/48
//     A1 = 2 mx my + C1, A2 = 2 vxy + C2, B1 = mx^2 + my^2 + C1, B2 = vx + vy + C2, S = A1 A2 / (B1 B2)
//     a = 2 my A2/(B1 B2) - 2 mx S/B1 + 2 cn mx S/B2 - 2 cn my A1/(B1 B2),  b = -cn S/B2,  c = 2 cn A1/(B1 B2)
//   per pixel p, each of the 3 channels:
//     g_pred[n, ch, p] = g_ssim[n] / (3 * 49 * (H-6)(W-6)) * (sum_{w contains p} a_w + 2 x[p] sum b_w + y[p] sum c_w)
// One workgroup = SSIML_T x SSIML_T output pixels.  It stages the (T+12)^2 grayscale halos of both images in LDS, forms a, b, c
// at its (T+6)^2 window positions (0 at positions that are no valid window: off the image or past H-7 / W-7), then every
// thread takes the three 49-term transposed box sums of its four pixels.  Everything after the fp32 grayscale is float64
// with one rounding at the store: near pred = target, where training spends its time, 2 x sum b and y sum c cancel.
// No atomics and a fixed summation order: bit-reproducible.  No workspace.
#include "common.h"

#define SSIML_T 32                            // output pixels per tile side
#define SSIML_WIN 7
#define SSIML_NW (SSIML_T + SSIML_WIN - 1)    // 38 window positions per tile side
#define SSIML_HALO (SSIML_NW + SSIML_WIN - 1) // 44 grayscale pixels per tile side

__global__ __launch_bounds__(256) void ssim_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target, int H,
                                                       int W, float data_range, const float* __restrict__ g_ssim,
                                                       float* __restrict__ g_pred) {
    __shared__ float gx[SSIML_HALO][SSIML_HALO + 1];   // gray of pred
    __shared__ float gy[SSIML_HALO][SSIML_HALO + 1];   // gray of target
    __shared__ double wa[SSIML_NW][SSIML_NW + 1];
    __shared__ double wb[SSIML_NW][SSIML_NW + 1];
    __shared__ double wc[SSIML_NW][SSIML_NW + 1];
    const int n = blockIdx.y;
    const int OH = H - SSIML_WIN + 1, OW = W - SSIML_WIN + 1;
    const int tiles_x = (W + SSIML_T - 1) / SSIML_T;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * SSIML_T, x0 = tx * SSIML_T;    // first output pixel of the tile
    const int64_t HW = (int64_t)H * W;
    float* go = g_pred + (int64_t)n * 3 * HW;
    const int lx = threadIdx.x & 31, ly0 = threadIdx.x >> 5;
    const float gs = g_ssim[n];
    if (gs == 0.f) {                                   // uniform per workgroup: an image without upstream gradient gets exact zeros
        for (int k = 0; k < 4; ++k) {
            const int y = y0 + ly0 + 8 * k, x = x0 + lx;
            if (y < H && x < W) {
                const int64_t o = (int64_t)y * W + x;
                go[o] = 0.f; go[HW + o] = 0.f; go[2 * HW + o] = 0.f;
            }
        }
        return;
    }
    const float* pp = pred + (int64_t)n * 3 * HW;
    const float* pt = target + (int64_t)n * 3 * HW;
    // halo origin: the first window that contains the tile's first pixel starts 6 pixels before it
    const int hy0 = y0 - (SSIML_WIN - 1), hx0 = x0 - (SSIML_WIN - 1);
    for (int i = threadIdx.x; i < SSIML_HALO * SSIML_HALO; i += 256) {
        const int r = i / SSIML_HALO, c = i - r * SSIML_HALO;
        const int y = hy0 + r, x = hx0 + c;
        float a = 0.f, b = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const int64_t o = (int64_t)y * W + x;
            a = ((pp[o] + pp[HW + o]) + pp[2 * HW + o]) / 3.0f;
            b = ((pt[o] + pt[HW + o]) + pt[2 * HW + o]) / 3.0f;
        }
        gx[r][c] = a;
        gy[r][c] = b;
    }
    __syncthreads();
    const double C1 = (0.01 * data_range) * (0.01 * data_range), C2 = (0.03 * data_range) * (0.03 * data_range);
    const double NP = SSIML_WIN * SSIML_WIN, cn = NP / (NP - 1.0), inv = 1.0 / NP;
#pragma unroll 1
    for (int i = threadIdx.x; i < SSIML_NW * SSIML_NW; i += 256) {
        const int r = i / SSIML_NW, c = i - r * SSIML_NW;
        const int wy = hy0 + r, wx = hx0 + c;          // top-left of this window
        double a = 0.0, b = 0.0, cc = 0.0;
        if (wy >= 0 && wy < OH && wx >= 0 && wx < OW) {
            double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
            for (int dy = 0; dy < SSIML_WIN; ++dy)
#pragma unroll
                for (int dx = 0; dx < SSIML_WIN; ++dx) {
                    const double u = gx[r + dy][c + dx], v = gy[r + dy][c + dx];
                    sx += u; sy += v; sxx += u * u; syy += v * v; sxy += u * v;
                }
            const double mx = sx * inv, my = sy * inv;
            const double vx = cn * (sxx * inv - mx * mx), vy = cn * (syy * inv - my * my), vxy = cn * (sxy * inv - mx * my);
            const double A1 = 2 * mx * my + C1, A2 = 2 * vxy + C2, B1 = mx * mx + my * my + C1, B2 = vx + vy + C2;
            const double iB1 = 1.0 / B1, iB2 = 1.0 / B2, iB = iB1 * iB2;
            const double S = A1 * A2 * iB;
            a = 2 * (my * A2 * iB - mx * S * iB1 + cn * (mx * S * iB2 - my * A1 * iB));
            b = -cn * S * iB2;
            cc = 2 * cn * A1 * iB;
        }
        wa[r][c] = a;
        wb[r][c] = b;
        wc[r][c] = cc;
    }
    __syncthreads();
    const double coef = (double)gs / (3.0 * NP * (double)OH * (double)OW);
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const int ly = ly0 + 8 * k;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= H || x >= W) continue;
        // pixel (ly, lx) lies in the windows at positions [ly, ly+6] x [lx, lx+6] of the tile's window grid
        double sa = 0, sb = 0, sc = 0;
        for (int dy = 0; dy < SSIML_WIN; ++dy)
#pragma unroll
            for (int dx = 0; dx < SSIML_WIN; ++dx) {
                sa += wa[ly + dy][lx + dx];
                sb += wb[ly + dy][lx + dx];
                sc += wc[ly + dy][lx + dx];
            }
        const double xv = gx[ly + SSIML_WIN - 1][lx + SSIML_WIN - 1], yv = gy[ly + SSIML_WIN - 1][lx + SSIML_WIN - 1];
        const float g = (float)(coef * (sa + 2.0 * xv * sb + yv * sc));
        const int64_t o = (int64_t)y * W + x;
        go[o] = g; go[HW + o] = g; go[2 * HW + o] = g;
    }
}

extern "C" int adh_ssim_gray_bwd(void* stream, const float* pred_nchw, const float* target_nchw, int N, int H, int W,
                                 float data_range, const float* g_ssim, float* g_pred_nchw) {
    if (!pred_nchw || !target_nchw || !g_ssim || !g_pred_nchw || N < 1 || N > 65535) return ADH_E_ARG;
    if (H < SSIML_WIN || W < SSIML_WIN) return ADH_E_UNSUPPORTED;
    // a tile reads pixels that its neighbours write: the gradient may not overlap either image
    const uintptr_t g0 = (uintptr_t)g_pred_nchw, bytes = (uintptr_t)N * 3 * (uintptr_t)H * (uintptr_t)W * sizeof(float);
    const uintptr_t p0 = (uintptr_t)pred_nchw, t0 = (uintptr_t)target_nchw;
    if ((g0 < p0 + bytes && p0 < g0 + bytes) || (g0 < t0 + bytes && t0 < g0 + bytes)) return ADH_E_ARG;
    const int64_t tiles = (int64_t)adh_ceil_div(H, SSIML_T) * adh_ceil_div(W, SSIML_T);
    if (tiles > 0x7fffffff) return ADH_E_UNSUPPORTED;
    hipLaunchKernelGGL(ssim_bwd_kernel, dim3((unsigned)tiles, N), dim3(256), 0, (hipStream_t)stream, pred_nchw, target_nchw, H, W,
                       data_range, g_ssim, g_pred_nchw);
    return adh_check_launch();
}
