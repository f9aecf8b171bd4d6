// DenseNet121 training passes (torchvision densenet.py _DenseLayer / _Transition / norm5), gfx950.
// A dense block keeps all of its features in one NHWC buffer [N,H,W,c0 + 32 L] written in place; every layer's norm1 is a
// pre-activation BatchNorm + ReLU over the channel slice [0, c) of that buffer (channel stride = the buffer's width).
// Train-mode batch statistics are per channel and do not depend on the layer, so they are taken once per channel --
// the block input by adh_bn_slice_stats, each 32-channel growth slice by its conv2's epilogue -- kept as fp64 moments of the
// whole buffer, and every BatchNorm only folds its own gamma / beta (adh_bn_fold_moments).  The backward pass adds each
// layer's input gradient into the one gradient buffer of the block (adh_bn_preact_bwd_accum).  Streaming kernels: 16 B per
// lane, a channel quad per thread, per-block partial sums reduced in a fixed order (bit-reproducible).
#include "common.h"

// ---------------------------------------------------------------------------------------------
// statistics of a strided channel slice: partials[b][0][c] = sum x, partials[b][1][c] = sum x^2 over pixel block b
// (the layout adh_bn_finalize / adh_bn_partial_sums / adh_bn_slice_moments read, pitch C)
// ---------------------------------------------------------------------------------------------
#define SS_PPB 512     // pixels per block (as adh_bn_bwd_reduce)
#define SS_UNROLL 4

extern "C" int adh_bn_slice_stats_num_blocks(int64_t P, int C) {
    (void)C;
    return P < 1 ? ADH_E_ARG : adh_ceil_div(P, SS_PPB);
}

__global__ __launch_bounds__(256) void bn_slice_stats_kernel(const float* __restrict__ x, int x_cs, int64_t P, int C,
                                                             float* __restrict__ partials) {
    __shared__ f32x4 red[2][256];
    for (int cbase = 0; cbase < C; cbase += 1024) {     // channel groups (bn_stream.h)
        int CQ, R, prow, c;
        bn_group_decode(C, cbase, CQ, R, prow, c);
        f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = s;
        if (prow < R) {
            const int64_t p0 = (int64_t)blockIdx.x * SS_PPB;
            const int64_t p1 = p0 + SS_PPB < P ? p0 + SS_PPB : P;
            for (int64_t p = p0 + prow; p < p1; p += SS_UNROLL * R) {
                f32x4 v[SS_UNROLL];
#pragma unroll
                for (int u = 0; u < SS_UNROLL; ++u) {
                    const int64_t r = p + u * R < p1 ? p + u * R : p;
                    v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(x + r * x_cs + c));
                }
#pragma unroll
                for (int u = 0; u < SS_UNROLL; ++u)
                    if (p + u * R < p1) {
                        s += v[u];
                        q += v[u] * v[u];
                    }
            }
        }
        bn_block_fold(red, s, q, CQ, R, c, C, partials);
    }
}

extern "C" int adh_bn_slice_stats(void* stream, const float* x, int x_cs, int64_t P, int C, float* partials) {
    if (!x || !partials || P < 1 || C < 4 || (C & 3) || C > 4096 || x_cs < C || (x_cs & 3)) return ADH_E_ARG;
    hipLaunchKernelGGL(bn_slice_stats_kernel, dim3(adh_bn_slice_stats_num_blocks(P, C)), dim3(256), 0, (hipStream_t)stream, x,
                       x_cs, P, C, partials);
    return adh_check_launch();
}

// ---------------------------------------------------------------------------------------------
// partials[nblk][2][pitch] (sum, sum of squares) -> fp64 mean[c] and biased variance var[c] (fixed-order fp64 reduce)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void bn_slice_moments_kernel(const float* __restrict__ partials, int nblk, int pitch, int C,
                                                                double count, double* __restrict__ mean,
                                                                double* __restrict__ var) {
    __shared__ double red[2][32][33];
    int c;
    double S, Q, m, v;
    if (!bn_column_sums<2>(partials, nblk, pitch, C, red, c, S, Q)) return;
    bn_mean_var(S, Q, count, m, v);
    mean[c] = m;
    var[c] = v;
}

extern "C" int adh_bn_slice_moments(void* stream, const float* partials, int nblk, int pitch, int C, double count, double* mean,
                                    double* var) {
    if (!partials || !mean || !var || nblk < 1 || C < 1 || pitch < C || count <= 0) return ADH_E_ARG;
    hipLaunchKernelGGL(bn_slice_moments_kernel, dim3(adh_ceil_div(C, 32)), dim3(1024), 0, (hipStream_t)stream, partials, nblk,
                       pitch, C, count, mean, var);
    return adh_check_launch();
}

// ---------------------------------------------------------------------------------------------
// one BatchNorm2d of the block from the shared moments: scale / shift / mean / invstd and nn.BatchNorm2d's buffer update
// (momentum, unbiased running variance, num_batches_tracked += 1) -- bn_fold_channel, as adh_bn_finalize after its reduce
// ---------------------------------------------------------------------------------------------
__global__ void bn_fold_moments_kernel(int C, const double* __restrict__ mean, const double* __restrict__ var, double count,
                                       const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                       float momentum, float* running_mean, float* running_var, float* scale, float* shift,
                                       float* save_mean, float* save_invstd, int64_t* num_batches_tracked) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    bn_fold_channel(c, mean[c], var[c], count, gamma, beta, eps, momentum, running_mean, running_var, scale, shift, save_mean,
                    save_invstd, num_batches_tracked);
}

extern "C" int adh_bn_fold_moments(void* stream, int C, const double* mean, const double* var, double count, const float* gamma,
                                   const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                                   float* scale, float* shift, float* save_mean, float* save_invstd,
                                   int64_t* num_batches_tracked) {
    if (C < 1 || !mean || !var || !scale || !shift || count <= 0) return ADH_E_ARG;
    hipLaunchKernelGGL(bn_fold_moments_kernel, dim3(adh_ceil_div(C, 256)), dim3(256), 0, (hipStream_t)stream, C, mean, var, count,
                       gamma, beta, eps, momentum, running_mean, running_var, scale, shift, save_mean, save_invstd,
                       num_batches_tracked);
    return adh_check_launch();
}

// ---------------------------------------------------------------------------------------------
// AvgPool2d(2, 2) backward with F.avg_pool2d's floor: gx[n][iy][ix] = g[n][iy/2][ix/2] / 4 for iy < 2 OH, ix < 2 OW, and 0
// in the dropped last row / column of an odd H / W.  accumulate != 0: gx += instead of gx =.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void avgpool2_bwd_kernel(const float* __restrict__ g, int g_cs, int H, int W, int CQ,
                                                           float* __restrict__ gx, int gx_cs, int accumulate) {
    const int n = blockIdx.y;
    const int OH = H >> 1, OW = W >> 1;
    const int64_t total = (int64_t)H * W * CQ;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ip = t / CQ;
        const int c = (int)(t - ip * CQ) * 4;
        const int iy = (int)(ip / W), ix = (int)(ip - (int64_t)iy * W);
        const int oy = iy >> 1, ox = ix >> 1;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (oy < OH && ox < OW)
            v = *reinterpret_cast<const f32x4*>(g + ((size_t)n * OH * OW + (size_t)oy * OW + ox) * g_cs + c) * 0.25f;
        f32x4* d = reinterpret_cast<f32x4*>(gx + ((size_t)n * H * W + ip) * gx_cs + c);
        if (accumulate) v += *d;
        *d = v;
    }
}

extern "C" int adh_avgpool2_bwd(void* stream, const float* g, int g_cs, int N, int H, int W, int C, float* gx, int gx_cs,
                                int accumulate) {
    if (!g || !gx || N < 1 || H < 2 || W < 2 || C < 4 || (C & 3) || g_cs < C || gx_cs < C || (g_cs & 3) || (gx_cs & 3))
        return ADH_E_ARG;
    hipLaunchKernelGGL(avgpool2_bwd_kernel, dim3(adh_min_i(adh_ceil_div((int64_t)H * W * (C / 4), 256), 4096), N), dim3(256), 0,
                       (hipStream_t)stream, g, g_cs, H, W, C / 4, gx, gx_cs, accumulate);
    return adh_check_launch();
}

// ---------------------------------------------------------------------------------------------
// pre-activation BatchNorm + ReLU backward into the block's gradient buffer:
//   m = [fma(x, scale, shift) > 0] (the forward expression, from x and the layer's folded scale / shift = ss[0] / ss[1])
//   training:  dx = coef0 * (m dA - coef1 - (x - mean) * invstd * coef2)   (coef = adh_bn_bwd_finalize's [3][C] output:
//              gamma * invstd, mean(m dA), mean(m dA xhat))
//   frozen statistics: dx = coef0 * m dA   (coef0 = the folded scale)
//   dbuf[p][c] += dx (accumulate != 0) or = dx, at dbuf's channel stride
// ---------------------------------------------------------------------------------------------
#define PB_MAXBLK (256 * 32)   // the three-stream grid cap adh_bn_bwd_apply measured fastest
#define PB_UNROLL 8

__global__ __launch_bounds__(256) void bn_preact_bwd_accum_kernel(const float* __restrict__ dA, int dA_cs,
                                                                  const float* __restrict__ x, int x_cs,
                                                                  const float* __restrict__ ss, const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd,
                                                                  const float* __restrict__ coef, int training,
                                                                  float* __restrict__ dbuf, int dbuf_cs, int64_t P, int C,
                                                                  int accumulate) {
    int64_t p, pstep;
    int c;
    adh_stream_decode(C / 4, p, pstep, c);
    const f32x4 k0 = *reinterpret_cast<const f32x4*>(coef + c);
    const f32x4 msc = *reinterpret_cast<const f32x4*>(ss + c);
    const f32x4 msh = *reinterpret_cast<const f32x4*>(ss + C + c);
    f32x4 mg = {0.f, 0.f, 0.f, 0.f}, kx = mg, mu = mg;
    if (training) {
        mg = *reinterpret_cast<const f32x4*>(coef + C + c);
        mu = *reinterpret_cast<const f32x4*>(mean + c);
        kx = *reinterpret_cast<const f32x4*>(invstd + c) * *reinterpret_cast<const f32x4*>(coef + 2 * C + c);
    }
    for (; p < P; p += PB_UNROLL * pstep) {
        f32x4 g[PB_UNROLL], xx[PB_UNROLL], d[PB_UNROLL];
#pragma unroll
        for (int u = 0; u < PB_UNROLL; ++u) {
            const int64_t q = p + u * pstep < P ? p + u * pstep : p;
            g[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(dA + q * dA_cs + c));
            xx[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(x + q * x_cs + c));
            if (accumulate) d[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(dbuf + q * dbuf_cs + c));
        }
#pragma unroll
        for (int u = 0; u < PB_UNROLL; ++u) {
            const int64_t q = p + u * pstep;
            if (q < P) {
                f32x4 gg = g[u];   // bn_masked_grad's (bn_stream.h) ReLU-from-(scale, shift) form, written out: through the helper
#pragma unroll             // hipcc allocates this kernel's registers differently (156 -> 158 VGPRs) and it measured slower
                for (int j = 0; j < 4; ++j) gg[j] = fmaf(xx[u][j], msc[j], msh[j]) > 0.f ? gg[j] : 0.f;
                f32x4 r = training ? k0 * (gg - mg - (xx[u] - mu) * kx) : k0 * gg;
                if (accumulate) r += d[u];
                __builtin_nontemporal_store(r, reinterpret_cast<f32x4*>(dbuf + q * dbuf_cs + c));
            }
        }
    }
}

extern "C" int adh_bn_preact_bwd_accum(void* stream, const float* dA, int dA_cs, const float* x, int x_cs, const float* ss,
                                       const float* mean, const float* invstd, const float* coef, int training, float* dbuf,
                                       int dbuf_cs, int64_t P, int C, int accumulate) {
    if (!dA || !x || !ss || !coef || !dbuf || P < 1 || C < 4 || (C & 3) || dA_cs < C || x_cs < C || dbuf_cs < C ||
        ((dA_cs | x_cs | dbuf_cs) & 3))
        return ADH_E_ARG;
    if (training && (!mean || !invstd)) return ADH_E_ARG;
    hipLaunchKernelGGL(bn_preact_bwd_accum_kernel, dim3(adh_stream_blocks(P, C / 4, PB_UNROLL, PB_MAXBLK)), dim3(256), 0,
                       (hipStream_t)stream, dA, dA_cs, x, x_cs, ss, mean, invstd, coef, training, dbuf, dbuf_cs, P, C, accumulate);
    return adh_check_launch();
}
