// The pieces the BatchNorm streaming kernels share (bn_act.hip, densenet.hip; the layout helpers and the activations also
// cbam.hip and depthwise.hip), each said once.  common.h includes it at its end, and so does tools/host_emu/common.h, which stands
// in for common.h in the host-emulation build: hipcc and the sanitizer runs compile this one text.
#pragma once

// ---------------------------------------------------------------------------------------------
// The activations of the BatchNorm / depthwise epilogues: value at the pre-activation z, and g times the derivative at z with
// torch autograd's kink conventions (ReLU6: 0 at z = 0 and 6; Hardswish: 0 for z <= -3, 1 for z >= 3; Hardsigmoid: 1/6 only
// for -3 < z < 3).  The backward passes always work from z, never from the output (Hardswish is not invertible).
// ---------------------------------------------------------------------------------------------
__host__ __device__ static inline bool adh_act_valid(int act) {
    return act == ADH_ACT_NONE || act == ADH_ACT_RELU || act == ADH_ACT_RELU6 || act == ADH_ACT_HARDSWISH ||
           act == ADH_ACT_HARDSIGMOID;
}
static inline bool adh_act_host_valid(int act) { return adh_act_valid(act); }
__device__ __forceinline__ float adh_act_fwd(int act, float z) {
    switch (act) {
        case ADH_ACT_RELU: return fmaxf(z, 0.f);
        case ADH_ACT_RELU6: return fminf(fmaxf(z, 0.f), 6.f);
        case ADH_ACT_HARDSWISH: return z * fminf(fmaxf(z + 3.f, 0.f), 6.f) / 6.f;
        case ADH_ACT_HARDSIGMOID: return fminf(fmaxf(z + 3.f, 0.f), 6.f) / 6.f;
        default: return z;
    }
}
__device__ __forceinline__ float adh_act_bwd(int act, float z, float g) {
    switch (act) {
        case ADH_ACT_RELU: return z > 0.f ? g : 0.f;
        case ADH_ACT_RELU6: return (z > 0.f && z < 6.f) ? g : 0.f;
        case ADH_ACT_HARDSWISH: return z <= -3.f ? 0.f : (z < 3.f ? g * (z / 3.f + 0.5f) : g);
        case ADH_ACT_HARDSIGMOID: return (z > -3.f && z < 3.f) ? g / 6.f : 0.f;
        default: return g;
    }
}

// ---------------------------------------------------------------------------------------------
// Streaming layout of the element-wise kernels (bn_apply, bn_bwd_apply, bn_preact_bwd_accum, cbam_scale, cbam_bwd_e): the launch
// has T = gridDim.x * 256 threads with T a multiple of CQ (channel quads per pixel), so a thread keeps one channel quad for the
// whole sweep -- its per-channel constants are loaded once and no index division happens inside the loop -- and walks pixels
// p, p + pstep, ... `unroll` at a time.
// ---------------------------------------------------------------------------------------------
// blocks of 256 threads for P pixels: one trip of `unroll` pixels per thread, capped at maxblk, rounded up to a multiple of
// CQ / gcd(CQ, 256)
static inline int adh_stream_blocks(int64_t P, int CQ, int unroll, int maxblk) {
    int g = CQ, r = 256;   // gcd(CQ, 256)
    while (r) { const int t = g % r; g = r; r = t; }
    const int mult = CQ / g;                                  // blocks must be a multiple of this
    int64_t want = (P * CQ + 256 * unroll - 1) / (256 * unroll);
    if (want > maxblk) want = maxblk;
    int64_t blocks = (want + mult - 1) / mult * mult;
    if (blocks < mult) blocks = mult;
    return (int)blocks;
}
// this thread's first pixel p, its pixel step and the first channel c of its quad
__device__ __forceinline__ void adh_stream_decode(int CQ, int64_t& p, int64_t& pstep, int& c) {
    const int64_t t = blockIdx.x * (int64_t)256 + threadIdx.x;
    pstep = (int64_t)gridDim.x * 256 / CQ;
    p = t / CQ;
    c = (int)(t - p * CQ) * 4;
}

// ---------------------------------------------------------------------------------------------
// The gradient behind the activation, g times act'(pre-activation), as the forward pass decided it.  bn_apply_kernel's
// w = fmaf(y, scale, shift) is repeated here exactly: the forward pass and both backward passes must agree on every kink.
//   bits:  ReLU from bn_apply's nibble mask `mb` (bit j = element j passed)
//   ss:    ReLU / ReLU6 / Hardswish / Hardsigmoid from the pre-activation recomputed from y and the forward's (msc, msh)
//   else:  ReLU from the forward's output `o`
// Operands a form does not use may be uninitialised: they are taken by reference and not read.  bn_bwd_reduce_kernel calls it;
// bn_bwd_apply_kernel and bn_preact_bwd_accum_kernel carry the same text written out, because they measured slower through it.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ f32x4 bn_masked_grad(f32x4 gg, int act, bool bits, const int& mb, bool ss, const f32x4& yy,
                                                const f32x4& msc, const f32x4& msh, const f32x4& o) {
    if (bits) {
#pragma unroll
        for (int j = 0; j < 4; ++j) gg[j] = ((mb >> j) & 1) ? gg[j] : 0.f;
    } else if (act == ADH_ACT_RELU) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float ov = ss ? fmaf(yy[j], msc[j], msh[j]) : o[j];
            gg[j] = ov > 0.f ? gg[j] : 0.f;
        }
    } else if (act != ADH_ACT_NONE) {   // the derivative at the pre-activation (ss is required)
#pragma unroll
        for (int j = 0; j < 4; ++j) gg[j] = adh_act_bwd(act, fmaf(yy[j], msc[j], msh[j]), gg[j]);
    }
    return gg;
}

// ---------------------------------------------------------------------------------------------
// Per-block sums of the pixel-block kernels (bn_bwd_reduce, bn_slice_stats): 256 threads, channels in groups of at most 1024
// (256 quads, one per thread): one group for every layer of the dehazing branches, two for the 2048-channel BatchNorms of the
// resnet50 HDEN.  With CQ quads in the group, R = 256 / CQ pixel rows run concurrently; thread = (prow, quad).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void bn_group_decode(int C, int cbase, int& CQ, int& R, int& prow, int& c) {
    CQ = (C - cbase < 1024 ? C - cbase : 1024) / 4;
    R = 256 / CQ;
    const int cq = threadIdx.x % CQ;
    prow = threadIdx.x / CQ;   // rows >= R are idle
    c = cbase + cq * 4;
}
// partials[blockIdx.x][0 / 1][c .. c + 3] = the sum over the pixel rows of (a, b), in row order; every thread calls it
__device__ __forceinline__ void bn_block_fold(f32x4 (&red)[2][256], const f32x4& a, const f32x4& b, int CQ, int R, int c, int C,
                                              float* partials) {
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    if (threadIdx.x < CQ) {
        f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};
        for (int r = 0; r < R; ++r) {
            sa += red[0][r * CQ + threadIdx.x];
            sb += red[1][r * CQ + threadIdx.x];
        }
        *reinterpret_cast<f32x4*>(partials + ((size_t)blockIdx.x * 2 + 0) * C + c) = sa;
        *reinterpret_cast<f32x4*>(partials + ((size_t)blockIdx.x * 2 + 1) * C + c) = sb;
    }
    __syncthreads();   // (the next channel group reuses `red`)
}

// ---------------------------------------------------------------------------------------------
// fp64 column sums of partials[nblk][2][pitch] in a fixed order: a block of 1024 threads takes 32 channels x 32 row slices,
// every thread keeps CHAINS (2 or 4) independent chains of rows 32 apart in flight (the loop is latency-bound), the chains
// are paired (s0 + s1) + (s2 + s3) and the 32 slices summed in order.  Returns true in the thread that holds (S, Q) of
// channel c (row slice 0, c < C); every thread of the block calls it.
// (bn_finalize_kernel paired its four chains (s0 + s2) + (s1 + s3) before it called this: its S and Q may differ from that
// form's by one rounding of 2^-53.)
// ---------------------------------------------------------------------------------------------
template <int CHAINS>
__device__ __forceinline__ bool bn_column_sums(const float* __restrict__ partials, int nblk, int pitch, int C,
                                               double (&red)[2][32][33], int& c, double& S, double& Q) {
    static_assert(CHAINS == 2 || CHAINS == 4, "two or four chains");
    const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
    c = blockIdx.x * 32 + cx;
    double s[CHAINS] = {}, q[CHAINS] = {};
    if (c < C) {
        int b = ry;
        for (; b + 32 * (CHAINS - 1) < nblk; b += 32 * CHAINS) {
#pragma unroll
            for (int k = 0; k < CHAINS; ++k) {
                s[k] += (double)partials[((size_t)(b + 32 * k) * 2 + 0) * pitch + c];
                q[k] += (double)partials[((size_t)(b + 32 * k) * 2 + 1) * pitch + c];
            }
        }
        for (; b < nblk; b += 32) {
            s[0] += (double)partials[((size_t)b * 2 + 0) * pitch + c];
            q[0] += (double)partials[((size_t)b * 2 + 1) * pitch + c];
        }
    }
    if constexpr (CHAINS == 4) {
        red[0][ry][cx] = (s[0] + s[1]) + (s[2] + s[3]);
        red[1][ry][cx] = (q[0] + q[1]) + (q[2] + q[3]);
    } else {
        red[0][ry][cx] = s[0] + s[1];
        red[1][ry][cx] = q[0] + q[1];
    }
    __syncthreads();
    if (ry != 0 || c >= C) return false;
    S = 0.0;
    Q = 0.0;
    for (int r = 0; r < 32; ++r) {
        S += red[0][r][cx];
        Q += red[1][r][cx];
    }
    return true;
}

// sum, sum of squares, count -> mean and the biased variance, clamped at 0
__device__ __forceinline__ void bn_mean_var(double S, double Q, double count, double& mean, double& var) {
    mean = S / count;
    var = Q / count - mean * mean;
    if (var < 0.0) var = 0.0;
}

// One channel of nn.BatchNorm2d's train-mode bookkeeping from its moments: the folded scale / shift, the saved mean / invstd,
// the running statistics (momentum, unbiased variance) and the counter (one writer: channel 0).
__device__ __forceinline__ void bn_fold_channel(int c, double mean, double var, double count, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, float eps, float momentum, float* running_mean,
                                                float* running_var, float* scale, float* shift, float* save_mean,
                                                float* save_invstd, int64_t* num_batches_tracked) {
    const double invstd = 1.0 / sqrt(var + (double)eps);
    const float gm = gamma ? gamma[c] : 1.f;
    const float bt = beta ? beta[c] : 0.f;
    scale[c] = (float)(gm * invstd);
    shift[c] = (float)(bt - mean * gm * invstd);
    if (save_mean) save_mean[c] = (float)mean;
    if (save_invstd) save_invstd[c] = (float)invstd;
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mean;
    if (running_var) {
        const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
    }
    if (num_batches_tracked && c == 0) *num_batches_tracked += 1;     // BatchNorm2d's counter (one writer)
}

// One channel of the BatchNorm backward's middle step: dbeta / dgamma (= or +=) from the sums (dS, dQ) = (sum g, sum g xhat),
// and coef[3][C] = (gamma * invstd, mean g, mean g xhat) for the input-gradient pass from the sums (mS, mQ) over `count`
// elements.  (dS, dQ) and (mS, mQ) differ only under synchronised BatchNorm: this rank's sums and the sums of all ranks.
__device__ __forceinline__ void bn_bwd_coef_channel(int c, int C, double dS, double dQ, double mS, double mQ, double count,
                                                    const float* gamma, const float* invstd, float* dgamma, float* dbeta,
                                                    int accumulate, float* coef) {
    if (dgamma) dgamma[c] = accumulate ? dgamma[c] + (float)dQ : (float)dQ;
    if (dbeta) dbeta[c] = accumulate ? dbeta[c] + (float)dS : (float)dS;
    coef[0 * C + c] = (gamma ? gamma[c] : 1.f) * invstd[c];
    coef[1 * C + c] = (float)(mS / count);
    coef[2 * C + c] = (float)(mQ / count);
}
