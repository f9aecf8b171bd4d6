// The eight symmetries of the square (D4: the flips and 90-degree rotations, which are also the eight EXIF orientations) on a
// dense fp32 [N,C,H,W] batch, gfx950: self-ensemble inference and EXIF orientation (image_io.py) are built on this one entry.
//
// Element definition (the contract).  dst is dense [N,C,Hd,Wd], (Hd,Wd) = transpose ? (W,H) : (H,W).
//     t = transpose ? src^T : src;  mirror t along x if bit 0 of the flip code is set;  mirror t along y if bit 1 is set.
// Equivalently  v(n,c,y',x') = src[n,c,y,x]  with
//     u = bit1 ? Hd-1-y' : y',   w = bit0 ? Wd-1-x' : x',   (y,x) = transpose ? (w,u) : (u,w).
// The flip code is `flips` for every image when flip_ops is NULL, else flip_ops[n] & 3 (a device int32[N]; the mask keeps any
// value from reaching an address).  The transpose bit is always the launch argument: one launch has one output shape.
// Stored value = accumulate ? dst + v : v (one fp32 add), then, if scale != 1.0f, __fmul_rn(., scale).  With accumulate == 0 and
// scale == 1 no arithmetic touches the value: a bit copy, NaN payloads and -0 survive.  An add followed by a product cannot be
// contracted into an FMA and the product is __fmul_rn, so the result is bit-equal to torch's ((dst + ref(src)) * scale) on the CPU.
//
// Non-transposing codes stream (the style of image_io.hip): a lane owns four neighbouring pixels of a dst row, one wave per
// row, four rows per workgroup; one 16-byte access per side where both bases are 16-byte aligned and W % 4 == 0 (then the
// mirrored quad, which starts at W - 4 - x, is aligned too), single floats otherwise; decided once per launch on the host.  For
// an x-mirror the lane reverses its four values.
// Transposing codes stage a D4_TILE x D4_TILE tile through LDS: the grid walks dst tiles, a wave reads a src row of the tile
// (coalesced along src x) and writes a dst row (coalesced along dst x); the sixteen rows of a wave are unrolled so that all
// its loads are in flight before the first LDS write (rolled up, each row waited for its own load).  The flips move the tile's
// src origin and reverse the in-tile indices, so all four transposing codes share one kernel.  The tile pitch is 65 dwords: ds_write_b32 and
// ds_read_b32 bank on (dword address) % 32 within each 32-lane half of the wave; the row-wise write puts lane l at r * 65 + l
// (32 consecutive dwords: 32 banks), the column-wise read puts lane l at (+-l) * 65 + c = +-l + c (mod 32): 32 banks again.
// Conflict degree 1 for both.  LDS is 16,640 bytes per workgroup of four waves, so LDS would let eight workgroups fill the 32
// wave slots of a CU; the registers of sixteen loads in flight (41-43 VGPRs) leave 7 waves per SIMD.
// The per-image flip code is one uniform load per workgroup and plane.  Planes (n, c) ride on grid z, rows / tile rows on grid y;
// both loop where the count exceeds 65,535.  All index arithmetic is 64-bit.
#include "common.h"

#define D4_QUAD 4      // pixels per lane (streaming kernel)
#define D4_ROWS 4      // rows per workgroup (one wave each)
#define D4_TILE 64     // tile edge (transposing kernel)
#define D4_PITCH 65    // tile pitch in dwords
#define D4_PER (D4_TILE / D4_ROWS)   // tile rows per wave

template <bool ACC>
__device__ __forceinline__ float d4_value(float v, float old, bool scaled, float scale) {
    if (ACC) v = old + v;
    if (scaled) v = __fmul_rn(v, scale);
    return v;
}

template <bool ACC>
__global__ __launch_bounds__(256) void d4_stream_kernel(const float* __restrict__ src, int64_t planes, int C, int H, int W, int flips,
                                                        const int32_t* __restrict__ flip_ops, float* __restrict__ dst,
                                                        float scale, int wide) {
    const int64_t x = ((int64_t)blockIdx.x * 64 + (threadIdx.x & 63)) * D4_QUAD;
    if (x >= W) return;
    const int npx = (W - x) < D4_QUAD ? (int)(W - x) : D4_QUAD;
    const int64_t plane = (int64_t)H * W;
    const bool scaled = scale != 1.0f;
    for (int64_t p = blockIdx.z; p < planes; p += gridDim.z) {
        const int code = flip_ops ? (flip_ops[p / C] & 3) : flips;
        const bool fx = code & 1, fy = code & 2;
        for (int64_t y = (int64_t)blockIdx.y * D4_ROWS + (threadIdx.x >> 6); y < H; y += (int64_t)gridDim.y * D4_ROWS) {
            const float* __restrict__ in = src + p * plane + (fy ? H - 1 - y : y) * W;
            float* __restrict__ out = dst + p * plane + y * W + x;
            if (npx == D4_QUAD && wide) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(in + (fx ? W - D4_QUAD - x : x));
                f32x4 o = {0.f, 0.f, 0.f, 0.f};
                if (ACC) o = *reinterpret_cast<const f32x4*>(out);
                f32x4 r;
#pragma unroll
                for (int j = 0; j < D4_QUAD; ++j) r[j] = d4_value<ACC>(fx ? q[D4_QUAD - 1 - j] : q[j], o[j], scaled, scale);
                *reinterpret_cast<f32x4*>(out) = r;
            } else {
#pragma unroll
                for (int j = 0; j < D4_QUAD; ++j)
                    if (j < npx) {
                        const float v = in[fx ? W - 1 - (x + j) : x + j];
                        out[j] = d4_value<ACC>(v, ACC ? out[j] : 0.f, scaled, scale);
                    }
            }
        }
    }
}

// src plane is [H][W], dst plane is [W][H]
template <bool ACC>
__global__ __launch_bounds__(256) void d4_transpose_kernel(const float* __restrict__ src, int64_t planes, int C, int H, int W,
                                                           int flips, const int32_t* __restrict__ flip_ops,
                                                           float* __restrict__ dst, float scale) {
    __shared__ float tile[D4_TILE * D4_PITCH];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // uniform: row checks and row bases are scalar
    const int64_t Hd = W, Wd = H;
    const int64_t plane = (int64_t)H * W;
    const int64_t tiles_y = (Hd + D4_TILE - 1) / D4_TILE;
    const int64_t dx0 = (int64_t)blockIdx.x * D4_TILE;
    const bool scaled = scale != 1.0f;
    for (int64_t p = blockIdx.z; p < planes; p += gridDim.z) {
        const int code = flip_ops ? (flip_ops[p / C] & 3) : flips;
        const bool fx = code & 1, fy = code & 2;
        const float* __restrict__ in = src + p * plane;
        float* __restrict__ out = dst + p * plane;
        for (int64_t ty = blockIdx.y; ty < tiles_y; ty += gridDim.y) {
            const int64_t dy0 = ty * D4_TILE;
            // dst (dy0 + j, dx0 + i) takes src (y, x) = (w, u): the tile's src origin, which an odd edge leaves partly outside
            const int64_t sy0 = fx ? Wd - dx0 - D4_TILE : dx0;
            const int64_t sx0 = fy ? Hd - dy0 - D4_TILE : dy0;
            const bool sx_in = sx0 + lane >= 0 && sx0 + lane < W;
            float v[D4_PER];                           // a wave's sixteen rows: every load is issued before the first LDS write
#pragma unroll
            for (int i = 0; i < D4_PER; ++i) {
                const int64_t sy = sy0 + wave + i * D4_ROWS;         // uniform, and so is the row's offset: a scalar base
                v[i] = (sx_in && sy >= 0 && sy < H) ? in[(sy * W + sx0) + lane] : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < D4_PER; ++i) tile[(wave + i * D4_ROWS) * D4_PITCH + lane] = v[i];
            __syncthreads();
            const bool ox_in = dx0 + lane < Wd;
            const int tr = fx ? D4_TILE - 1 - lane : lane;
            // the wave's tile columns are wave + 4 k whatever the code (constant LDS offsets); column c is dst row fy ? 63 - c : c
            const int64_t oy0 = dy0 + (fy ? D4_TILE - 1 - wave : wave), oys = fy ? -D4_ROWS : D4_ROWS;
            float old[D4_PER];
#pragma unroll
            for (int k = 0; k < D4_PER; ++k) {
                const int64_t oy = oy0 + k * oys;
                old[k] = (ACC && ox_in && oy < Hd) ? out[(oy * Wd + dx0) + lane] : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < D4_PER; ++k) {
                const int64_t oy = oy0 + k * oys;
                if (ox_in && oy < Hd)
                    out[(oy * Wd + dx0) + lane] = d4_value<ACC>(tile[tr * D4_PITCH + wave + k * D4_ROWS], old[k], scaled, scale);
            }
            __syncthreads();
        }
    }
}

extern "C" int adh_d4_apply(void* stream, const float* src, int N, int C, int H, int W, int transpose, int flips,
                            const int32_t* flip_ops, float* dst, int accumulate, float scale) {
    if (!src || !dst || N < 1 || C < 1 || H < 1 || W < 1) return ADH_E_ARG;
    if ((transpose != 0 && transpose != 1) || flips < 0 || flips > 3) return ADH_E_ARG;
    const int64_t planes = (int64_t)N * C;
    const uint64_t bytes = (uint64_t)planes * (uint64_t)H * (uint64_t)W * sizeof(float);
    const uintptr_t s = (uintptr_t)src, d = (uintptr_t)dst;
    if (s < d + bytes && d < s + bytes) return ADH_E_ARG;          // in place, or overlapping in part
    const unsigned gz = (unsigned)(planes < 65535 ? planes : 65535);
    if (!transpose) {
        const int wide = (((s | d) & 15) == 0 && (W & 3) == 0) ? 1 : 0;
        const dim3 grid((unsigned)adh_ceil_div(W, 64 * D4_QUAD), (unsigned)adh_min_i(adh_ceil_div(H, D4_ROWS), 65535), gz);
        if (accumulate)
            hipLaunchKernelGGL(d4_stream_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, src, planes, C, H, W, flips,
                               flip_ops, dst, scale, wide);
        else
            hipLaunchKernelGGL(d4_stream_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, src, planes, C, H, W, flips,
                               flip_ops, dst, scale, wide);
    } else {
        // dst is [W][H]: tiles along dst x cover H, along dst y cover W
        const dim3 grid((unsigned)adh_ceil_div(H, D4_TILE), (unsigned)adh_min_i(adh_ceil_div(W, D4_TILE), 65535), gz);
        if (accumulate)
            hipLaunchKernelGGL(d4_transpose_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, src, planes, C, H, W, flips,
                               flip_ops, dst, scale);
        else
            hipLaunchKernelGGL(d4_transpose_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, src, planes, C, H, W, flips,
                               flip_ops, dst, scale);
    }
    return adh_check_launch();
}
