// 8-bit image files in and out of the fp32 planes the branches work on, gfx950: interleaved rows of bytes (what an image decoder
// hands over: grey, RGB or RGBA, rows `row_pitch` bytes apart, images `image_pitch` bytes apart, any base alignment) to dense
// [N,3,H,W] in [0,1] and back.  Pure streaming kernels, one launch per batch, no LDS, nothing shared between lanes.
//
// A lane owns four neighbouring pixels of one row.  On the planar side that is one 16-byte access per plane where the tensor
// allows it (base 16-byte aligned and W % 4 == 0, so every quad of every row and plane is aligned).  On the interleaved side the
// quad is C whole dwords where base, row pitch and image pitch are all multiples of 4 (a quad starts 4 C bytes into its row);
// both decisions are made once per launch on the host.  Everything else -- an unaligned base (a crop, the right pane of a
// panel), an odd pitch, the last quad of a row whose width is no multiple of 4 -- goes byte by byte and pixel by pixel, so that
// no byte outside the W * C run of a row is ever read or written.  A workgroup is four waves on four rows; the grid walks the
// quads in x, the rows in y and the images in z, and loops where H or N exceed what a grid dimension holds.
#include "common.h"

#define IMG_QUAD 4      // pixels per lane
#define IMG_ROWS 4      // rows per workgroup (one wave each)
#define IMG_WIDE_U8 1   // flags: the interleaved side moves dwords
#define IMG_WIDE_F32 2  //        the planar side moves float4

// v / 255 correctly rounded: a product with a rounded reciprocal differs for some of the 256 values
__device__ __forceinline__ float u8_unit(uint32_t v) { return (float)v / 255.0f; }

// rint(min(max(x, 0), 1) * 255): the comparison is false for NaN, quiet or signalling, which so becomes 0 like every x <= 0; the
// product is rounded once on its own (__fmul_rn is never contracted) and rintf rounds halves to even
__device__ __forceinline__ uint32_t unit_u8(float x) {
    return (uint32_t)(int)rintf(__fmul_rn(x > 0.0f ? fminf(x, 1.0f) : 0.0f, 255.0f));
}

template <int C>
__global__ __launch_bounds__(256) void u8_to_image_kernel(const uint8_t* __restrict__ src, int64_t row_pitch, int64_t image_pitch,
                                                          int N, int H, int W, float* __restrict__ dst, int flags) {
    const int64_t x = ((int64_t)blockIdx.x * 64 + (threadIdx.x & 63)) * IMG_QUAD;
    if (x >= W) return;
    const int npx = (W - x) < IMG_QUAD ? (int)(W - x) : IMG_QUAD;
    const int64_t plane = (int64_t)H * W;
    for (int64_t n = blockIdx.z; n < N; n += gridDim.z)
        for (int64_t y = (int64_t)blockIdx.y * IMG_ROWS + (threadIdx.x >> 6); y < H; y += (int64_t)gridDim.y * IMG_ROWS) {
            const uint8_t* __restrict__ in = src + n * image_pitch + y * row_pitch + x * C;
            float* __restrict__ out = dst + n * 3 * plane + y * W + x;
            float v[3][IMG_QUAD];
            if (npx == IMG_QUAD && (flags & IMG_WIDE_U8)) {
                uint32_t w[C];
#pragma unroll
                for (int k = 0; k < C; ++k) w[k] = reinterpret_cast<const uint32_t*>(in)[k];
#pragma unroll
                for (int j = 0; j < IMG_QUAD; ++j)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int b = j * C + (C == 1 ? 0 : c);
                        v[c][j] = (C == 1 && c > 0) ? v[0][j] : u8_unit((w[b >> 2] >> ((b & 3) * 8)) & 255u);
                    }
            } else {
#pragma unroll
                for (int j = 0; j < IMG_QUAD; ++j)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        v[c][j] = (j >= npx) ? 0.0f : (C == 1 && c > 0) ? v[0][j] : u8_unit(in[j * C + (C == 1 ? 0 : c)]);
            }
            if (npx == IMG_QUAD && (flags & IMG_WIDE_F32)) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    f32x4 q;
#pragma unroll
                    for (int j = 0; j < IMG_QUAD; ++j) q[j] = v[c][j];
                    *reinterpret_cast<f32x4*>(out + c * plane) = q;
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int j = 0; j < IMG_QUAD; ++j)
                        if (j < npx) out[c * plane + j] = v[c][j];
            }
        }
}

template <int C>
__global__ __launch_bounds__(256) void image_to_u8_kernel(const float* __restrict__ src, int N, int H, int W,
                                                          uint8_t* __restrict__ dst, int64_t row_pitch, int64_t image_pitch,
                                                          int flags) {
    const int64_t x = ((int64_t)blockIdx.x * 64 + (threadIdx.x & 63)) * IMG_QUAD;
    if (x >= W) return;
    const int npx = (W - x) < IMG_QUAD ? (int)(W - x) : IMG_QUAD;
    const int64_t plane = (int64_t)H * W;
    for (int64_t n = blockIdx.z; n < N; n += gridDim.z)
        for (int64_t y = (int64_t)blockIdx.y * IMG_ROWS + (threadIdx.x >> 6); y < H; y += (int64_t)gridDim.y * IMG_ROWS) {
            const float* __restrict__ in = src + n * 3 * plane + y * W + x;
            uint8_t* __restrict__ out = dst + n * image_pitch + y * row_pitch + x * C;
            uint32_t q[IMG_QUAD][4];        // [pixel][channel] as the bytes lie in memory; channel 3 is the alpha of C == 4
            if (npx == IMG_QUAD && (flags & IMG_WIDE_F32)) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const f32x4 p = *reinterpret_cast<const f32x4*>(in + c * plane);
#pragma unroll
                    for (int j = 0; j < IMG_QUAD; ++j) q[j][c] = unit_u8(p[j]);
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int j = 0; j < IMG_QUAD; ++j) q[j][c] = (j < npx) ? unit_u8(in[c * plane + j]) : 0u;
            }
#pragma unroll
            for (int j = 0; j < IMG_QUAD; ++j) q[j][3] = 255u;
            if (npx == IMG_QUAD && (flags & IMG_WIDE_U8)) {
#pragma unroll
                for (int k = 0; k < C; ++k) {
                    uint32_t w = 0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int b = k * 4 + i;
                        w |= q[b / C][b % C] << (i * 8);
                    }
                    reinterpret_cast<uint32_t*>(out)[k] = w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < IMG_QUAD; ++j)
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        if (j < npx) out[j * C + c] = (uint8_t)q[j][c];
            }
        }
}

// the checks both entry points share; on success the launch grid and the two width flags
static int image_io_plan(const void* u8, int64_t row_pitch, int64_t image_pitch, int N, int H, int W, int C, const void* f32,
                         dim3* grid, int* flags) {
    if (!u8 || !f32 || N <= 0 || H <= 0 || W <= 0) return ADH_E_ARG;
    if (row_pitch < (int64_t)W * C) return ADH_E_ARG;
    if (N > 1 && (row_pitch > INT64_MAX / H || image_pitch < (int64_t)H * row_pitch)) return ADH_E_ARG;
    const int64_t step = N > 1 ? image_pitch : 0;
    *flags = (((((uintptr_t)u8) | (uintptr_t)row_pitch | (uintptr_t)step) & 3) == 0 ? IMG_WIDE_U8 : 0) |
             (((((uintptr_t)f32) & 15) == 0 && (W & 3) == 0) ? IMG_WIDE_F32 : 0);
    *grid = dim3((unsigned)adh_ceil_div(W, 64 * IMG_QUAD), (unsigned)adh_min_i(adh_ceil_div(H, IMG_ROWS), 65535),
                 (unsigned)adh_min_i(N, 65535));
    return ADH_OK;
}

extern "C" int adh_u8_to_image(void* stream, const uint8_t* src, int64_t row_pitch, int64_t image_pitch, int N, int H, int W,
                               int C, float* dst_nchw) {
    if (C != 1 && C != 3 && C != 4) return ADH_E_ARG;
    dim3 grid;
    int flags;
    const int rc = image_io_plan(src, row_pitch, image_pitch, N, H, W, C, dst_nchw, &grid, &flags);
    if (rc != ADH_OK) return rc;
    if (C == 1)
        hipLaunchKernelGGL(u8_to_image_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, src, row_pitch, image_pitch, N, H, W,
                           dst_nchw, flags);
    else if (C == 3)
        hipLaunchKernelGGL(u8_to_image_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, src, row_pitch, image_pitch, N, H, W,
                           dst_nchw, flags);
    else
        hipLaunchKernelGGL(u8_to_image_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, src, row_pitch, image_pitch, N, H, W,
                           dst_nchw, flags);
    return adh_check_launch();
}

extern "C" int adh_image_to_u8(void* stream, const float* src_nchw, int N, int H, int W, uint8_t* dst, int64_t row_pitch,
                               int64_t image_pitch, int C) {
    if (C != 3 && C != 4) return ADH_E_ARG;
    dim3 grid;
    int flags;
    const int rc = image_io_plan(dst, row_pitch, image_pitch, N, H, W, C, src_nchw, &grid, &flags);
    if (rc != ADH_OK) return rc;
    if (C == 3)
        hipLaunchKernelGGL(image_to_u8_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, src_nchw, N, H, W, dst, row_pitch,
                           image_pitch, flags);
    else
        hipLaunchKernelGGL(image_to_u8_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, src_nchw, N, H, W, dst, row_pitch,
                           image_pitch, flags);
    return adh_check_launch();
}
