// The device-resident 8-bit dataset cache, gfx950: a split of an image-folder dataset lives on the device as dense
// uint8 [M, H, W, 3], and a training step's input is gathered from it.
//
//   adh_u8_resize_bilinear  cache build, one launch per decoded file: interleaved grey / RGB / RGBA bytes of any size (the
//                           addressing of csrc/image_io.hip) to one dense [OH, OW, 3] slot of the cache.  The source
//                           coordinates are those of adh_bilinear (csrc/pointwise.hip, align_corners false), in the same fp32
//                           arithmetic.  One lane per output pixel, byte accesses: it runs once per file, not per step.
//   adh_batch_from_u8       every step, once per role (hazy, clear): images index[n] of the cache to fp32 [N,3,H,W] planes of
//                           v / 255, with the flips and the ColorJitter of adh_paired_augment (csrc/train_io.hip) when a parameter
//                           row per sample is given.  Without parameters one launch; with them two: the grey mean the contrast
//                           step sees (fixed-order two-stage float64 sum, no atomics), then one gather pass.
//   adh_batch_window_from_u8  the same from a flat cache of images of any sizes: sample n is the CH x CW window whose row y
//                           starts at cache + window[n][0] + y * window[n][1] (a crop of an image at its own resolution; the host
//                           turns image offset, width and crop origin into that pair).  Bit for bit adh_batch_from_u8 on a dense
//                           copy of the window's bytes: the mean pass walks the flat window-pixel number in the same quads, blocks
//                           and lanes, the gather pass is the same kernel with another row address.  A quad's 12 bytes start at
//                           any address there: three aligned dwords, a fourth when the address is off phase, and a funnel shift
//                           (ds_load12), where the cache starts and ends on a multiple of 4; bytes otherwise.
//
// The gather pass is csrc/image_io.hip's u8_to_image_kernel with a source that moves: a lane owns four neighbouring pixels of one
// OUTPUT row, which are four neighbouring pixels of one source row whatever the flips (flip_h reverses their order inside the quad
// and the order of the quads in the row; flip_v picks another row), so the interleaved side is still three whole dwords per lane
// where base, image pitch and W * 3 are multiples of 4, and the planar side one 16-byte store per plane where the output is
// 16-byte aligned and W % 4 == 0.  Everything else goes byte by byte and float by float, so no byte outside an image is read.
// The mean pass reads an image as one flat run of H * W * 3 bytes (a mean does not care about rows), dwords where base and image
// pitch allow.  No LDS beyond the four doubles of the block sum; the gather pass shares nothing between lanes but the butterfly
// that adds the image's partial sums.
#include "common.h"

#define DS_QUAD 4            // pixels per lane
#define DS_ROWS 4            // rows per workgroup of the gather pass (one wave each)
#define DS_WIDE_U8 1         // flags: the gather pass reads dwords
#define DS_WIDE_F32 2        //        and stores float4
#define DS_WIDE_FLAT 4       //        the mean pass reads dwords
#ifndef DS_PIXELS_PER_BLOCK
#define DS_PIXELS_PER_BLOCK (256 * 16)   // mean pass: four quads per lane
#endif
#ifndef DS_MAXBLK
#define DS_MAXBLK 128        // partial sums per image (a 512 x 1024 image has exactly 128 blocks)
#endif
#ifndef DS_MAXBLK_RESIZE
#define DS_MAXBLK_RESIZE 4096
#endif

// v / 255 correctly rounded (csrc/image_io.hip's u8_unit)
__device__ __forceinline__ float ds_unit(uint32_t v) { return (float)v / 255.0f; }

// the 12 bytes at p, any address, as the three dwords an aligned read of them would give: the dword that holds p and the next two,
// a fourth only when p is off phase, shifted together.  No misaligned dword is dereferenced; the last byte touched is that of the
// dword holding p + 11, so the caller needs [p rounded down to 4, p + 12 rounded up to 4) readable.
__device__ __forceinline__ void ds_load12(const uint8_t* __restrict__ p, uint32_t (&w)[3]) {
    const unsigned s = (unsigned)((uintptr_t)p & 3);
    const uint32_t* __restrict__ in = reinterpret_cast<const uint32_t*>(p - s);
    uint32_t d[4];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = in[k];
    if (s != 0) {
        d[3] = in[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = (d[k] >> (8 * s)) | (d[k + 1] << (32 - 8 * s));
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = d[k];
    }
}

// ------------------------------------------------------------------------------------------------ resize
// adh_bilinear's source index for align_corners false (csrc/pointwise.hip bilin_src), the same fp32 operations in the same order
__device__ __forceinline__ void ds_src(int o, int in, int out, int& i0, int& i1, float& l1) {
    const float sc = (float)in / (float)out;
    float src = sc * ((float)o + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    i0 = (int)src;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = src - (float)i0;
}

template <int C>
__global__ __launch_bounds__(256) void u8_resize_kernel(const uint8_t* __restrict__ src, int64_t row_pitch, int H, int W,
                                                        uint8_t* __restrict__ dst, int OH, int OW) {
    const int64_t total = (int64_t)OH * OW;
    for (int64_t t = blockIdx.x * (int64_t)256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int oy = (int)(t / OW), ox = (int)(t - (int64_t)oy * OW);
        int y0, y1, x0, x1;
        float ly, lx;
        ds_src(oy, H, OH, y0, y1, ly);
        ds_src(ox, W, OW, x0, x1, lx);
        const float hy = 1.f - ly, hx = 1.f - lx;
        const uint8_t* __restrict__ r0 = src + (int64_t)y0 * row_pitch;
        const uint8_t* __restrict__ r1 = src + (int64_t)y1 * row_pitch;
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (C == 1 && c > 0) {
                v[c] = v[0];
                continue;
            }
            const float v00 = (float)r0[(int64_t)x0 * C + c], v01 = (float)r0[(int64_t)x1 * C + c];
            const float v10 = (float)r1[(int64_t)x0 * C + c], v11 = (float)r1[(int64_t)x1 * C + c];
            const float r = (v00 * hx + v01 * lx) * hy + (v10 * hx + v11 * lx) * ly;
            v[c] = fminf(fmaxf(rintf(r), 0.f), 255.f);      // halves to even
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[t * 3 + c] = (uint8_t)(int)v[c];
    }
}

extern "C" int adh_u8_resize_bilinear(void* stream, const uint8_t* src, int64_t row_pitch, int H, int W, int C, uint8_t* dst,
                                      int OH, int OW) {
    if (!src || !dst || H < 1 || W < 1 || OH < 1 || OW < 1) return ADH_E_ARG;
    if (C != 1 && C != 3 && C != 4) return ADH_E_ARG;
    if (row_pitch < (int64_t)W * C) return ADH_E_ARG;
    const dim3 grid((unsigned)adh_min_i(adh_ceil_div((int64_t)OH * OW, 256), DS_MAXBLK_RESIZE));
    if (C == 1)
        hipLaunchKernelGGL(u8_resize_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, src, row_pitch, H, W, dst, OH, OW);
    else if (C == 3)
        hipLaunchKernelGGL(u8_resize_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, src, row_pitch, H, W, dst, OH, OW);
    else
        hipLaunchKernelGGL(u8_resize_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, src, row_pitch, H, W, dst, OH, OW);
    return adh_check_launch();
}

// ------------------------------------------------------------------------------------------------ batch assembly
// grey of one pixel as the contrast step of adh_paired_augment sees it (aug_gray_partial_kernel's expression)
__device__ __forceinline__ float ds_gray(float r, float g, float bl, bool bfirst, float b) {
    if (bfirst) {
        r = fminf(fmaxf(b * r, 0.f), 1.f);
        g = fminf(fmaxf(b * g, 0.f), 1.f);
        bl = fminf(fmaxf(b * bl, 0.f), 1.f);
    }
    return 0.2989f * r + 0.587f * g + 0.114f * bl;
}

// partial[n * gridDim.x + blockIdx.x] = this block's share of sum(grey) over image index[n], summed in float64 in an order that
// depends on H * W alone
__global__ __launch_bounds__(256) void batch_gray_partial_kernel(const uint8_t* __restrict__ cache, int64_t image_pitch,
                                                                 const int64_t* __restrict__ index,
                                                                 const float* __restrict__ params, int64_t HW, int flags,
                                                                 double* __restrict__ partial) {
    const int n = blockIdx.y;
    const float* p = params + n * 5;
    const bool bfirst = p[2] != 0.f;
    const float b = p[3];
    const uint8_t* __restrict__ img = cache + index[n] * image_pitch;
    const int64_t nquad = (HW + DS_QUAD - 1) / DS_QUAD;
    double acc = 0.0;
    for (int64_t q = blockIdx.x * (int64_t)256 + threadIdx.x; q < nquad; q += (int64_t)gridDim.x * 256) {
        const int64_t i = q * DS_QUAD;
        const int npx = (HW - i) < DS_QUAD ? (int)(HW - i) : DS_QUAD;
        const uint8_t* __restrict__ in = img + i * 3;
        if (npx == DS_QUAD && (flags & DS_WIDE_FLAT)) {
            uint32_t w[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) w[k] = reinterpret_cast<const uint32_t*>(in)[k];
#pragma unroll
            for (int j = 0; j < DS_QUAD; ++j) {
                float v[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int k = j * 3 + c;
                    v[c] = ds_unit((w[k >> 2] >> ((k & 3) * 8)) & 255u);
                }
                acc += (double)ds_gray(v[0], v[1], v[2], bfirst, b);
            }
        } else {
            for (int j = 0; j < npx; ++j)
                acc += (double)ds_gray(ds_unit(in[j * 3]), ds_unit(in[j * 3 + 1]), ds_unit(in[j * 3 + 2]), bfirst, b);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    __shared__ double s[4];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)n * gridDim.x + blockIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
}

// The same sum over the window window[n] = {byte offset of its first pixel, row pitch}: the flat window-pixel number
// i = y * CW + x is dealt to quads, lanes and blocks exactly as batch_gray_partial_kernel deals the pixels of a dense image, and a
// quad's pixels are added in the same order, so the partials are those of a dense copy of the window, bit for bit.  (y, x) of a
// lane's next quad follow from the grid's stride without a division; a quad that straddles rows takes its pixels one by one.
__global__ __launch_bounds__(256) void window_gray_partial_kernel(const uint8_t* __restrict__ cache,
                                                                  const int64_t* __restrict__ window,
                                                                  const float* __restrict__ params, int CW, int64_t HW, int flags,
                                                                  double* __restrict__ partial) {
    const int n = blockIdx.y;
    const float* p = params + n * 5;
    const bool bfirst = p[2] != 0.f;
    const float b = p[3];
    const uint8_t* __restrict__ win = cache + window[2 * n];
    const int64_t pitch = window[2 * n + 1];
    const int64_t step = (int64_t)gridDim.x * 256 * DS_QUAD;
    const int64_t dy = step / CW;
    const int64_t dx = step - dy * CW;
    int64_t i = (blockIdx.x * (int64_t)256 + threadIdx.x) * DS_QUAD;
    int64_t y = i / CW;
    int64_t x = i - y * CW;                 // 64 bits: x + dx and x + DS_QUAD pass 2^31 for a CW close to it
    double acc = 0.0;
    for (; i < HW; i += step) {
        const int npx = (HW - i) < DS_QUAD ? (int)(HW - i) : DS_QUAD;
        const uint8_t* __restrict__ in = win + y * pitch + x * 3;
        if (npx == DS_QUAD && x + DS_QUAD <= CW && (flags & DS_WIDE_U8)) {
            uint32_t w[3];
            ds_load12(in, w);
#pragma unroll
            for (int j = 0; j < DS_QUAD; ++j) {
                float v[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int k = j * 3 + c;
                    v[c] = ds_unit((w[k >> 2] >> ((k & 3) * 8)) & 255u);
                }
                acc += (double)ds_gray(v[0], v[1], v[2], bfirst, b);
            }
        } else {
            int64_t yy = y, xx = x;
            for (int j = 0; j < npx; ++j, ++xx) {
                while (xx >= CW) xx -= CW, ++yy;
                const uint8_t* __restrict__ px = win + yy * pitch + xx * 3;
                acc += (double)ds_gray(ds_unit(px[0]), ds_unit(px[1]), ds_unit(px[2]), bfirst, b);
            }
        }
        y += dy, x += dx;
        if (x >= CW) x -= CW, ++y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    __shared__ double s[4];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)n * gridDim.x + blockIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
}

// AUG == false: params and partial are not looked at.  WIN == false: where[n] is the number of a dense image, image_pitch bytes
// apart, rows W * 3 bytes apart.  WIN == true: where[n] = {byte offset of the window's first pixel, row pitch}, H x W the window,
// image_pitch unused, and DS_WIDE_U8 means ds_load12 may be used on every whole quad.
template <bool AUG, bool WIN>
__global__ __launch_bounds__(256) void batch_gather_kernel(const uint8_t* __restrict__ cache, int64_t image_pitch,
                                                           const int64_t* __restrict__ where, const float* __restrict__ params,
                                                           const double* __restrict__ partial, int nblk, int H, int W,
                                                           float* __restrict__ out, int flags) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.z;
    const int64_t plane = (int64_t)H * W;
    bool fh = false, fv = false, bfirst = false;
    float b = 1.f, c = 1.f, mean = 0.f;
    if (AUG) {
        const float* p = params + n * 5;
        fh = p[0] != 0.f, fv = p[1] != 0.f, bfirst = p[2] != 0.f;
        b = p[3], c = p[4];
        // every wave sums the image's partials the same way, lane l the blocks l, l + 64, ... and then the butterfly, whose
        // two partners add the same two numbers: one order, the same bits in every lane of every wave (all 64 lanes take part,
        // so this stands before the lanes right of the image leave)
        double m = 0.0;
        for (int i = lane; i < nblk; i += 64) m += partial[(int64_t)n * nblk + i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o, 64);
        mean = (float)(m / (double)plane);
    }
    const int64_t x = ((int64_t)blockIdx.x * 64 + lane) * DS_QUAD;
    if (x >= W) return;
    const int npx = (W - x) < DS_QUAD ? (int)(W - x) : DS_QUAD;
    const uint8_t* __restrict__ img = WIN ? cache + where[2 * n] : cache + where[n] * image_pitch;
    const int64_t row_pitch = WIN ? where[2 * n + 1] : (int64_t)W * 3;
    float* __restrict__ dst = out + (int64_t)n * 3 * plane;
    for (int64_t y = (int64_t)blockIdx.y * DS_ROWS + (threadIdx.x >> 6); y < H; y += (int64_t)gridDim.y * DS_ROWS) {
        const uint8_t* __restrict__ row = img + (fv ? H - 1 - y : y) * row_pitch;
        float v[3][DS_QUAD];
        if (npx == DS_QUAD && (flags & DS_WIDE_U8)) {
            // the four source pixels are neighbours either way; under flip_h they start at W - 4 - x and arrive reversed
            const uint8_t* __restrict__ in = row + (fh ? W - DS_QUAD - x : x) * 3;
            uint32_t w[3];
            if (WIN) {
                ds_load12(in, w);
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) w[k] = reinterpret_cast<const uint32_t*>(in)[k];
            }
            float s[3][DS_QUAD];
#pragma unroll
            for (int j = 0; j < DS_QUAD; ++j)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const int k = j * 3 + ch;
                    s[ch][j] = ds_unit((w[k >> 2] >> ((k & 3) * 8)) & 255u);
                }
#pragma unroll
            for (int j = 0; j < DS_QUAD; ++j)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) v[ch][j] = fh ? s[ch][DS_QUAD - 1 - j] : s[ch][j];
        } else {
#pragma unroll
            for (int j = 0; j < DS_QUAD; ++j) {
                const int64_t sx = fh ? W - 1 - (x + j) : x + j;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) v[ch][j] = (j < npx) ? ds_unit(row[sx * 3 + ch]) : 0.0f;
            }
        }
        if (AUG) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int j = 0; j < DS_QUAD; ++j) {
                    float t = v[ch][j];         // aug_apply_kernel's expressions
                    if (bfirst) {
                        t = fminf(fmaxf(b * t, 0.f), 1.f);
                        t = fminf(fmaxf(c * t + (1.f - c) * mean, 0.f), 1.f);
                    } else {
                        t = fminf(fmaxf(c * t + (1.f - c) * mean, 0.f), 1.f);
                        t = fminf(fmaxf(b * t, 0.f), 1.f);
                    }
                    v[ch][j] = t;
                }
        }
        float* __restrict__ o = dst + y * W + x;
        if (npx == DS_QUAD && (flags & DS_WIDE_F32)) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                f32x4 q;
#pragma unroll
                for (int j = 0; j < DS_QUAD; ++j) q[j] = v[ch][j];
                *reinterpret_cast<f32x4*>(o + ch * plane) = q;
            }
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int j = 0; j < DS_QUAD; ++j)
                    if (j < npx) o[ch * plane + j] = v[ch][j];
        }
    }
}

extern "C" int adh_batch_num_blocks(int64_t HW) {
    return adh_max_i(1, adh_min_i(adh_ceil_div(HW, DS_PIXELS_PER_BLOCK), DS_MAXBLK));
}

extern "C" int adh_batch_from_u8(void* stream, const uint8_t* cache, int64_t image_pitch, int64_t M, int H, int W,
                                 const int64_t* index, const float* params, int N, double* partial, int nblk, float* out_nchw) {
    if (!cache || !index || !out_nchw || (params && !partial)) return ADH_E_ARG;
    if (N < 1 || N > 65535 || H < 1 || W < 1 || M < 1) return ADH_E_ARG;
    const int64_t HW = (int64_t)H * W;
    if (HW > INT64_MAX / 3 || image_pitch < HW * 3 || (M > 1 && image_pitch > INT64_MAX / M)) return ADH_E_ARG;
    if (nblk != adh_batch_num_blocks(HW)) return ADH_E_ARG;
    const bool al4 = ((((uintptr_t)cache) | (uintptr_t)image_pitch) & 3) == 0;
    const int flags = (al4 ? DS_WIDE_FLAT : 0) | ((al4 && (W & 3) == 0) ? DS_WIDE_U8 : 0) |
                      (((((uintptr_t)out_nchw) & 15) == 0 && (W & 3) == 0) ? DS_WIDE_F32 : 0);
    const dim3 grid((unsigned)adh_ceil_div(W, 64 * DS_QUAD), (unsigned)adh_min_i(adh_ceil_div(H, DS_ROWS), 65535), (unsigned)N);
    if (params) {
        hipLaunchKernelGGL(batch_gray_partial_kernel, dim3(nblk, N), dim3(256), 0, (hipStream_t)stream, cache, image_pitch, index,
                           params, HW, flags, partial);
        hipLaunchKernelGGL((batch_gather_kernel<true, false>), grid, dim3(256), 0, (hipStream_t)stream, cache, image_pitch, index, params,
                           partial, nblk, H, W, out_nchw, flags);
    } else {
        hipLaunchKernelGGL((batch_gather_kernel<false, false>), grid, dim3(256), 0, (hipStream_t)stream, cache, image_pitch, index, params,
                           partial, nblk, H, W, out_nchw, flags);
    }
    return adh_check_launch();
}

extern "C" int adh_batch_window_from_u8(void* stream, const uint8_t* cache, int64_t cache_bytes, const int64_t* window,
                                        const float* params, int N, int CH, int CW, double* partial, int nblk, float* out_nchw) {
    if (!cache || !window || !out_nchw || (params && !partial)) return ADH_E_ARG;
    if (N < 1 || N > 65535 || CH < 1 || CW < 1) return ADH_E_ARG;
    const int64_t HW = (int64_t)CH * CW;
    if (HW > INT64_MAX / 3 || cache_bytes < HW * 3) return ADH_E_ARG;
    if (nblk != adh_batch_num_blocks(HW)) return ADH_E_ARG;
    // aligned dwords around any byte of the cache stay inside it when it starts and ends on a multiple of 4
    const bool al4 = ((((uintptr_t)cache) | (uintptr_t)cache_bytes) & 3) == 0;
    const int flags = (al4 ? DS_WIDE_U8 : 0) | (((((uintptr_t)out_nchw) & 15) == 0 && (CW & 3) == 0) ? DS_WIDE_F32 : 0);
    const dim3 grid((unsigned)adh_ceil_div(CW, 64 * DS_QUAD), (unsigned)adh_min_i(adh_ceil_div(CH, DS_ROWS), 65535), (unsigned)N);
    if (params) {
        hipLaunchKernelGGL(window_gray_partial_kernel, dim3(nblk, N), dim3(256), 0, (hipStream_t)stream, cache, window, params, CW,
                           HW, flags, partial);
        hipLaunchKernelGGL((batch_gather_kernel<true, true>), grid, dim3(256), 0, (hipStream_t)stream, cache, (int64_t)0, window,
                           params, partial, nblk, CH, CW, out_nchw, flags);
    } else {
        hipLaunchKernelGGL((batch_gather_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, cache, (int64_t)0, window,
                           params, partial, nblk, CH, CW, out_nchw, flags);
    }
    return adh_check_launch();
}

// ------------------------------------------------------------------------------------------------ depth cache, haze synthesis
//   adh_u16_resize_bilinear  depth-cache build, one launch per file: single-channel 8-bit (v * 257, so v / 255 == v * 257 / 65535)
//                           or 16-bit depth of any size to one dense uint16 [OH, OW] slot, with adh_u8_resize_bilinear's source
//                           coordinates and fp32 arithmetic, rounded half-even and clamped to 0..65535.
//   adh_batch_haze_from_u8  every step for the hazy role when the dataset holds clear images and depth maps: the CH x CW windows
//                           geom[n] of a flat cache of clear RGB bytes, hazed by the scattering model at SOURCE coordinates
//                           (I = J t + A (1 - t), t = exp(-beta d) in float64, one exp per pixel shared by the channels: fog_kernel
//                           of csrc/train_io.hip), then the flips and the ColorJitter of batch_gather_kernel: augment(fog(x)).
//                           d comes from a flat uint16 depth cache (near + (far - near) * u / 65535) or, without one, is fog_kernel's
//                           radial map over the window.  The grey mean of the contrast step is that of the hazed window, so with
//                           parameters it is two launches as above, each of which evaluates the model.
// A lane's four pixels are 12 clear bytes (ds_load12) and 8 depth bytes at an even address: two aligned dwords, or three and a
// funnel shift when the address is 2 mod 4 (hz_load8), where the respective cache starts and ends on a multiple of 4.
#define DS_WIDE_U16 8        // flag: whole quads read their depth as dwords

// the four uint16 at p (p even) as the dwords an aligned read gives; the last byte touched is that of the dword holding p + 7
__device__ __forceinline__ void hz_load8(const uint8_t* __restrict__ p, uint32_t (&u)[DS_QUAD]) {
    const unsigned s = (unsigned)((uintptr_t)p & 2);
    const uint32_t* __restrict__ in = reinterpret_cast<const uint32_t*>(p - s);
    uint32_t w0 = in[0], w1 = in[1];
    if (s != 0) {
        const uint32_t w2 = in[2];
        w0 = (w0 >> 16) | (w1 << 16);
        w1 = (w1 >> 16) | (w2 << 16);
    }
    u[0] = w0 & 0xFFFFu, u[1] = w0 >> 16, u[2] = w1 & 0xFFFFu, u[3] = w1 >> 16;
}

struct hz_ctx {
    double b, A, dnear, span, sx, sy;
};

__device__ __forceinline__ hz_ctx hz_make(const float* __restrict__ fog, int n, double dnear, double dfar, int CH, int CW) {
    hz_ctx k;
    k.b = (double)fog[2 * n], k.A = (double)fog[2 * n + 1];
    k.dnear = dnear, k.span = dfar - dnear;
    k.sx = CW > 1 ? 1.0 / (double)(CW - 1) : 0.0, k.sy = CH > 1 ? 1.0 / (double)(CH - 1) : 0.0;
    return k;
}

// one source pixel (y, x) of the window: bytes rgb, depth level u -> the hazed, clamped fp32 values (fog_kernel's expressions)
template <bool DEPTH>
__device__ __forceinline__ void hz_pixel(const hz_ctx& k, uint32_t r, uint32_t g, uint32_t bl, uint32_t u, int64_t y, int64_t x,
                                         float& hr, float& hg, float& hb) {
    double d;
    if (DEPTH) {
        d = k.dnear + k.span * ((double)u / 65535.0);
    } else {
        const double dx = (double)x * k.sx - 0.5, dy = (double)y * k.sy - 0.2;
        d = 0.3 + 0.7 * sqrt(dx * dx + dy * dy);
    }
    const double t = exp(-k.b * d);
    const double a = k.A * (1.0 - t);
    hr = fminf(fmaxf((float)((double)ds_unit(r) * t + a), 0.f), 1.f);
    hg = fminf(fmaxf((float)((double)ds_unit(g) * t + a), 0.f), 1.f);
    hb = fminf(fmaxf((float)((double)ds_unit(bl) * t + a), 0.f), 1.f);
}

// the pixel at cp / dp, byte by byte (dp is even: one uint16)
template <bool DEPTH>
__device__ __forceinline__ void hz_one(const hz_ctx& k, const uint8_t* __restrict__ cp, const uint8_t* __restrict__ dp, int64_t y,
                                       int64_t x, float& hr, float& hg, float& hb) {
    const uint32_t u = DEPTH ? (uint32_t)*reinterpret_cast<const uint16_t*>(dp) : 0u;
    hz_pixel<DEPTH>(k, cp[0], cp[1], cp[2], u, y, x, hr, hg, hb);
}

// four neighbouring source pixels (y, x .. x + 3) at cp / dp, in source order
template <bool DEPTH>
__device__ __forceinline__ void hz_quad(const hz_ctx& k, const uint8_t* __restrict__ cp, const uint8_t* __restrict__ dp, int flags,
                                        int64_t y, int64_t x, float (&s)[3][DS_QUAD]) {
    uint32_t px[DS_QUAD * 3], u[DS_QUAD] = {0u, 0u, 0u, 0u};
    if (flags & DS_WIDE_U8) {
        uint32_t w[3];
        ds_load12(cp, w);
#pragma unroll
        for (int i = 0; i < DS_QUAD * 3; ++i) px[i] = (w[i >> 2] >> ((i & 3) * 8)) & 255u;
    } else {
#pragma unroll
        for (int i = 0; i < DS_QUAD * 3; ++i) px[i] = cp[i];
    }
    if (DEPTH) {
        if (flags & DS_WIDE_U16) {
            hz_load8(dp, u);
        } else {
#pragma unroll
            for (int j = 0; j < DS_QUAD; ++j) u[j] = reinterpret_cast<const uint16_t*>(dp)[j];
        }
    }
#pragma unroll
    for (int j = 0; j < DS_QUAD; ++j) hz_pixel<DEPTH>(k, px[j * 3], px[j * 3 + 1], px[j * 3 + 2], u[j], y, x + j, s[0][j], s[1][j], s[2][j]);
}

// window_gray_partial_kernel over the hazed window: the same deal of the flat window-pixel number to quads, lanes and blocks and
// the same order of additions, so the partials are those of a dense copy of the window (and of its depth), bit for bit
template <bool DEPTH>
__global__ __launch_bounds__(256) void haze_gray_partial_kernel(const uint8_t* __restrict__ clear, const uint8_t* __restrict__ depth,
                                                                const int64_t* __restrict__ geom, const float* __restrict__ fog,
                                                                double dnear, double dfar, const float* __restrict__ params,
                                                                int CH, int CW, int64_t HW, int flags,
                                                                double* __restrict__ partial) {
    const int n = blockIdx.y;
    const float* p = params + n * 5;
    const bool bfirst = p[2] != 0.f;
    const float b = p[3];
    const hz_ctx k = hz_make(fog, n, dnear, dfar, CH, CW);
    const uint8_t* __restrict__ win = clear + geom[4 * n];
    const int64_t pitch = geom[4 * n + 1];
    const uint8_t* __restrict__ dwin = DEPTH ? depth + geom[4 * n + 2] : nullptr;
    const int64_t dpitch = DEPTH ? geom[4 * n + 3] : 0;
    const int64_t step = (int64_t)gridDim.x * 256 * DS_QUAD;
    const int64_t dy = step / CW;
    const int64_t dx = step - dy * CW;
    int64_t i = (blockIdx.x * (int64_t)256 + threadIdx.x) * DS_QUAD;
    int64_t y = i / CW;
    int64_t x = i - y * CW;
    double acc = 0.0;
    for (; i < HW; i += step) {
        const int npx = (HW - i) < DS_QUAD ? (int)(HW - i) : DS_QUAD;
        if (npx == DS_QUAD && x + DS_QUAD <= CW) {
            float s[3][DS_QUAD];
            hz_quad<DEPTH>(k, win + y * pitch + x * 3, DEPTH ? dwin + y * dpitch + x * 2 : nullptr, flags, y, x, s);
#pragma unroll
            for (int j = 0; j < DS_QUAD; ++j) acc += (double)ds_gray(s[0][j], s[1][j], s[2][j], bfirst, b);
        } else {
            int64_t yy = y, xx = x;
            for (int j = 0; j < npx; ++j, ++xx) {
                while (xx >= CW) xx -= CW, ++yy;
                float hr, hg, hb;
                hz_one<DEPTH>(k, win + yy * pitch + xx * 3, DEPTH ? dwin + yy * dpitch + xx * 2 : nullptr, yy, xx, hr, hg, hb);
                acc += (double)ds_gray(hr, hg, hb, bfirst, b);
            }
        }
        y += dy, x += dx;
        if (x >= CW) x -= CW, ++y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    __shared__ double s4[4];
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)n * gridDim.x + blockIdx.x] = (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

// batch_gather_kernel<AUG, true> with the scattering model between the bytes and the transform: the lane's four output pixels
// are hazed at their source coordinates (row fv ? H - 1 - y : y, columns from fh ? W - 4 - x : x) and arrive reversed under flip_h
template <bool AUG, bool DEPTH>
__global__ __launch_bounds__(256) void haze_gather_kernel(const uint8_t* __restrict__ clear, const uint8_t* __restrict__ depth,
                                                          const int64_t* __restrict__ geom, const float* __restrict__ fog,
                                                          double dnear, double dfar, const float* __restrict__ params,
                                                          const double* __restrict__ partial, int nblk, int H, int W,
                                                          float* __restrict__ out, int flags) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.z;
    const int64_t plane = (int64_t)H * W;
    bool fh = false, fv = false, bfirst = false;
    float b = 1.f, c = 1.f, mean = 0.f;
    if (AUG) {
        const float* p = params + n * 5;
        fh = p[0] != 0.f, fv = p[1] != 0.f, bfirst = p[2] != 0.f;
        b = p[3], c = p[4];
        double m = 0.0;                     // batch_gather_kernel's sum of the partials: one order in every lane of every wave
        for (int i = lane; i < nblk; i += 64) m += partial[(int64_t)n * nblk + i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o, 64);
        mean = (float)(m / (double)plane);
    }
    const int64_t x = ((int64_t)blockIdx.x * 64 + lane) * DS_QUAD;
    if (x >= W) return;
    const int npx = (W - x) < DS_QUAD ? (int)(W - x) : DS_QUAD;
    const hz_ctx k = hz_make(fog, n, dnear, dfar, H, W);
    const uint8_t* __restrict__ img = clear + geom[4 * n];
    const int64_t row_pitch = geom[4 * n + 1];
    const uint8_t* __restrict__ dimg = DEPTH ? depth + geom[4 * n + 2] : nullptr;
    const int64_t dpitch = DEPTH ? geom[4 * n + 3] : 0;
    float* __restrict__ dst = out + (int64_t)n * 3 * plane;
    for (int64_t y = (int64_t)blockIdx.y * DS_ROWS + (threadIdx.x >> 6); y < H; y += (int64_t)gridDim.y * DS_ROWS) {
        const int64_t sy = fv ? H - 1 - y : y;
        const uint8_t* __restrict__ row = img + sy * row_pitch;
        const uint8_t* __restrict__ drow = DEPTH ? dimg + sy * dpitch : nullptr;
        float v[3][DS_QUAD];
        if (npx == DS_QUAD) {
            const int64_t sx = fh ? W - DS_QUAD - x : x;
            float s[3][DS_QUAD];
            hz_quad<DEPTH>(k, row + sx * 3, DEPTH ? drow + sx * 2 : nullptr, flags, sy, sx, s);
#pragma unroll
            for (int j = 0; j < DS_QUAD; ++j)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) v[ch][j] = fh ? s[ch][DS_QUAD - 1 - j] : s[ch][j];
        } else {
#pragma unroll
            for (int j = 0; j < DS_QUAD; ++j) {
                v[0][j] = v[1][j] = v[2][j] = 0.0f;
                if (j < npx) {
                    const int64_t sx = fh ? W - 1 - (x + j) : x + j;
                    hz_one<DEPTH>(k, row + sx * 3, DEPTH ? drow + sx * 2 : nullptr, sy, sx, v[0][j], v[1][j], v[2][j]);
                }
            }
        }
        if (AUG) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int j = 0; j < DS_QUAD; ++j) {
                    float t = v[ch][j];         // aug_apply_kernel's expressions
                    if (bfirst) {
                        t = fminf(fmaxf(b * t, 0.f), 1.f);
                        t = fminf(fmaxf(c * t + (1.f - c) * mean, 0.f), 1.f);
                    } else {
                        t = fminf(fmaxf(c * t + (1.f - c) * mean, 0.f), 1.f);
                        t = fminf(fmaxf(b * t, 0.f), 1.f);
                    }
                    v[ch][j] = t;
                }
        }
        float* __restrict__ o = dst + y * W + x;
        if (npx == DS_QUAD && (flags & DS_WIDE_F32)) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                f32x4 q;
#pragma unroll
                for (int j = 0; j < DS_QUAD; ++j) q[j] = v[ch][j];
                *reinterpret_cast<f32x4*>(o + ch * plane) = q;
            }
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int j = 0; j < DS_QUAD; ++j)
                    if (j < npx) o[ch * plane + j] = v[ch][j];
        }
    }
}

// B: bytes per source pixel.  u8_resize_kernel's arithmetic on one channel of 16-bit levels.
template <int B>
__global__ __launch_bounds__(256) void u16_resize_kernel(const uint8_t* __restrict__ src, int64_t row_pitch, int H, int W,
                                                         uint16_t* __restrict__ dst, int OH, int OW) {
    const int64_t total = (int64_t)OH * OW;
    for (int64_t t = blockIdx.x * (int64_t)256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int oy = (int)(t / OW), ox = (int)(t - (int64_t)oy * OW);
        int y0, y1, x0, x1;
        float ly, lx;
        ds_src(oy, H, OH, y0, y1, ly);
        ds_src(ox, W, OW, x0, x1, lx);
        const float hy = 1.f - ly, hx = 1.f - lx;
        const uint8_t* __restrict__ r0 = src + (int64_t)y0 * row_pitch;
        const uint8_t* __restrict__ r1 = src + (int64_t)y1 * row_pitch;
        float v00, v01, v10, v11;
        if (B == 1) {
            v00 = (float)(r0[x0] * 257u), v01 = (float)(r0[x1] * 257u);
            v10 = (float)(r1[x0] * 257u), v11 = (float)(r1[x1] * 257u);
        } else {
            v00 = (float)reinterpret_cast<const uint16_t*>(r0)[x0], v01 = (float)reinterpret_cast<const uint16_t*>(r0)[x1];
            v10 = (float)reinterpret_cast<const uint16_t*>(r1)[x0], v11 = (float)reinterpret_cast<const uint16_t*>(r1)[x1];
        }
        const float r = (v00 * hx + v01 * lx) * hy + (v10 * hx + v11 * lx) * ly;
        dst[t] = (uint16_t)(int)fminf(fmaxf(rintf(r), 0.f), 65535.f);      // halves to even
    }
}

extern "C" int adh_u16_resize_bilinear(void* stream, const uint8_t* src, int64_t src_pitch_bytes, int h, int w, int bytes_per_px,
                                       void* dst_u16, int OH, int OW) {
    uint16_t* dst = reinterpret_cast<uint16_t*>(dst_u16);
    if (!src || !dst_u16 || h < 1 || w < 1 || OH < 1 || OW < 1) return ADH_E_ARG;
    if (bytes_per_px != 1 && bytes_per_px != 2) return ADH_E_ARG;
    if (src_pitch_bytes < (int64_t)w * bytes_per_px) return ADH_E_ARG;
    if ((uintptr_t)dst_u16 & 1) return ADH_E_ARG;
    if (bytes_per_px == 2 && ((((uintptr_t)src) | (uintptr_t)src_pitch_bytes) & 1)) return ADH_E_ARG;
    const dim3 grid((unsigned)adh_min_i(adh_ceil_div((int64_t)OH * OW, 256), DS_MAXBLK_RESIZE));
    if (bytes_per_px == 1)
        hipLaunchKernelGGL(u16_resize_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, src, src_pitch_bytes, h, w, dst, OH, OW);
    else
        hipLaunchKernelGGL(u16_resize_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, src, src_pitch_bytes, h, w, dst, OH, OW);
    return adh_check_launch();
}

extern "C" int adh_batch_haze_from_u8(void* stream, const uint8_t* clear, int64_t clear_bytes, const void* depth,
                                      int64_t depth_bytes, const int64_t* geom, const float* fog, double depth_near,
                                      double depth_far, const float* params, int N, int CH, int CW, double* partial, int nblk,
                                      float* out_nchw) {
    if (!clear || !geom || !fog || !out_nchw || (params && !partial)) return ADH_E_ARG;
    if (N < 1 || N > 65535 || CH < 1 || CW < 1) return ADH_E_ARG;
    const int64_t HW = (int64_t)CH * CW;
    if (HW > INT64_MAX / 3 || clear_bytes < HW * 3) return ADH_E_ARG;
    if (depth && ((((uintptr_t)depth) & 1) || depth_bytes < HW * 2)) return ADH_E_ARG;
    if (nblk != adh_batch_num_blocks(HW)) return ADH_E_ARG;
    // aligned dwords around any byte of a cache stay inside it when it starts and ends on a multiple of 4
    const bool al4 = ((((uintptr_t)clear) | (uintptr_t)clear_bytes) & 3) == 0;
    const bool dal4 = depth && ((((uintptr_t)depth) | (uintptr_t)depth_bytes) & 3) == 0;
    const int flags = (al4 ? DS_WIDE_U8 : 0) | (dal4 ? DS_WIDE_U16 : 0) |
                      (((((uintptr_t)out_nchw) & 15) == 0 && (CW & 3) == 0) ? DS_WIDE_F32 : 0);
    const uint8_t* dbytes = reinterpret_cast<const uint8_t*>(depth);
    const dim3 grid((unsigned)adh_ceil_div(CW, 64 * DS_QUAD), (unsigned)adh_min_i(adh_ceil_div(CH, DS_ROWS), 65535), (unsigned)N);
#define HZ_LAUNCH(D)                                                                                                              \
    if (params) {                                                                                                                 \
        hipLaunchKernelGGL((haze_gray_partial_kernel<D>), dim3(nblk, N), dim3(256), 0, (hipStream_t)stream, clear, dbytes, geom,  \
                           fog, depth_near, depth_far, params, CH, CW, HW, flags, partial);                                       \
        hipLaunchKernelGGL((haze_gather_kernel<true, D>), grid, dim3(256), 0, (hipStream_t)stream, clear, dbytes, geom, fog,      \
                           depth_near, depth_far, params, partial, nblk, CH, CW, out_nchw, flags);                                \
    } else {                                                                                                                      \
        hipLaunchKernelGGL((haze_gather_kernel<false, D>), grid, dim3(256), 0, (hipStream_t)stream, clear, dbytes, geom, fog,     \
                           depth_near, depth_far, params, partial, nblk, CH, CW, out_nchw, flags);                                \
    }
    if (depth) {
        HZ_LAUNCH(true)
    } else {
        HZ_LAUNCH(false)
    }
#undef HZ_LAUNCH
    return adh_check_launch();
}

// ------------------------------------------------------------------------------------------------ patchy, chromatic haze
//   adh_batch_nhhaze_from_u8  adh_batch_haze_from_u8 with beta_c and A_c per channel and the optical depth scaled per source
//                           pixel by m = 1 + s (2 f - 1), f in [0, 1] a density field anchored to the IMAGE: K octaves of value
//                           noise on an integer-hashed lattice at image coordinates (y + oy, x + ox), evaluated in the lane's
//                           registers (no LDS, no workspace, no launch of its own).
// Octave k: p = (double)coordinate * (f0 2^k) is ONE multiplication and floor(p) the lattice cell, so a host restatement lands in
// the same cells; the corner values are 32-bit hashes / 2^32 (exact), blended by the fade u u (3 - 2 u).  The field's arithmetic
// is compiled with contraction off: every operation is the IEEE one a host restatement performs (a fused p - floor(p) would
// differ from it by the rounding of p, which at coordinates near 2^31 is no small number), and a pixel's value does not depend
// on which path (quad or single) computed it.  The host checks f0 2^(K-1) <= 0.5 and coordinate * f below 2^31.
// The kernels are siblings of haze_gray_partial_kernel / haze_gather_kernel, statement for statement, with nh_quad / nh_one in
// the place of hz_quad / hz_one: the same grid, flags, access paths and deal of pixels.  They are not one template with those,
// because wrapping the old kernels' bodies changed the code the compiler makes for them.
#ifndef NH_SHARE_CORNERS
#define NH_SHARE_CORNERS 1   // 0: every pixel of a quad hashes its own four corners (A/B measurements only)
#endif

struct nh_ctx {
    double b[3], A[3], s, f0;
    int64_t oy, ox;
    uint32_t seed;
    int K;
    bool grey;               // beta_r == beta_g == beta_b: one exp serves the three channels
};

__device__ __forceinline__ nh_ctx nh_make(const float* __restrict__ fog, const double* __restrict__ field, int n) {
    nh_ctx q;
#pragma unroll
    for (int c = 0; c < 3; ++c) q.b[c] = (double)fog[6 * n + c], q.A[c] = (double)fog[6 * n + 3 + c];
    const double* f = field + 6 * n;
    q.seed = (uint32_t)f[0], q.oy = (int64_t)f[1], q.ox = (int64_t)f[2], q.K = (int)f[3];
    q.s = f[4], q.f0 = f[5];
    q.grey = q.b[0] == q.b[1] && q.b[1] == q.b[2];
    return q;
}

// hz_make without beta and A
__device__ __forceinline__ hz_ctx nh_geom(double dnear, double dfar, int CH, int CW) {
    hz_ctx k;
    k.b = 0.0, k.A = 0.0;
    k.dnear = dnear, k.span = dfar - dnear;
    k.sx = CW > 1 ? 1.0 / (double)(CW - 1) : 0.0, k.sy = CH > 1 ? 1.0 / (double)(CH - 1) : 0.0;
    return k;
}

__device__ __forceinline__ uint32_t nh_mix(uint32_t h) {
    h ^= h >> 16, h *= 0x7FEB352Du;
    h ^= h >> 15, h *= 0x846CA68Bu;
    return h ^ (h >> 16);
}

// the hash's share of lattice row iy of octave o, and the lattice value at column ix of that row, in [0, 1)
__device__ __forceinline__ uint32_t nh_row(uint32_t iy, int o, uint32_t seed) {
    return (iy * 0x85EBCA77u) ^ ((uint32_t)o * 0xC2B2AE3Du) ^ seed;
}
__device__ __forceinline__ double nh_value(uint32_t ix, uint32_t row) {
    return (double)nh_mix((ix * 0x9E3779B1u) ^ row) * (1.0 / 4294967296.0);
}

// the field at window pixels (y, x .. x + NPX - 1), NPX = 1 or DS_QUAD.  The pixels share the row and, with the finest cell at
// least 2 pixels wide, start in at most three neighbouring lattice columns: four columns x two rows are hashed once per octave.
template <int NPX>
__device__ __forceinline__ void nh_field(const nh_ctx& q, int64_t y, int64_t x, double (&f)[NPX]) {
#pragma clang fp contract(off)
    constexpr int NCOL = NPX == 1 ? 2 : 4;
    const double Y = (double)(y + q.oy);
    double acc[NPX], norm = 0.0;
#pragma unroll
    for (int j = 0; j < NPX; ++j) acc[j] = 0.0;
    for (int o = 0; o < q.K; ++o) {
        const double fk = q.f0 * (double)(1 << o), wk = 1.0 / (double)(1 << o);
        const double py = Y * fk, fy = floor(py), uy = py - fy;
        const double wy = uy * uy * (3.0 - 2.0 * uy);
        const uint32_t iy = (uint32_t)(int64_t)fy;
        const uint32_t r0 = nh_row(iy, o, q.seed), r1 = nh_row(iy + 1u, o, q.seed);
        const double fx0 = floor((double)(x + q.ox) * fk);
        const uint32_t ix0 = (uint32_t)(int64_t)fx0;
        double top[NCOL], bot[NCOL];
#pragma unroll
        for (int c = 0; c < NCOL; ++c) top[c] = bot[c] = 0.0;
        if (NPX == 1 || NH_SHARE_CORNERS) {
#pragma unroll
            for (int c = 0; c < NCOL; ++c) top[c] = nh_value(ix0 + (uint32_t)c, r0), bot[c] = nh_value(ix0 + (uint32_t)c, r1);
        }
#pragma unroll
        for (int j = 0; j < NPX; ++j) {
            const double px = (double)(x + q.ox + j) * fk, fx = floor(px), ux = px - fx;
            const double wx = ux * ux * (3.0 - 2.0 * ux);
            double v00, v01, v10, v11;
            if (NPX == 1) {
                v00 = top[0], v01 = top[1], v10 = bot[0], v11 = bot[1];
            } else if (NH_SHARE_CORNERS) {
                const int c = (int)(fx - fx0);                 // 0, 1 or 2; selects: a runtime index would put the arrays in scratch
                v00 = c == 0 ? top[0] : c == 1 ? top[1] : top[NCOL - 2];
                v01 = c == 0 ? top[1] : c == 1 ? top[NCOL - 2] : top[NCOL - 1];
                v10 = c == 0 ? bot[0] : c == 1 ? bot[1] : bot[NCOL - 2];
                v11 = c == 0 ? bot[1] : c == 1 ? bot[NCOL - 2] : bot[NCOL - 1];
            } else {
                const uint32_t ix = (uint32_t)(int64_t)fx;
                v00 = nh_value(ix, r0), v01 = nh_value(ix + 1u, r0), v10 = nh_value(ix, r1), v11 = nh_value(ix + 1u, r1);
            }
            const double t = v00 + wx * (v01 - v00), b = v10 + wx * (v11 - v10);
            acc[j] = acc[j] + wk * (t + wy * (b - t));
        }
        norm = norm + wk;
    }
#pragma unroll
    for (int j = 0; j < NPX; ++j) f[j] = acc[j] / norm;
}

// hz_pixel under the non-uniform model: field value f, beta and A per channel, the same expressions otherwise
template <bool DEPTH>
__device__ __forceinline__ void nh_pixel(const hz_ctx& k, const nh_ctx& q, double f, uint32_t r, uint32_t g, uint32_t bl, uint32_t u,
                                         int64_t y, int64_t x, float& hr, float& hg, float& hb) {
    double d;
    if (DEPTH) {
        d = k.dnear + k.span * ((double)u / 65535.0);
    } else {
        const double dx = (double)x * k.sx - 0.5, dy = (double)y * k.sy - 0.2;
        d = 0.3 + 0.7 * sqrt(dx * dx + dy * dy);
    }
    double bm[3];
    {
#pragma clang fp contract(off)
        const double m = 1.0 + q.s * (2.0 * f - 1.0);
#pragma unroll
        for (int c = 0; c < 3; ++c) bm[c] = q.b[c] * m;
    }
    double t[3];
    t[0] = exp(-bm[0] * d);
    if (q.grey) {
        t[1] = t[2] = t[0];
    } else {
        t[1] = exp(-bm[1] * d);
        t[2] = exp(-bm[2] * d);
    }
    const double a0 = q.A[0] * (1.0 - t[0]), a1 = q.A[1] * (1.0 - t[1]), a2 = q.A[2] * (1.0 - t[2]);
    hr = fminf(fmaxf((float)((double)ds_unit(r) * t[0] + a0), 0.f), 1.f);
    hg = fminf(fmaxf((float)((double)ds_unit(g) * t[1] + a1), 0.f), 1.f);
    hb = fminf(fmaxf((float)((double)ds_unit(bl) * t[2] + a2), 0.f), 1.f);
}

// hz_one
template <bool DEPTH>
__device__ __forceinline__ void nh_one(const hz_ctx& k, const nh_ctx& q, const uint8_t* __restrict__ cp,
                                       const uint8_t* __restrict__ dp, int64_t y, int64_t x, float& hr, float& hg, float& hb) {
    const uint32_t u = DEPTH ? (uint32_t)*reinterpret_cast<const uint16_t*>(dp) : 0u;
    double f[1];
    nh_field<1>(q, y, x, f);
    nh_pixel<DEPTH>(k, q, f[0], cp[0], cp[1], cp[2], u, y, x, hr, hg, hb);
}

// hz_quad: its access paths, then the field of the four pixels at once
template <bool DEPTH>
__device__ __forceinline__ void nh_quad(const hz_ctx& k, const nh_ctx& q, const uint8_t* __restrict__ cp,
                                        const uint8_t* __restrict__ dp, int flags, int64_t y, int64_t x, float (&s)[3][DS_QUAD]) {
    uint32_t px[DS_QUAD * 3], u[DS_QUAD] = {0u, 0u, 0u, 0u};
    if (flags & DS_WIDE_U8) {
        uint32_t w[3];
        ds_load12(cp, w);
#pragma unroll
        for (int i = 0; i < DS_QUAD * 3; ++i) px[i] = (w[i >> 2] >> ((i & 3) * 8)) & 255u;
    } else {
#pragma unroll
        for (int i = 0; i < DS_QUAD * 3; ++i) px[i] = cp[i];
    }
    if (DEPTH) {
        if (flags & DS_WIDE_U16) {
            hz_load8(dp, u);
        } else {
#pragma unroll
            for (int j = 0; j < DS_QUAD; ++j) u[j] = reinterpret_cast<const uint16_t*>(dp)[j];
        }
    }
    double f[DS_QUAD];
    nh_field<DS_QUAD>(q, y, x, f);
#pragma unroll
    for (int j = 0; j < DS_QUAD; ++j)
        nh_pixel<DEPTH>(k, q, f[j], px[j * 3], px[j * 3 + 1], px[j * 3 + 2], u[j], y, x + j, s[0][j], s[1][j], s[2][j]);
}

// haze_gray_partial_kernel
template <bool DEPTH>
__global__ __launch_bounds__(256) void nhhaze_gray_partial_kernel(const uint8_t* __restrict__ clear, const uint8_t* __restrict__ depth,
                                                                  const int64_t* __restrict__ geom, const float* __restrict__ fog,
                                                                  const double* __restrict__ field, double dnear, double dfar,
                                                                  const float* __restrict__ params, int CH, int CW, int64_t HW,
                                                                  int flags, double* __restrict__ partial) {
    const int n = blockIdx.y;
    const float* p = params + n * 5;
    const bool bfirst = p[2] != 0.f;
    const float b = p[3];
    const hz_ctx k = nh_geom(dnear, dfar, CH, CW);
    const nh_ctx q = nh_make(fog, field, n);
    const uint8_t* __restrict__ win = clear + geom[4 * n];
    const int64_t pitch = geom[4 * n + 1];
    const uint8_t* __restrict__ dwin = DEPTH ? depth + geom[4 * n + 2] : nullptr;
    const int64_t dpitch = DEPTH ? geom[4 * n + 3] : 0;
    const int64_t step = (int64_t)gridDim.x * 256 * DS_QUAD;
    const int64_t dy = step / CW;
    const int64_t dx = step - dy * CW;
    int64_t i = (blockIdx.x * (int64_t)256 + threadIdx.x) * DS_QUAD;
    int64_t y = i / CW;
    int64_t x = i - y * CW;
    double acc = 0.0;
    for (; i < HW; i += step) {
        const int npx = (HW - i) < DS_QUAD ? (int)(HW - i) : DS_QUAD;
        if (npx == DS_QUAD && x + DS_QUAD <= CW) {
            float s[3][DS_QUAD];
            nh_quad<DEPTH>(k, q, win + y * pitch + x * 3, DEPTH ? dwin + y * dpitch + x * 2 : nullptr, flags, y, x, s);
#pragma unroll
            for (int j = 0; j < DS_QUAD; ++j) acc += (double)ds_gray(s[0][j], s[1][j], s[2][j], bfirst, b);
        } else {
            int64_t yy = y, xx = x;
            for (int j = 0; j < npx; ++j, ++xx) {
                while (xx >= CW) xx -= CW, ++yy;
                float hr, hg, hb;
                nh_one<DEPTH>(k, q, win + yy * pitch + xx * 3, DEPTH ? dwin + yy * dpitch + xx * 2 : nullptr, yy, xx, hr, hg, hb);
                acc += (double)ds_gray(hr, hg, hb, bfirst, b);
            }
        }
        y += dy, x += dx;
        if (x >= CW) x -= CW, ++y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    __shared__ double s4[4];
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)n * gridDim.x + blockIdx.x] = (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

// haze_gather_kernel
template <bool AUG, bool DEPTH>
__global__ __launch_bounds__(256) void nhhaze_gather_kernel(const uint8_t* __restrict__ clear, const uint8_t* __restrict__ depth,
                                                            const int64_t* __restrict__ geom, const float* __restrict__ fog,
                                                            const double* __restrict__ field, double dnear, double dfar,
                                                            const float* __restrict__ params, const double* __restrict__ partial,
                                                            int nblk, int H, int W, float* __restrict__ out, int flags) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.z;
    const int64_t plane = (int64_t)H * W;
    bool fh = false, fv = false, bfirst = false;
    float b = 1.f, c = 1.f, mean = 0.f;
    if (AUG) {
        const float* p = params + n * 5;
        fh = p[0] != 0.f, fv = p[1] != 0.f, bfirst = p[2] != 0.f;
        b = p[3], c = p[4];
        double m = 0.0;                     // batch_gather_kernel's sum of the partials: one order in every lane of every wave
        for (int i = lane; i < nblk; i += 64) m += partial[(int64_t)n * nblk + i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o, 64);
        mean = (float)(m / (double)plane);
    }
    const int64_t x = ((int64_t)blockIdx.x * 64 + lane) * DS_QUAD;
    if (x >= W) return;
    const int npx = (W - x) < DS_QUAD ? (int)(W - x) : DS_QUAD;
    const hz_ctx k = nh_geom(dnear, dfar, H, W);
    const nh_ctx q = nh_make(fog, field, n);
    const uint8_t* __restrict__ img = clear + geom[4 * n];
    const int64_t row_pitch = geom[4 * n + 1];
    const uint8_t* __restrict__ dimg = DEPTH ? depth + geom[4 * n + 2] : nullptr;
    const int64_t dpitch = DEPTH ? geom[4 * n + 3] : 0;
    float* __restrict__ dst = out + (int64_t)n * 3 * plane;
    for (int64_t y = (int64_t)blockIdx.y * DS_ROWS + (threadIdx.x >> 6); y < H; y += (int64_t)gridDim.y * DS_ROWS) {
        const int64_t sy = fv ? H - 1 - y : y;
        const uint8_t* __restrict__ row = img + sy * row_pitch;
        const uint8_t* __restrict__ drow = DEPTH ? dimg + sy * dpitch : nullptr;
        float v[3][DS_QUAD];
        if (npx == DS_QUAD) {
            const int64_t sx = fh ? W - DS_QUAD - x : x;
            float s[3][DS_QUAD];
            nh_quad<DEPTH>(k, q, row + sx * 3, DEPTH ? drow + sx * 2 : nullptr, flags, sy, sx, s);
#pragma unroll
            for (int j = 0; j < DS_QUAD; ++j)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) v[ch][j] = fh ? s[ch][DS_QUAD - 1 - j] : s[ch][j];
        } else {
#pragma unroll
            for (int j = 0; j < DS_QUAD; ++j) {
                v[0][j] = v[1][j] = v[2][j] = 0.0f;
                if (j < npx) {
                    const int64_t sx = fh ? W - 1 - (x + j) : x + j;
                    nh_one<DEPTH>(k, q, row + sx * 3, DEPTH ? drow + sx * 2 : nullptr, sy, sx, v[0][j], v[1][j], v[2][j]);
                }
            }
        }
        if (AUG) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int j = 0; j < DS_QUAD; ++j) {
                    float t = v[ch][j];         // aug_apply_kernel's expressions
                    if (bfirst) {
                        t = fminf(fmaxf(b * t, 0.f), 1.f);
                        t = fminf(fmaxf(c * t + (1.f - c) * mean, 0.f), 1.f);
                    } else {
                        t = fminf(fmaxf(c * t + (1.f - c) * mean, 0.f), 1.f);
                        t = fminf(fmaxf(b * t, 0.f), 1.f);
                    }
                    v[ch][j] = t;
                }
        }
        float* __restrict__ o = dst + y * W + x;
        if (npx == DS_QUAD && (flags & DS_WIDE_F32)) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                f32x4 q4;
#pragma unroll
                for (int j = 0; j < DS_QUAD; ++j) q4[j] = v[ch][j];
                *reinterpret_cast<f32x4*>(o + ch * plane) = q4;
            }
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int j = 0; j < DS_QUAD; ++j)
                    if (j < npx) o[ch * plane + j] = v[ch][j];
        }
    }
}

// fog [N,6] = {beta_r beta_g beta_b A_r A_g A_b}, field [N,6] (doubles) = {seed, oy, ox, K, s, f0}: adh_batch_haze_from_u8's
// checks, flags, grid and launches.  Neither geom nor field is validated on the device.
extern "C" int adh_batch_nhhaze_from_u8(void* stream, const uint8_t* clear, int64_t clear_bytes, const void* depth,
                                        int64_t depth_bytes, const int64_t* geom, const float* fog, const double* field,
                                        double depth_near, double depth_far, const float* params, int N, int CH, int CW,
                                        double* partial, int nblk, float* out_nchw) {
    if (!clear || !geom || !fog || !field || !out_nchw || (params && !partial)) return ADH_E_ARG;
    if (N < 1 || N > 65535 || CH < 1 || CW < 1) return ADH_E_ARG;
    const int64_t HW = (int64_t)CH * CW;
    if (HW > INT64_MAX / 3 || clear_bytes < HW * 3) return ADH_E_ARG;
    if (depth && ((((uintptr_t)depth) & 1) || depth_bytes < HW * 2)) return ADH_E_ARG;
    if (nblk != adh_batch_num_blocks(HW)) return ADH_E_ARG;
    const bool al4 = ((((uintptr_t)clear) | (uintptr_t)clear_bytes) & 3) == 0;
    const bool dal4 = depth && ((((uintptr_t)depth) | (uintptr_t)depth_bytes) & 3) == 0;
    const int flags = (al4 ? DS_WIDE_U8 : 0) | (dal4 ? DS_WIDE_U16 : 0) |
                      (((((uintptr_t)out_nchw) & 15) == 0 && (CW & 3) == 0) ? DS_WIDE_F32 : 0);
    const uint8_t* dbytes = reinterpret_cast<const uint8_t*>(depth);
    const dim3 grid((unsigned)adh_ceil_div(CW, 64 * DS_QUAD), (unsigned)adh_min_i(adh_ceil_div(CH, DS_ROWS), 65535), (unsigned)N);
#define NH_LAUNCH(D)                                                                                                              \
    if (params) {                                                                                                                 \
        hipLaunchKernelGGL((nhhaze_gray_partial_kernel<D>), dim3(nblk, N), dim3(256), 0, (hipStream_t)stream, clear, dbytes,      \
                           geom, fog, field, depth_near, depth_far, params, CH, CW, HW, flags, partial);                          \
        hipLaunchKernelGGL((nhhaze_gather_kernel<true, D>), grid, dim3(256), 0, (hipStream_t)stream, clear, dbytes, geom, fog,    \
                           field, depth_near, depth_far, params, partial, nblk, CH, CW, out_nchw, flags);                         \
    } else {                                                                                                                      \
        hipLaunchKernelGGL((nhhaze_gather_kernel<false, D>), grid, dim3(256), 0, (hipStream_t)stream, clear, dbytes, geom, fog,   \
                           field, depth_near, depth_far, params, partial, nblk, CH, CW, out_nchw, flags);                         \
    }
    if (depth) {
        NH_LAUNCH(true)
    } else {
        NH_LAUNCH(false)
    }
#undef NH_LAUNCH
    return adh_check_launch();
}
