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
