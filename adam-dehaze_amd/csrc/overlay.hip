// Detection overlays on the 8-bit interleaved image adh_image_to_u8 writes, gfx950: box outlines and caption tags drawn in
// place, one launch per batch.  The addressing contract is image_io.hip's: pixel (n, y, x) is the C bytes at
// img + n * image_pitch + y * row_pitch + x * C, C is 3 or 4, the base may have any alignment (one pane of a panel is a pointer
// offset), and with C == 4 the alpha byte is never touched.  A byte of a pixel that no box covers is neither read nor written.
//
// Definition (the contract; tests/_overlay_ref.py restates it per pixel in numpy).  After one floorf / ceilf per coordinate
// everything is integer arithmetic, so the bytes are reproducible exactly.
//   box      x_lo = clamp(floor(x1), 0, W-1), x_hi = clamp(ceil(x2) - 1, 0, W-1), y the same with H.  A box with a coordinate
//            that is not finite, or with x2 <= x1 or y2 <= y1, is skipped.
//   outline  the pixels of [x_lo..x_hi] x [y_lo..y_hi] that are not in [x_lo+t..x_hi-t] x [y_lo+t..y_hi-t], t = thickness: a box
//            narrower than 2 t is filled.
//   tag      len = the number of leading non-negative entries of the box's text row (0: no tag; a null text reads as T = 0).
//            Columns x_lo .. min(x_lo + scale (6 len + 1) - 1, W-1); rows y_lo - 9 scale .. y_lo - 1 where y_lo - 9 scale >= 0,
//            else y_lo .. min(y_lo + 9 scale - 1, H-1); row0 is the first of them.  With u = (x - x_lo - scale) / scale and
//            v = (y - row0 - scale) / scale (both numerators >= 0), the pixel is a glyph pixel when k = u / 6 < len, u % 6 < 5,
//            v < 7, text[k] < G and bit 4 - u % 6 of glyphs[text[k]][v] is set.
//   layers   per pixel, the boxes of its image in list order: the first box whose tag or outline holds the pixel decides it.
//            Inside a tag it is opaque, the text colour on a glyph pixel and the box colour elsewhere; on an outline it is
//            out = (alpha c + (255 - alpha) old + 127) / 255 per channel, in integers.
//
// A workgroup owns a tile of OVL_TW x OVL_TH pixels: 64 lanes along x, so that a wave's stores to a horizontal edge or a tag are
// one contiguous run of 64 C bytes, and four waves on four rows, four passes down the tile.  Outlines are a few pixels thick, so
// most tiles of a frame hold nothing: the workgroup first culls the image's boxes against its tile, OVL_CHUNK at a time, one
// box per thread -- coordinates to integers, the tag's rectangle, and the test "the tag meets the tile, or the outer rectangle
// meets it and the tile does not lie wholly in the inner one" -- and compacts the survivors into an LDS list in list order
// (a ballot per wave, the four masks through LDS).  A tile without survivors goes on to the next chunk, or returns, without
// touching the image.  Otherwise every pixel walks the survivors until one decides it; a pixel decided in one chunk is out of
// the walk of the later ones, so chunks preserve the order too.  The cost follows the covered area (plus one cull per tile and
// chunk), not H * W * M.  Every lane of a wave reads the same list entry: LDS broadcasts, no bank conflicts.  The list is
// 13 x 256 ints and the four masks, 13,344 bytes, so LDS allows the eight workgroups that fill a CU's 32 wave slots.  Stores are
// byte stores at any alignment; a pixel is written by the one lane that owns it, so nothing is atomic and the result does not
// depend on the launch geometry.  With alpha == 255 an outline pixel is not read.  Tile rows ride on grid y and images on grid z, both looped
// where the count exceeds 65,535; addresses are 64-bit.
#include "common.h"

#define OVL_TW 64                        // tile width: one lane per pixel
#define OVL_TH 16                        // tile height
#define OVL_ROWS 4                       // waves per workgroup, one row each per pass
#define OVL_PER (OVL_TH / OVL_ROWS)      // passes: pixels per lane
#define OVL_CHUNK 256                    // boxes culled at a time, one per thread: the capacity of the LDS list
#ifndef OVL_MAX_GRID                     // (the host-emulation build sets it small, so that the row and image loops run)
#define OVL_MAX_GRID 65535
#endif

// a float that holds an integer (a floorf / ceilf result) plus `add`, clamped to [0, hi]: in float64, where both are exact
__device__ __forceinline__ int ovl_clamp(float f, double add, int hi) {
    const double d = (double)f + add;
    return d <= 0.0 ? 0 : d >= (double)hi ? hi : (int)d;
}

__global__ __launch_bounds__(256) void draw_boxes_kernel(uint8_t* __restrict__ img, int64_t row_pitch, int64_t image_pitch, int N,
                                                         int H, int W, int C, const int32_t* __restrict__ first, int M,
                                                         const float* __restrict__ boxes, const uint8_t* __restrict__ colors,
                                                         const int8_t* __restrict__ text, int T,
                                                         const uint8_t* __restrict__ glyphs, int G, int thickness, int scale,
                                                         int alpha) {
    // the survivors of a chunk: outer rectangle, inner rectangle, the tag's last column and its rows (ty1 < ty0: no tag), the
    // caption's length, the box's index
    __shared__ int s_ox0[OVL_CHUNK], s_ox1[OVL_CHUNK], s_oy0[OVL_CHUNK], s_oy1[OVL_CHUNK];
    __shared__ int s_ix0[OVL_CHUNK], s_ix1[OVL_CHUNK], s_iy0[OVL_CHUNK], s_iy1[OVL_CHUNK];
    __shared__ int s_tx1[OVL_CHUNK], s_ty0[OVL_CHUNK], s_ty1[OVL_CHUNK], s_len[OVL_CHUNK], s_idx[OVL_CHUNK];
    __shared__ unsigned long long s_mask[OVL_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int X0 = (int)blockIdx.x * OVL_TW;                               // the grid's x covers W exactly: X0 < W
    const int X1 = (W - 1 - X0 < OVL_TW - 1) ? W - 1 : X0 + OVL_TW - 1;
    const bool x_in = lane <= X1 - X0;
    const int x = X0 + (x_in ? lane : 0);
    const int tiles_y = (H - 1) / OVL_TH + 1;
    const int64_t th9 = 9 * (int64_t)scale;
    for (int64_t n = blockIdx.z; n < N; n += gridDim.z) {
        const int f0 = first[n], f1 = first[n + 1];
        const int b0 = f0 < 0 ? 0 : f0 > M ? M : f0, b1 = f1 < 0 ? 0 : f1 > M ? M : f1;
        uint8_t* __restrict__ base = img + n * image_pitch;
        for (int ty = blockIdx.y; ty < tiles_y; ty += gridDim.y) {
            const int Y0 = ty * OVL_TH;
            const int Y1 = (H - 1 - Y0 < OVL_TH - 1) ? H - 1 : Y0 + OVL_TH - 1;
            unsigned todo = 0;                                             // bit j: the lane's pixel of pass j is undecided
#pragma unroll
            for (int j = 0; j < OVL_PER; ++j)
                if (x_in && wave + j * OVL_ROWS <= Y1 - Y0) todo |= 1u << j;
            for (int64_t c0 = b0; c0 < b1; c0 += OVL_CHUNK) {
                // ---- cull: box c0 + thread against the tile
                const int64_t m = c0 + threadIdx.x;
                bool hit = false;
                int ox0 = 0, ox1 = 0, oy0 = 0, oy1 = 0, ix0 = 0, ix1 = 0, iy0 = 0, iy1 = 0, tx1 = 0, ty0 = 0, ty1 = -1, len = 0;
                if (m < b1) {
                    const float x1 = boxes[m * 4], y1 = boxes[m * 4 + 1], x2 = boxes[m * 4 + 2], y2 = boxes[m * 4 + 3];
                    if (isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2) && x2 > x1 && y2 > y1) {
                        ox0 = ovl_clamp(floorf(x1), 0.0, W - 1);
                        ox1 = ovl_clamp(ceilf(x2), -1.0, W - 1);
                        oy0 = ovl_clamp(floorf(y1), 0.0, H - 1);
                        oy1 = ovl_clamp(ceilf(y2), -1.0, H - 1);
                        const int64_t lim = INT32_MAX;
                        ix0 = (int)(((int64_t)ox0 + thickness < lim) ? (int64_t)ox0 + thickness : lim);
                        iy0 = (int)(((int64_t)oy0 + thickness < lim) ? (int64_t)oy0 + thickness : lim);
                        ix1 = ox1 - thickness;                             // >= -INT32_MAX
                        iy1 = oy1 - thickness;
                        const bool ring = ox0 <= X1 && ox1 >= X0 && oy0 <= Y1 && oy1 >= Y0 &&
                                          !(X0 >= ix0 && X1 <= ix1 && Y0 >= iy0 && Y1 <= iy1);
                        // the tag's rows do not depend on the caption; its text is read only where they meet the tile
                        if (oy0 - th9 >= 0) {
                            ty0 = (int)(oy0 - th9);
                            ty1 = oy0 - 1;
                        } else {
                            ty0 = oy0;
                            ty1 = (int)((oy0 + th9 - 1 < H - 1) ? oy0 + th9 - 1 : H - 1);
                        }
                        bool tag = false;
                        if (text && T > 0 && ty0 <= Y1 && ty1 >= Y0 && ox0 <= X1) {
                            const int8_t* __restrict__ row = text + m * T;
                            while (len < T && row[len] >= 0) ++len;
                            if (len > 0) {
                                const int64_t cells = 6 * (int64_t)len + 1;  // more cells than W: clipped at W - 1 whatever the scale
                                const int64_t end = cells > W ? W - 1 : ox0 + scale * cells - 1;
                                tx1 = (int)(end < W - 1 ? end : W - 1);
                                tag = tx1 >= X0;
                            }
                        }
                        if (!tag) {
                            len = 0;
                            ty1 = ty0 - 1;
                        }
                        hit = ring || tag;
                    }
                }
                // ---- compact the survivors in list order
                const unsigned long long mask = __ballot(hit);
                if (lane == 0) s_mask[wave] = mask;
                __syncthreads();
                int before = 0, total = 0;
#pragma unroll
                for (int w = 0; w < OVL_ROWS; ++w) {
                    const int c = __popcll(s_mask[w]);
                    before += w < wave ? c : 0;
                    total += c;
                }
                if (total == 0) {                                          // the same in every thread
                    __syncthreads();                                       // s_mask is written again in the next chunk
                    continue;
                }
                if (hit) {
                    const int e = before + __popcll(mask & ((1ull << lane) - 1ull));
                    s_ox0[e] = ox0; s_ox1[e] = ox1; s_oy0[e] = oy0; s_oy1[e] = oy1;
                    s_ix0[e] = ix0; s_ix1[e] = ix1; s_iy0[e] = iy0; s_iy1[e] = iy1;
                    s_tx1[e] = tx1; s_ty0[e] = ty0; s_ty1[e] = ty1; s_len[e] = len; s_idx[e] = (int)m;
                }
                __syncthreads();
                // ---- every undecided pixel walks the survivors
                for (int e = 0; e < total && todo; ++e) {
                    const int ex0 = s_ox0[e], ex1 = s_ox1[e], etx1 = s_tx1[e], ety0 = s_ty0[e], ety1 = s_ty1[e];
                    if (x < ex0 || (x > ex1 && (ety1 < ety0 || x > etx1))) continue;
                    const int ey0 = s_oy0[e], ey1 = s_oy1[e];
                    const bool x_inner = x >= s_ix0[e] && x <= s_ix1[e];
                    const int jy0 = s_iy0[e], jy1 = s_iy1[e], elen = s_len[e];
                    const int64_t bi = s_idx[e];
#pragma unroll
                    for (int j = 0; j < OVL_PER; ++j) {
                        if (!(todo & (1u << j))) continue;
                        const int y = Y0 + wave + j * OVL_ROWS;
                        int kind;                                          // 0 box colour, opaque; 3 text colour, opaque; -1 blended
                        if (y >= ety0 && y <= ety1 && x <= etx1) {
                            kind = 0;
                            const int nx = x - ex0 - scale, ny = y - ety0 - scale;
                            if (nx >= 0 && ny >= 0) {
                                const int u = nx / scale, v = ny / scale, k = u / 6, r = u % 6;
                                if (k < elen && r < 5 && v < 7) {
                                    const int g = text[bi * T + k];
                                    if (g < G && ((glyphs[(int64_t)g * 7 + v] >> (4 - r)) & 1)) kind = 3;
                                }
                            }
                        } else if (x <= ex1 && y >= ey0 && y <= ey1 && !(x_inner && y >= jy0 && y <= jy1)) {
                            kind = -1;
                        } else {
                            continue;
                        }
                        todo &= ~(1u << j);
                        const uint8_t* __restrict__ col = colors + bi * 6 + (kind > 0 ? kind : 0);
                        uint8_t* __restrict__ p = base + (int64_t)y * row_pitch + (int64_t)x * C;
                        if (kind >= 0 || alpha == 255) {
                            p[0] = col[0]; p[1] = col[1]; p[2] = col[2];
                        } else {
#pragma unroll
                            for (int c = 0; c < 3; ++c)
                                p[c] = (uint8_t)(((unsigned)alpha * col[c] + (unsigned)(255 - alpha) * p[c] + 127u) / 255u);
                        }
                    }
                }
                __syncthreads();                                           // the list is written again in the next chunk
            }
        }
    }
}

extern "C" int adh_draw_boxes(void* stream, uint8_t* img, int64_t row_pitch, int64_t image_pitch, int N, int H, int W, int C,
                              const int32_t* first, int M, const float* boxes, const uint8_t* colors, const void* text, int T,
                              const uint8_t* glyphs, int G, int thickness, int scale, int alpha) {
    if (!img || !first || N < 1 || H < 1 || W < 1 || (C != 3 && C != 4)) return ADH_E_ARG;
    if (row_pitch < (int64_t)W * C) return ADH_E_ARG;
    if (N > 1 && (row_pitch > INT64_MAX / H || image_pitch < (int64_t)H * row_pitch)) return ADH_E_ARG;
    if (thickness < 1 || scale < 1 || alpha < 0 || alpha > 255 || M < 0 || T < 0 || G < 0) return ADH_E_ARG;
    if (M > 0 && (!boxes || !colors)) return ADH_E_ARG;
    if (T > 0 && G > 0 && (!text || !glyphs)) return ADH_E_ARG;
    if (M == 0) return ADH_OK;
    const dim3 grid((unsigned)adh_ceil_div(W, OVL_TW), (unsigned)adh_min_i(adh_ceil_div(H, OVL_TH), OVL_MAX_GRID),
                    (unsigned)adh_min_i(N, OVL_MAX_GRID));
    hipLaunchKernelGGL(draw_boxes_kernel, grid, dim3(256), 0, (hipStream_t)stream, img, row_pitch, image_pitch, N, H, W, C, first, M,
                       boxes, colors, (const int8_t*)text, T, glyphs, G, thickness, scale, alpha);
    return adh_check_launch();
}
