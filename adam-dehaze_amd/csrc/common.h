// Shared device/host helpers for libadamdehaze_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/adam_dehaze_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define ADH_WAVE 64

// floats per workgroup of the multi-tensor kernels (train_io.hip: Adam and the gradient guard; ema.hip): adh_adam_chunk_elems()
#define ADH_ADAM_CHUNK 16384

// the launch's dynamic LDS as an array of T (a macro so that tools/host_emu/common.h can stand in a heap block for it)
#define ADH_DYN_LDS(T, name) extern __shared__ __attribute__((aligned(16))) T name[]

static inline int adh_check_launch() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADH_OK : ADH_E_LAUNCH;
}

__host__ __device__ static inline int adh_min_i(int a, int b) { return a < b ? a : b; }
__host__ __device__ static inline int adh_max_i(int a, int b) { return a > b ? a : b; }
static inline int adh_ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
static inline int adh_round_up(int a, int b) { return (a + b - 1) / b * b; }

// Tap-extent helpers (host + device)
__host__ __device__ static inline int adh_tap_min(int d0, int step, int k) {
    int e = d0 + (k - 1) * step;
    return d0 < e ? d0 : e;
}
__host__ __device__ static inline int adh_tap_max(int d0, int step, int k) {
    int e = d0 + (k - 1) * step;
    return d0 > e ? d0 : e;
}

// Geometry of one conv launch, derived on the host and passed by value.
struct ConvGeom {
    int dmin_y, dmin_x;     // smallest tap offsets
    int halo_h, halo_w;     // input footprint of one TH x 32 tile
    int npx, npxp;          // halo pixels, padded (odd) pitch
    int tiles_x, tiles_y;
    int KC, KQ_log2;        // channels per LDS chunk, log2(KC/4)
    int KQtot;              // padded Cin / 4
    int TH;                 // tile rows (8 for forward)
    int xp;                 // wgrad: floats per staged input pixel (32, or Cin alloc (8) in packed small-Cin mode)
};

#include "wave.h"   // wave_sum, wave_max (shared with the host-emulation build)
__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + __expf(-v)); }
// (the activations of the BatchNorm / depthwise epilogues, adh_act_*: bn_stream.h)

// a - b on float4 as two v_pk_fma_f32 (b * (-1) + a, exact: one rounding) instead of the four v_sub_f32 hipcc emits for a
// vector subtraction; `m1` is -1.0f held in an SGPR the compiler cannot see through (adh_opaque(-1.f)), otherwise it folds
// the product back into a subtraction.  Matters where VALU instructions come out of fp32 MFMA time.
__device__ __forceinline__ float adh_opaque(float v) {
    asm volatile("" : "+s"(v));
    return v;
}
__device__ __forceinline__ f32x4 adh_pksub(const f32x4& a, const f32x4& b, float m1) { return m1 * b + a; }

// gfx950: an MFMA that reads a VGPR a VALU instruction wrote one or two instructions earlier gets the OLD value (measured
// with tools/dev_wgrad32_probe.py on conv_wgrad32_kernel: the product of the frequency whose MFMA hipcc scheduled right behind the v_fmac that
// finishes its B operand lost exactly that term).  hipcc pads VALU -> MFMA hazards for MFMA *instructions*; ours are inline
// asm, which its hazard recogniser does not look into.  The operands therefore pass through an asm that holds two wait
// states behind the last VALU write before any MFMA may issue.
template <int TN>
__device__ __forceinline__ void adh_mfma_operand_fence(float (&V)[4], float (&M)[TN][4]) {
    if constexpr (TN == 1)
        asm volatile("s_nop 1" : "+v"(V[0]), "+v"(V[1]), "+v"(V[2]), "+v"(V[3]), "+v"(M[0][0]), "+v"(M[0][1]), "+v"(M[0][2]), "+v"(M[0][3]));
    if constexpr (TN == 2)
        asm volatile("s_nop 1" : "+v"(V[0]), "+v"(V[1]), "+v"(V[2]), "+v"(V[3]), "+v"(M[0][0]), "+v"(M[0][1]), "+v"(M[0][2]), "+v"(M[0][3]),
                     "+v"(M[1][0]), "+v"(M[1][1]), "+v"(M[1][2]), "+v"(M[1][3]));
    if constexpr (TN == 3)
        asm volatile("s_nop 1" : "+v"(V[0]), "+v"(V[1]), "+v"(V[2]), "+v"(V[3]), "+v"(M[0][0]), "+v"(M[0][1]), "+v"(M[0][2]), "+v"(M[0][3]),
                     "+v"(M[1][0]), "+v"(M[1][1]), "+v"(M[1][2]), "+v"(M[1][3]), "+v"(M[2][0]), "+v"(M[2][1]), "+v"(M[2][2]), "+v"(M[2][3]));
}

// Offset of element (tap (ty, tx), k, n) of a weight tensor described by `L` (include/adam_dehaze_hip.h, adh_wlayout).  The tap
// strides may be negative (reversed taps: tap_off0 then names the last tap).  The pack kernels read, and the weight-gradient reduce
// kernels write, through this one expression (conv_wino43.hip's pack kernels stage the nine taps of a (k, n) pair as one window
// from the smallest tap offset instead).  The tap part alone is for callers that hoist it out of a (k, n) loop.
__host__ __device__ static inline int64_t adh_wlayout_tap_off(const adh_wlayout& L, int ty, int tx) {
    return (int64_t)L.tap_off0 + ty * L.tap_off_sy + tx * L.tap_off_sx;
}
__host__ __device__ static inline int64_t adh_wlayout_off(const adh_wlayout& L, int ty, int tx, int k, int n) {
    return adh_wlayout_tap_off(L, ty, tx) + (int64_t)k * L.stride_k + (int64_t)n * L.stride_n;
}

// Grid of the split-accumulating weight-gradient kernels (conv_wgrad_rows_kernel, conv_wgrad32_kernel, conv_wgrad32v2*_kernel,
// conv_wgrad_wino43_kernel): `ngroups` workgroups (channel-block pairs) share one pixel split and so re-read the same tiles.
// One workgroup is resident per CU and the hardware deals workgroups to the 8 XCDs round-robin (block b runs on XCD b % 8), so
// block b is mapped to  group = (b >> 3) % ngroups,  split = (b >> 3) / ngroups * 8 + (b & 7):  the groups of one split have ids
// congruent mod 8, land on one XCD and are served by its L2 after the first read; XCD x gets the splits = x mod 8 of every
// group.  The split count is rounded up to a multiple of 8 for the launch; a block whose split >= nsplit returns at once.
// (engine._rows_nsplit chooses nsplit from the cost of the rounds this mapping gives.)
static inline int adh_split_grid_blocks(int nsplit, int ngroups) { return ((nsplit + 7) / 8) * ngroups * 8; }
__device__ __forceinline__ void adh_split_grid_decode(int bid, int ngroups, int& group, int& split) {
    const int q = bid >> 3;
    group = q % ngroups;
    split = (q / ngroups) * 8 + (bid & 7);
}

// Interpolation points +-a, +-b (and 0, infinity) of the F(4x4,3x3) weight gradient: conv_wgrad43.hip transforms with them,
// conv_wgrad_reduce.hip inverts
#define G4_A 0.75f
#define G4_B 1.25f

// conv_wgrad_reduce.hip: slab[0] = sum over `nsplit` partial slabs of n4 float4 each (in place, fixed order)
void adh_wgrad_sum_splits(hipStream_t s, float* slab, int nsplit, int64_t n4);

// conv_wgrad32.hip: the kernel-parity classes of the F(3x3,2x2)-domain weight gradient of `d`, for adh_wgrad_reduce_wino32:
// output tap (hy, hx) of class c is tap index tap0[c] + ty tap_sy[c] + tx tap_sx[c] of d's KH x KW taps, (ty, tx) = (hy, hx), or
// (1 - hy, 1 - hx) where rev[c] (taps walked backwards).  Returns 0 when `d` is not one of that path's shapes.
struct adh_wg32_taps {
    int ncls;
    int tap0[4], tap_sy[4], tap_sx[4], rev[4];
};
int adh_wgrad32_class_taps(const adh_conv_desc* d, adh_wg32_taps* tp);

// conv_rows.hip: direct forward kernel for the 2x2 / 3x3-tap gather forms (0 blocks / ADH_E_UNSUPPORTED when `d`
// is not one of its shapes; conv_igemm.hip then takes the launch)
int adh_rows_fwd_num_blocks(const adh_conv_desc* d);
int adh_rows_fwd_launch(void* stream, const adh_conv_desc* d);

// the pieces the streaming kernels share (bn_act.hip, densenet.hip, cbam.hip, depthwise.hip) and the activations adh_act_*; the
// host-emulation build's stand-in for this file includes the same header
#include "bn_stream.h"
