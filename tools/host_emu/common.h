// Host stand-in for csrc/common.h: lets a kernel source file of the library that uses nothing but threadIdx / blockIdx,
// static __shared__ arrays and __syncthreads() be compiled by a host C++ compiler and run on CPU threads -- one OS thread per
// GPU thread, a pthread barrier for __syncthreads(), the workgroups of a launch one after the other.  The point is to run the
// kernel's own index arithmetic under the host sanitizers (-fsanitize=address,undefined) and against float64 without a GPU;
// it says nothing about speed.  Used by tests/test_ssim_loss_hostemu_cpu.py on a copy of csrc/ssim_loss.hip and, with
// -DADH_HOST_EMU (the section at the end), by tests/test_ema_hostemu_cpu.py on a copy of csrc/ema.hip; with
// -DADH_HOST_EMU_DYN_LDS on top, by tests/test_fft_loss_hostemu_cpu.py on a copy of csrc/fft_loss.hip; with
// -DADH_HOST_EMU_STREAM on top of ADH_HOST_EMU (the last section; the cross-lane shuffle and the wave reductions are ADH_HOST_EMU's), by
// tests/test_{bn_act,depthwise,densenet,image_io,d4,ciede2000}_hostemu_cpu.py, by
// tests/test_{cbam,lpips,detect,pointwise,train_io}_hostemu_cpu.py and tests/test_wgrad_reduce_hostemu_cpu.py on copies of their kernel
// files (pointwise and train_io a second time with their grid caps set small by -D), by tests/test_msssim_hostemu_cpu.py on a copy of
// csrc/msssim.hip (its grid.y cap set to 2 by -D, so that the plane loop runs), by tests/test_overlay_hostemu_cpu.py on a copy of
// csrc/overlay.hip (its grid cap set to 2 by -D; the wave vote __ballot is built on the shuffle), by
// tests/test_dataset_hostemu_cpu.py on a copy of csrc/dataset.hip (float64 butterflies in both of its batch kernels), by
// tests/test_nss_hostemu_cpu.py on a copy of csrc/nss.hip (its grid cap set to 2 by -D, so that the region loop runs), and by
// tests/test_hostemu_shuffle_cpu.py on the shuffle itself.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <pthread.h>
#include <thread>
#include <vector>
#define __global__
#define __shared__ static
#define __launch_bounds__(x)
#define ADH_OK 0
#define ADH_E_ARG (-1)
#define ADH_E_LAUNCH (-2)
#define ADH_E_UNSUPPORTED (-3)
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
typedef void* hipStream_t;
extern thread_local dim3 threadIdx;
extern dim3 blockIdx, gridDim;
extern pthread_barrier_t emu_barrier;
static inline void __syncthreads() { pthread_barrier_wait(&emu_barrier); }
static inline int adh_check_launch() { return ADH_OK; }
static inline int adh_ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
void emu_launch(dim3 grid, dim3 block, std::function<void()> fn);
#define hipLaunchKernelGGL(k, grid, block, shmem, stream, ...) emu_launch(grid, block, [&]() { k(__VA_ARGS__); })

#ifdef ADH_HOST_EMU
// What csrc/conv_wgrad_reduce.hip takes from csrc/common.h beyond the above: the public structs, the grid-stride loop's
// blockDim, float4 arithmetic, and the helpers and internal declarations it shares with the other source files (copies of
// csrc/common.h's: keep them the same), and for its one-wave-per-element kernel the cross-lane shuffle and csrc/wave.h.
#include "adam_dehaze_hip.h"   // include/, on the include path
#include <atomic>
#define __host__
#define __device__
#define __forceinline__ inline
extern dim3 blockDim;
typedef float f32x4 __attribute__((vector_size(16)));
static inline int adh_min_i(int a, int b) { return a < b ? a : b; }
static inline int64_t adh_wlayout_tap_off(const adh_wlayout& L, int ty, int tx) {
    return (int64_t)L.tap_off0 + ty * L.tap_off_sy + tx * L.tap_off_sx;
}
static inline int64_t adh_wlayout_off(const adh_wlayout& L, int ty, int tx, int k, int n) {
    return adh_wlayout_tap_off(L, ty, tx) + (int64_t)k * L.stride_k + (int64_t)n * L.stride_n;
}
#define G4_A 0.75f
#define G4_B 1.25f
void adh_wgrad_sum_splits(hipStream_t s, float* slab, int nsplit, int64_t n4);
struct adh_wg32_taps {
    int ncls;
    int tap0[4], tap_sy[4], tap_sx[4], rev[4];
};
int adh_wgrad32_class_taps(const adh_conv_desc* d, adh_wg32_taps* tp);
#define ADH_ADAM_CHUNK 16384   // csrc/ema.hip: floats per workgroup (csrc/common.h's)
// __shfl_xor(v, mask, 64): lanes t and u = t ^ mask exchange 32 bits through the channel the pair owns, emu_chan[t][mask] and
// emu_chan[u][mask], and wait for nobody else, so a pair may shuffle inside a loop the rest of its workgroup has already left
// (bn_apply_kernel), and the waves of a workgroup may shuffle different numbers of times (cbam_mlp_kernel).  A channel counts
// the shuffles its lane has made with THIS partner, so the n-th shuffle of t with u meets the n-th shuffle of u with t whatever
// either lane has exchanged with third lanes in between -- a butterfly changes partners every step.  For its n-th shuffle
// with u, t writes slot n & 1 of its channel, publishes n + 1, waits until u's channel has published n + 1 and reads u's slot
// n & 1.  Two slots are enough: t overwrites slot n & 1 in its shuffle n + 2 with u, after it finished n + 1, that is after u
// published n + 2, which u does only after it has read t's slot of shuffle n (release / acquire on `seq` orders the plain
// accesses).  The counters run on over the workgroups of a launch; stream_rt.cpp clears them before the next one, and under a
// launcher that does not (wgrad_reduce_main.cpp) they run on over the launches too, which pairs as well.  A lane whose partner
// has left the kernel waits for ever: the tests run every driver under a timeout.  mask is 1..63 and the partner must be a
// lane of the workgroup; the value travels bit for bit (a NaN payload, -0.0f; a double as two such exchanges).
struct emu_channel {
    std::atomic<unsigned> seq;
    uint32_t val[2];
};
inline emu_channel emu_chan[1024][64];       // (an inline variable: no driver has to define it)
static inline uint32_t emu_shfl_bits(uint32_t v, int mask) {
    if (mask == 0) return v;
    const unsigned u = threadIdx.x ^ (unsigned)mask;
    if (mask < 0 || mask > 63 || u >= blockDim.x) {
        fprintf(stderr, "__shfl_xor: lane %u, mask %d: no such partner in a workgroup of %u\n", threadIdx.x, mask, blockDim.x);
        abort();
    }
    emu_channel& mine = emu_chan[threadIdx.x][mask];
    emu_channel& theirs = emu_chan[u][mask];
    const unsigned n = mine.seq.load(std::memory_order_relaxed);
    mine.val[n & 1] = v;
    mine.seq.store(n + 1, std::memory_order_release);
    while (theirs.seq.load(std::memory_order_acquire) < n + 1) std::this_thread::yield();
    return theirs.val[n & 1];
}
static inline int __shfl_xor(int v, int mask, int) { return (int)emu_shfl_bits((uint32_t)v, mask); }
static inline unsigned __shfl_xor(unsigned v, int mask, int) { return emu_shfl_bits(v, mask); }
static inline float __shfl_xor(float v, int mask, int) {
    uint32_t b;
    memcpy(&b, &v, 4);
    b = emu_shfl_bits(b, mask);
    memcpy(&v, &b, 4);
    return v;
}
// a double travels as two 32-bit exchanges on the pair's channel, low word first: both lanes make the same two, so the counts of
// the channel stay in step and the 64 bits arrive bit for bit (csrc/train_io.hip's float64 butterflies)
static inline double __shfl_xor(double v, int mask, int) {
    uint32_t w[2];
    memcpy(w, &v, 8);
    w[0] = emu_shfl_bits(w[0], mask);
    w[1] = emu_shfl_bits(w[1], mask);
    memcpy(&v, w, 8);
    return v;
}
#include "../adam-dehaze_amd/csrc/wave.h"
#endif

#if defined(ADH_HOST_EMU_DYN_LDS) || defined(ADH_HOST_EMU_STREAM)
// Dynamic LDS (csrc/fft_loss.hip; in the stream section cbam_mlp_kernel, cbam_bwd_d2_kernel and nms_scan_kernel): every launch
// gets a heap block of exactly the bytes it asked for, so that an LDS index out of range is the sanitizer's to report as well.
extern void* emu_dyn_lds;
#define ADH_DYN_LDS(T, name) T* name = (T*)emu_dyn_lds
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, grid, block, shmem, stream, ...)     \
    do {                                                           \
        emu_dyn_lds = malloc((shmem) ? (shmem) : 1);               \
        emu_launch(grid, block, [&]() { k(__VA_ARGS__); });        \
        free(emu_dyn_lds);                                         \
    } while (0)
#endif

#ifdef ADH_HOST_EMU_DYN_LDS
// What csrc/fft_loss.hip takes beyond the ADH_HOST_EMU section and dynamic LDS (tests/test_fft_loss_hostemu_cpu.py defines
// both): the attribute call that lifts the 64 KiB limit on the device; bit reversal; and sincospif, here the float64 functions
// rounded once.
#define hipFuncAttributeMaxDynamicSharedMemorySize 0
static inline int hipFuncSetAttribute(const void*, int, int) { return 0; }
static inline unsigned __brev(unsigned v) {
    unsigned r = 0;
    for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i);
    return r;
}
static inline void sincospif(float x, float* s, float* c) {
    *s = (float)sin(3.14159265358979323846 * (double)x);
    *c = (float)cos(3.14159265358979323846 * (double)x);
}
#endif

#ifdef ADH_HOST_EMU_STREAM
// What csrc/bn_act.hip, csrc/depthwise.hip, csrc/densenet.hip, csrc/image_io.hip and csrc/d4.hip (tests/test_d4_hostemu_cpu.py; its
// transposing kernel stages a static LDS tile between barriers) take beyond the ADH_HOST_EMU section; their drivers link
// stream_rt.cpp, whose emu_launch walks grid.x, grid.y and grid.z.  The non-temporal builtins are plain loads and stores.  The
// activation helpers and the shared BatchNorm pieces are csrc/bn_stream.h itself, included at the end of this section as
// csrc/common.h includes it at its end (the path is found from include/, which every build of this file has on its include path).
#define __builtin_nontemporal_load(p) (*(p))
#define __builtin_nontemporal_store(v, p) (*(p) = (v))
static inline int adh_max_i(int a, int b) { return a > b ? a : b; }
#define __builtin_amdgcn_readfirstlane(v) (v)   // csrc/d4.hip: a value its caller knows to be wave-uniform
static inline float __fmul_rn(float a, float b) { return a * b; }   // csrc/image_io.hip: a product nothing is contracted into
static inline int hipMemsetAsync(void* p, int v, size_t n, hipStream_t) { memset(p, v, n); return 0; }   // csrc/detect.hip
using std::isfinite;   // csrc/train_io.hip calls it unqualified, as device code does; <cmath> only declares std::isfinite
// csrc/overlay.hip: the wave's vote as a 64-bit mask, bit l = lane l's predicate, here an OR butterfly of two 32-bit halves over
// the shuffle above; every lane of a whole 64-lane wave must call it, as on the device.  And the population count.
static inline unsigned long long __ballot(int pred) {
    const unsigned l = threadIdx.x & 63;
    unsigned lo = (pred && l < 32) ? 1u << l : 0u, hi = (pred && l >= 32) ? 1u << (l - 32) : 0u;
    for (int o = 32; o > 0; o >>= 1) {
        lo |= __shfl_xor(lo, o, 64);
        hi |= __shfl_xor(hi, o, 64);
    }
    return ((unsigned long long)hi << 32) | lo;
}
static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
#include "../adam-dehaze_amd/csrc/bn_stream.h"
#endif
