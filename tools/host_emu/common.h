// Host stand-in for csrc/common.h: lets a kernel source file of the library that uses nothing but threadIdx / blockIdx,
// static __shared__ arrays and __syncthreads() be compiled by a host C++ compiler and run on CPU threads -- one OS thread per
// GPU thread, a pthread barrier for __syncthreads(), the workgroups of a launch one after the other.  The point is to run the
// kernel's own index arithmetic under the host sanitizers (-fsanitize=address,undefined) and against float64 without a GPU;
// it says nothing about speed.  Used by tests/test_ssim_loss_hostemu_cpu.py on a copy of csrc/ssim_loss.hip and, with
// -DADH_HOST_EMU (the section at the end), by tests/test_wgrad_reduce_hostemu_cpu.py on a copy of csrc/conv_wgrad_reduce.hip and
// by tests/test_ema_hostemu_cpu.py on a copy of csrc/ema.hip; with -DADH_HOST_EMU_DYN_LDS on top (the last section), by
// tests/test_fft_loss_hostemu_cpu.py on a copy of csrc/fft_loss.hip; with -DADH_HOST_EMU_STREAM on top of ADH_HOST_EMU (the section
// after it), by tests/test_{bn_act,depthwise,densenet,image_io}_hostemu_cpu.py on copies of the four streaming kernel files and by
// tests/test_ciede2000_hostemu_cpu.py on a copy of csrc/ciede2000.hip (which reduces through LDS and barriers: no shuffle).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
// csrc/common.h's: keep them the same).  Its one-wave-per-element kernel needs cross-lane shuffles and is compiled out.
#include "adam_dehaze_hip.h"   // include/, on the include path
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
#endif

#ifdef ADH_HOST_EMU_DYN_LDS
// What csrc/fft_loss.hip takes beyond the ADH_HOST_EMU section (tests/test_fft_loss_hostemu_cpu.py defines both): dynamic LDS,
// which every launch gets as a heap block of exactly the bytes it asked for, so that an LDS index out of range is the
// sanitizer's to report as well; the attribute call that lifts the 64 KiB limit on the device; bit reversal; and sincospif,
// here the float64 functions rounded once.
extern void* emu_dyn_lds;
#define ADH_DYN_LDS(T, name) T* name = (T*)emu_dyn_lds
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, grid, block, shmem, stream, ...)     \
    do {                                                           \
        emu_dyn_lds = malloc((shmem) ? (shmem) : 1);               \
        emu_launch(grid, block, [&]() { k(__VA_ARGS__); });        \
        free(emu_dyn_lds);                                         \
    } while (0)
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
#include <atomic>
#define __builtin_nontemporal_load(p) (*(p))
#define __builtin_nontemporal_store(v, p) (*(p) = (v))
static inline int adh_max_i(int a, int b) { return a > b ? a : b; }
#define __builtin_amdgcn_readfirstlane(v) (v)   // csrc/d4.hip: a value its caller knows to be wave-uniform
static inline float __fmul_rn(float a, float b) { return a * b; }   // csrc/image_io.hip: a product nothing is contracted into
// __shfl_xor(v, mask, 64): lanes t and t ^ mask exchange through one mailbox per lane and wait for nobody else, so a pair may
// shuffle inside a loop the rest of its workgroup has already left (bn_apply_kernel).  A lane's n-th shuffle posts into slot
// n & 1 and publishes n + 1; its partner cannot post n + 2 before it has read n, so two slots are enough.  A lane whose
// partner has left the kernel waits for ever: the tests run every driver under a timeout.
struct emu_mailbox {
    std::atomic<unsigned> seq;
    int val[2];
};
extern emu_mailbox emu_mail[1024];           // stream_rt.cpp clears them before every launch
extern thread_local unsigned emu_shfl_count;
static inline int __shfl_xor(int v, int mask, int width) {
    (void)width;
    const unsigned n = emu_shfl_count++;
    emu_mailbox& mine = emu_mail[threadIdx.x];
    emu_mailbox& theirs = emu_mail[threadIdx.x ^ (unsigned)mask];
    mine.val[n & 1] = v;
    mine.seq.store(n + 1, std::memory_order_release);
    while (theirs.seq.load(std::memory_order_acquire) < n + 1) std::this_thread::yield();
    return theirs.val[n & 1];
}
#include "../adam-dehaze_amd/csrc/bn_stream.h"
#endif
