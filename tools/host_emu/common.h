// Host stand-in for csrc/common.h: lets a kernel source file of the library that uses nothing but threadIdx / blockIdx,
// static __shared__ arrays and __syncthreads() be compiled by a host C++ compiler and run on CPU threads -- one OS thread per
// GPU thread, a pthread barrier for __syncthreads(), the workgroups of a launch one after the other.  The point is to run the
// kernel's own index arithmetic under the host sanitizers (-fsanitize=address,undefined) and against float64 without a GPU;
// it says nothing about speed.  Used by tests/test_ssim_loss_hostemu_cpu.py on a copy of csrc/ssim_loss.hip.
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
