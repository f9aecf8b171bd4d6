// Exponential moving average of the weights, gfx950: a shadow copy of every parameter that follows the optimiser on the device
// (BasicSR's model_ema; the reference validates its raw last-step weights).  Streaming kernels in the mould of
// adam_multi_kernel (train_io.hip): one workgroup of 256 threads per (tensor, chunk) pair of a resident table, 16-byte accesses
// where every pointer of the tensor allows them, a scalar path otherwise and for the tail, no atomics, nothing shared between
// workgroups.  Whether a step updates the shadow is decided on the device: ema_begin_kernel reads the optimiser's adh_grad_ctrl
// (written earlier on the stream by grad_guard_finalize_kernel) and writes the small adh_ema_ctrl the blend kernel obeys.
#include "common.h"

#define EMA_CHUNK ADH_ADAM_CHUNK   // floats per workgroup: the (tensor, chunk) lists are built with adh_adam_chunk_elems()

// one workgroup; thread 0 writes.  Blend weight in double, rounded to float once.
__global__ __launch_bounds__(256) void ema_begin_kernel(adh_ema_ctrl* __restrict__ ctrl, double decay, int warmup,
                                                        const adh_grad_ctrl* __restrict__ guard) {
    if (threadIdx.x != 0) return;
    if (guard != nullptr && guard->finite == 0) {   // the optimiser skipped this step: the shadow stays, no update is counted
        ctrl->active = 0;
        return;
    }
    const int32_t updates = ctrl->updates + 1;
    double d = decay;
    if (warmup) {
        const double ramp = (1.0 + (double)updates) / (10.0 + (double)updates);
        d = ramp < decay ? ramp : decay;
    }
    ctrl->updates = updates;
    ctrl->active = 1;
    ctrl->w = (float)(1.0 - d);
}

// ema += w * (p - ema): reads p and ema, writes ema (12 B per parameter)
__global__ __launch_bounds__(256) void ema_multi_kernel(const adh_ema_tensor* __restrict__ table,
                                                        const int32_t* __restrict__ chunks,
                                                        const adh_ema_ctrl* __restrict__ ctrl) {
    if (ctrl->active == 0) return;                  // uniform load: every lane reads the same address
    const float w = ctrl->w;
    const int ti = chunks[2 * blockIdx.x], ci = chunks[2 * blockIdx.x + 1];
    const adh_ema_tensor t = table[ti];
    const int64_t base = (int64_t)ci * EMA_CHUNK;
    const int n = (int)((t.n - base) < EMA_CHUNK ? (t.n - base) : EMA_CHUNK);
    const float* __restrict__ p = t.p + base;
    float* __restrict__ e = t.ema + base;
    const bool vec = ((((uintptr_t)p) | ((uintptr_t)e)) & 15) == 0;
    const int n4 = vec ? (n >> 2) : 0;
    for (int i = threadIdx.x; i < n4; i += 256) {
        const f32x4 pv = reinterpret_cast<const f32x4*>(p)[i];
        f32x4 ev = reinterpret_cast<f32x4*>(e)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) ev[j] = ev[j] + w * (pv[j] - ev[j]);
        reinterpret_cast<f32x4*>(e)[i] = ev;
    }
    for (int i = n4 * 4 + threadIdx.x; i < n; i += 256) e[i] = e[i] + w * (p[i] - e[i]);
}

// p <-> ema in place, bit for bit (16 B per parameter); the pointers do not move
__global__ __launch_bounds__(256) void ema_swap_kernel(const adh_ema_tensor* __restrict__ table,
                                                       const int32_t* __restrict__ chunks) {
    const int ti = chunks[2 * blockIdx.x], ci = chunks[2 * blockIdx.x + 1];
    const adh_ema_tensor t = table[ti];
    const int64_t base = (int64_t)ci * EMA_CHUNK;
    const int n = (int)((t.n - base) < EMA_CHUNK ? (t.n - base) : EMA_CHUNK);
    float* __restrict__ p = t.p + base;             // plain loads and stores: no arithmetic touches a value, NaN payloads survive
    float* __restrict__ e = t.ema + base;
    const bool vec = ((((uintptr_t)p) | ((uintptr_t)e)) & 15) == 0;
    const int n4 = vec ? (n >> 2) : 0;
    for (int i = threadIdx.x; i < n4; i += 256) {
        const f32x4 pv = reinterpret_cast<f32x4*>(p)[i], ev = reinterpret_cast<f32x4*>(e)[i];
        reinterpret_cast<f32x4*>(p)[i] = ev;
        reinterpret_cast<f32x4*>(e)[i] = pv;
    }
    for (int i = n4 * 4 + threadIdx.x; i < n; i += 256) {
        const float pv = p[i], ev = e[i];
        p[i] = ev;
        e[i] = pv;
    }
}

extern "C" int adh_ema_begin(void* stream, void* ema_ctrl_dev, double decay, int warmup, const void* guard_ctrl_dev) {
    if (!ema_ctrl_dev || !(decay >= 0.0 && decay < 1.0) || (warmup != 0 && warmup != 1) ||
        (((uintptr_t)ema_ctrl_dev) & 7) != 0 || (((uintptr_t)guard_ctrl_dev) & 7) != 0)
        return ADH_E_ARG;
    hipLaunchKernelGGL(ema_begin_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (adh_ema_ctrl*)ema_ctrl_dev, decay, warmup,
                       (const adh_grad_ctrl*)guard_ctrl_dev);
    return adh_check_launch();
}

extern "C" int adh_ema_multi(void* stream, const void* table_dev, const int32_t* chunks_dev, int nchunks,
                             const void* ema_ctrl_dev) {
    if (!table_dev || !chunks_dev || !ema_ctrl_dev || nchunks < 1 || (((uintptr_t)ema_ctrl_dev) & 7) != 0) return ADH_E_ARG;
    hipLaunchKernelGGL(ema_multi_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream,
                       (const adh_ema_tensor*)table_dev, chunks_dev, (const adh_ema_ctrl*)ema_ctrl_dev);
    return adh_check_launch();
}

extern "C" int adh_ema_swap(void* stream, const void* table_dev, const int32_t* chunks_dev, int nchunks) {
    if (!table_dev || !chunks_dev || nchunks < 1) return ADH_E_ARG;
    hipLaunchKernelGGL(ema_swap_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream,
                       (const adh_ema_tensor*)table_dev, chunks_dev);
    return adh_check_launch();
}
