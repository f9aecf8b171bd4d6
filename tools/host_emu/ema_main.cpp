// Runs the entry points of a host-compiled copy of csrc/ema.hip (see common.h in this directory; built with -DADH_HOST_EMU).
//   ema_emu in.bin out.bin
// in.bin  = int32 h[8], double decay, int32 desc[3 * h[0]], then per tensor float p[n], float ema[n]
//   h[0] tensors   h[1] mode: 0 update without a guard block, 1 update with one, 2 swap, 3 argument rejections
//   h[2] finite of the guard block (mode 1)   h[3] warmup   h[4] updates before the first call   h[5] chained updates
//   desc[3 i ..] = n, p offset, ema offset of tensor i: the tensor starts `offset` floats into a 16-byte-aligned heap block of
//   exactly offset + n floats (offset 1: the scalar path), so an out-of-range access is the sanitizer's to report; the floats
//   in front of an offset tensor are poison the caller checks.
// out.bin = int32 return code (mode 3: the return codes of the bad calls, then -100), int32 ctrl[4], then per tensor the whole
//   p block and the whole ema block
#include "common.h"
#include <cstring>
thread_local dim3 threadIdx;
dim3 blockIdx, gridDim, blockDim;
pthread_barrier_t emu_barrier;

// block.x threads walk the workgroups of the launch together (two barriers per workgroup)
void emu_launch(dim3 grid, dim3 block, std::function<void()> fn) {
    gridDim = grid;
    blockDim = block;
    pthread_barrier_init(&emu_barrier, nullptr, block.x);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; ++t)
        th.emplace_back([&fn, &grid, t]() {
            threadIdx = dim3(t);
            for (unsigned b = 0; b < grid.x; ++b) {
                if (t == 0) blockIdx = dim3(b);
                __syncthreads();
                fn();
                __syncthreads();
            }
        });
    for (auto& x : th) x.join();
    pthread_barrier_destroy(&emu_barrier);
}

static void* block16(size_t bytes) {
    void* q = nullptr;
    if (posix_memalign(&q, 16, bytes ? bytes : 1)) exit(5);
    return q;
}

int main(int argc, char** argv) {
    if (argc != 3) return 1;
    int32_t h[8];
    double decay;
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(h, 4, 8, f) != 8 || fread(&decay, 8, 1, f) != 1) return 2;
    const int nt = h[0], mode = h[1];
    std::vector<int32_t> desc(3 * nt);
    if (fread(desc.data(), 4, desc.size(), f) != desc.size()) return 2;
    const int chunk = ADH_ADAM_CHUNK;
    adh_ema_tensor* table = (adh_ema_tensor*)malloc(sizeof(adh_ema_tensor) * nt);
    std::vector<float*> pb(nt), eb(nt);
    std::vector<int32_t> pairs;
    for (int i = 0; i < nt; ++i) {
        const size_t n = desc[3 * i], po = desc[3 * i + 1], eo = desc[3 * i + 2];
        pb[i] = (float*)block16((po + n) * 4);
        eb[i] = (float*)block16((eo + n) * 4);
        const uint32_t poison = 0x7fc0dead;
        for (size_t k = 0; k < po; ++k) memcpy(pb[i] + k, &poison, 4);
        for (size_t k = 0; k < eo; ++k) memcpy(eb[i] + k, &poison, 4);
        if (fread(pb[i] + po, 4, n, f) != n || fread(eb[i] + eo, 4, n, f) != n) return 2;
        table[i].p = pb[i] + po;
        table[i].ema = eb[i] + eo;
        table[i].n = (int64_t)n;
        for (int c = 0; c < (int)((n + chunk - 1) / chunk); ++c) {
            pairs.push_back(i);
            pairs.push_back(c);
        }
    }
    fclose(f);
    const int nchunks = (int)pairs.size() / 2;
    int32_t* chunks = (int32_t*)malloc(pairs.size() * 4);
    memcpy(chunks, pairs.data(), pairs.size() * 4);
    adh_ema_ctrl* ctrl = (adh_ema_ctrl*)block16(sizeof(adh_ema_ctrl));
    memset(ctrl, 0, sizeof(*ctrl));
    ctrl->updates = h[4];
    adh_grad_ctrl* guard = (adh_grad_ctrl*)block16(sizeof(adh_grad_ctrl));
    memset(guard, 0, sizeof(*guard));
    guard->finite = h[2];
    std::vector<int32_t> rcs;
    int rc = 0;
    if (mode == 0 || mode == 1) {
        for (int k = 0; k < h[5] && rc == 0; ++k) {
            rc = adh_ema_begin(nullptr, ctrl, decay, h[3], mode == 1 ? guard : nullptr);
            if (rc == 0) rc = adh_ema_multi(nullptr, table, chunks, nchunks, ctrl);
        }
        rcs.push_back(rc);
    } else if (mode == 2) {
        rcs.push_back(adh_ema_swap(nullptr, table, chunks, nchunks));
    } else {
        char* odd = (char*)ctrl + 4;
        rcs.push_back(adh_ema_begin(nullptr, nullptr, 0.9, 1, nullptr));
        rcs.push_back(adh_ema_begin(nullptr, ctrl, 1.0, 1, nullptr));
        rcs.push_back(adh_ema_begin(nullptr, ctrl, -0.1, 1, nullptr));
        rcs.push_back(adh_ema_begin(nullptr, ctrl, NAN, 1, nullptr));
        rcs.push_back(adh_ema_begin(nullptr, odd, 0.9, 1, nullptr));
        rcs.push_back(adh_ema_begin(nullptr, ctrl, 0.9, 1, (char*)guard + 4));
        rcs.push_back(adh_ema_begin(nullptr, ctrl, 0.9, 2, nullptr));
        rcs.push_back(adh_ema_multi(nullptr, nullptr, chunks, nchunks, ctrl));
        rcs.push_back(adh_ema_multi(nullptr, table, nullptr, nchunks, ctrl));
        rcs.push_back(adh_ema_multi(nullptr, table, chunks, nchunks, nullptr));
        rcs.push_back(adh_ema_multi(nullptr, table, chunks, 0, ctrl));
        rcs.push_back(adh_ema_multi(nullptr, table, chunks, nchunks, odd));
        rcs.push_back(adh_ema_swap(nullptr, nullptr, chunks, nchunks));
        rcs.push_back(adh_ema_swap(nullptr, table, nullptr, nchunks));
        rcs.push_back(adh_ema_swap(nullptr, table, chunks, 0));
        rcs.push_back(adh_ema_swap(nullptr, table, chunks, -1));
        rcs.push_back(-100);
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(rcs.data(), 4, rcs.size(), f) != rcs.size() || fwrite(ctrl, 4, 4, f) != 4) return 4;
    for (int i = 0; i < nt; ++i) {
        const size_t n = desc[3 * i], po = desc[3 * i + 1], eo = desc[3 * i + 2];
        if (fwrite(pb[i], 4, po + n, f) != po + n || fwrite(eb[i], 4, eo + n, f) != eo + n) return 4;
        free(pb[i]);
        free(eb[i]);
    }
    fclose(f);
    free(table); free(chunks); free(ctrl); free(guard);
    return 0;
}
