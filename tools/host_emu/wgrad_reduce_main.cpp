// Runs one reduce entry point of a host-compiled copy of csrc/conv_wgrad_reduce.hip (see common.h in this directory).
//   wgrad_reduce_emu in.bin out.bin
// in.bin  = int32 h[40], float slab[h[15]], float dst[h[14]];  out.bin = int32 return code, float dst[h[14]]
//   h[0] entry point: 0 adh_wgrad_reduce, 2 _packed, 3 _wino, 4 _wino32, 5 _wino43     h[1] nsplit   h[2] KP   h[3] NcP
//   h[4..12] adh_wlayout   h[13] accumulate   h[14] dst floats   h[15] slab floats   h[16..19] packed form: Cin KH KW Cout
//   h[20] classes of the wino32 form (0: not one of its shapes), h[21 + 4 i + c] tap0 / tap_sy / tap_sx / rev (i = 0..3) of class c
//   h[37] 1: pass a null slab
// Slab and dst are heap blocks of exactly their sizes, so an out-of-range access is the sanitizer's to report.  The class taps
// conv_wgrad32.hip derives from a descriptor come from the case instead (adh_wgrad32_class_taps below).
#include "common.h"
#include <cstring>
thread_local dim3 threadIdx;
dim3 blockIdx, gridDim, blockDim;
pthread_barrier_t emu_barrier;

// block.x threads walk the workgroups of the launch together (two barriers per workgroup; a kernel's own barriers in between)
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

static adh_wg32_taps case_taps;
int adh_wgrad32_class_taps(const adh_conv_desc*, adh_wg32_taps* tp) {
    *tp = case_taps;
    return case_taps.ncls > 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 1;
    int32_t h[40];
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(h, 4, 40, f) != 40) return 2;
    const size_t nslab = h[15], ndst = h[14];
    float* slab = (float*)malloc(nslab * 4);
    float* dst = (float*)malloc(ndst * 4);
    if (fread(slab, 4, nslab, f) != nslab || fread(dst, 4, ndst, f) != ndst) return 2;
    fclose(f);
    adh_wlayout L;
    memcpy(&L, h + 4, sizeof(L));
    float* sl = h[37] ? nullptr : slab;
    const int nsplit = h[1], KP = h[2], NcP = h[3], acc = h[13];
    int rc = -100;
    if (h[0] == 0) rc = adh_wgrad_reduce(nullptr, sl, nsplit, KP, NcP, &L, dst, acc);
    if (h[0] == 2) rc = adh_wgrad_reduce_packed(nullptr, sl, nsplit, NcP, h[16], h[17], h[18], h[19], dst, acc);
    if (h[0] == 3) rc = adh_wgrad_reduce_wino(nullptr, sl, nsplit, KP, NcP, &L, dst, acc);
    if (h[0] == 5) rc = adh_wgrad_reduce_wino43(nullptr, sl, nsplit, KP, NcP, &L, dst, acc);
    if (h[0] == 4) {
        case_taps.ncls = h[20];
        for (int c = 0; c < 4; ++c) {
            case_taps.tap0[c] = h[21 + c]; case_taps.tap_sy[c] = h[25 + c]; case_taps.tap_sx[c] = h[29 + c]; case_taps.rev[c] = h[33 + c];
        }
        adh_conv_desc d;
        memset(&d, 0, sizeof(d));
        d.KH = L.KHt; d.KW = L.KWt;
        rc = adh_wgrad_reduce_wino32(nullptr, sl, nsplit, &d, KP, NcP, &L, dst, acc);
    }
    f = fopen(argv[2], "wb");
    const int32_t rc32 = rc;
    if (!f || fwrite(&rc32, 4, 1, f) != 1 || fwrite(dst, 4, ndst, f) != ndst) return 4;
    fclose(f);
    free(slab); free(dst);
    return 0;
}
