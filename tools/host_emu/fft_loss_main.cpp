// Runs adh_fft_l1 of a host-compiled copy of csrc/fft_loss.hip (see common.h in this directory; built with -DADH_HOST_EMU
// -DADH_HOST_EMU_DYN_LDS).
//   fft_loss_emu N H W ortho grad in.bin out.bin
// in.bin = pred[N*3*H*W] target[N*3*H*W], fp32; out.bin = loss (one float), then g_pred[N*3*H*W] when grad = 1.
// Every buffer, the workspace, the partials and each launch's LDS included, is a heap block of exactly the size the library
// asks for, so an out-of-range access is the sanitizer's to report.  With grad = 0 no gradient buffer exists at all.
#include "common.h"
thread_local dim3 threadIdx;
dim3 blockIdx, gridDim, blockDim;
pthread_barrier_t emu_barrier;
void* emu_dyn_lds;

// block.x threads walk the workgroups of the launch together (two barriers per workgroup)
void emu_launch(dim3 grid, dim3 block, std::function<void()> fn) {
    gridDim = grid;
    blockDim = block;
    pthread_barrier_init(&emu_barrier, nullptr, block.x);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; ++t)
        th.emplace_back([&fn, &grid, t]() {
            threadIdx = dim3(t);
            for (unsigned by = 0; by < grid.y; ++by)
                for (unsigned bx = 0; bx < grid.x; ++bx) {
                    if (t == 0) blockIdx = dim3(bx, by);
                    __syncthreads();
                    fn();
                    __syncthreads();
                }
        });
    for (auto& x : th) x.join();
    pthread_barrier_destroy(&emu_barrier);
}

int main(int argc, char** argv) {
    if (argc != 8) return 1;
    const int N = atoi(argv[1]), H = atoi(argv[2]), W = atoi(argv[3]), ortho = atoi(argv[4]), want_grad = atoi(argv[5]);
    const size_t n = (size_t)N * 3 * H * W;
    const int wsb = adh_fft_l1_workspace_bytes(N, H, W), np = adh_fft_l1_num_partials(N, H, W);
    if (wsb < 0 || np < 0) {
        printf("queries returned %d %d\n", wsb, np);
        return 3;
    }
    float* p = (float*)malloc(n * 4);
    float* t = (float*)malloc(n * 4);
    void* ws = malloc(wsb);
    double* part = (double*)malloc((size_t)np * 8);
    float* loss = (float*)malloc(4);
    float* g = want_grad ? (float*)malloc(n * 4) : nullptr;
    FILE* f = fopen(argv[6], "rb");
    if (!f || fread(p, 4, n, f) != n || fread(t, 4, n, f) != n) return 2;
    fclose(f);
    *loss = NAN;
    for (int i = 0; i < np; ++i) part[i] = NAN;
    for (size_t i = 0; g && i < n; ++i) g[i] = NAN;
    const int rc = adh_fft_l1(nullptr, p, t, N, H, W, ortho, ws, part, loss, g);
    if (rc) {
        printf("adh_fft_l1 returned %d\n", rc);
        return 3;
    }
    f = fopen(argv[7], "wb");
    if (!f || fwrite(loss, 4, 1, f) != 1 || (g && fwrite(g, 4, n, f) != n)) return 4;
    fclose(f);
    free(p); free(t); free(ws); free(part); free(loss); free(g);
    return 0;
}
