// Runs adh_ssim_gray_bwd of a host-compiled copy of csrc/ssim_loss.hip (see common.h in this directory).
//   ssim_bwd_emu N H W in.bin out.bin      in.bin = pred[N*3*H*W] target[N*3*H*W] g_ssim[N], fp32; out.bin = g_pred[N*3*H*W]
// Every buffer is a heap block of exactly its size, so an out-of-range access is the sanitizer's to report.
#include "common.h"
thread_local dim3 threadIdx;
dim3 blockIdx, gridDim;
pthread_barrier_t emu_barrier;

void emu_launch(dim3 grid, dim3 block, std::function<void()> fn) {
    gridDim = grid;
    for (unsigned by = 0; by < grid.y; ++by)
        for (unsigned bx = 0; bx < grid.x; ++bx) {
            blockIdx = dim3(bx, by);
            pthread_barrier_init(&emu_barrier, nullptr, block.x);
            std::vector<std::thread> th;
            for (unsigned t = 0; t < block.x; ++t)
                th.emplace_back([&fn, t]() {
                    threadIdx = dim3(t);
                    fn();
                });
            for (auto& x : th) x.join();
            pthread_barrier_destroy(&emu_barrier);
        }
}

extern "C" int adh_ssim_gray_bwd(void*, const float*, const float*, int, int, int, float, const float*, float*);

int main(int argc, char** argv) {
    if (argc != 6) return 1;
    const int N = atoi(argv[1]), H = atoi(argv[2]), W = atoi(argv[3]);
    const size_t n = (size_t)N * 3 * H * W;
    float* p = (float*)malloc(n * 4);
    float* t = (float*)malloc(n * 4);
    float* g = (float*)malloc((size_t)N * 4);
    float* o = (float*)malloc(n * 4);
    FILE* f = fopen(argv[4], "rb");
    if (!f || fread(p, 4, n, f) != n || fread(t, 4, n, f) != n || fread(g, 4, N, f) != (size_t)N) return 2;
    fclose(f);
    for (size_t i = 0; i < n; ++i) o[i] = NAN;
    const int rc = adh_ssim_gray_bwd(nullptr, p, t, N, H, W, 1.0f, g, o);
    if (rc) {
        printf("adh_ssim_gray_bwd returned %d\n", rc);
        return 3;
    }
    f = fopen(argv[5], "wb");
    if (!f || fwrite(o, 4, n, f) != n) return 4;
    fclose(f);
    free(p); free(t); free(g); free(o);
    return 0;
}
