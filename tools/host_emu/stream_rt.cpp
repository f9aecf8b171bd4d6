// Runtime shared by the streaming drivers (built with -DADH_HOST_EMU -DADH_HOST_EMU_STREAM): the emulator's globals, an
// emu_launch that walks all three grid dimensions, the shuffle channels, the dynamic-LDS pointer, and the script reader of
// stream_rt.h.
#include "common.h"
#include "stream_rt.h"
#include <condition_variable>
#include <cstring>
#include <mutex>
thread_local dim3 threadIdx;
dim3 blockIdx, gridDim, blockDim;
pthread_barrier_t emu_barrier;
void* emu_dyn_lds;

// The lanes are a pool of OS threads kept over the launches of a script (a script makes hundreds of launches, and starting 256
// threads under the sanitizers costs more than most of these kernels): a launch publishes its job under a new generation
// number, lanes t < block.x run it, and the last one to finish wakes the launcher.
static std::mutex pool_mu;
static std::condition_variable pool_go, pool_done;
static std::vector<std::thread> pool;
static unsigned pool_gen, pool_lanes, pool_left;
static bool pool_quit;
static const std::function<void()>* pool_fn;

// block.x lanes walk the workgroups of the launch together (two barriers per workgroup), x fastest
static void lane_main(unsigned t) {
    unsigned seen = 0;
    for (;;) {
        {
            std::unique_lock<std::mutex> lk(pool_mu);
            pool_go.wait(lk, [&] { return pool_quit || pool_gen != seen; });
            if (pool_quit) return;
            seen = pool_gen;
            if (t >= pool_lanes) continue;
        }
        threadIdx = dim3(t);
        const dim3 grid = gridDim;
        for (unsigned z = 0; z < grid.z; ++z)
            for (unsigned y = 0; y < grid.y; ++y)
                for (unsigned x = 0; x < grid.x; ++x) {
                    if (t == 0) blockIdx = dim3(x, y, z);
                    __syncthreads();
                    (*pool_fn)();
                    __syncthreads();
                }
        std::lock_guard<std::mutex> lk(pool_mu);
        if (--pool_left == 0) pool_done.notify_one();
    }
}

void emu_launch(dim3 grid, dim3 block, std::function<void()> fn) {
    if (block.x < 1 || block.x > 1024 || block.y != 1 || block.z != 1) exit(6);
    gridDim = grid;
    blockDim = block;
    for (unsigned t = 0; t < block.x; ++t)
        for (auto& ch : emu_chan[t]) ch.seq.store(0, std::memory_order_relaxed);
    pthread_barrier_init(&emu_barrier, nullptr, block.x);
    std::unique_lock<std::mutex> lk(pool_mu);
    while (pool.size() < block.x) {
        const unsigned t = (unsigned)pool.size();
        pool.emplace_back(lane_main, t);
    }
    pool_fn = &fn;
    pool_lanes = pool_left = block.x;
    ++pool_gen;
    pool_go.notify_all();
    pool_done.wait(lk, [] { return pool_left == 0; });
    lk.unlock();
    pthread_barrier_destroy(&emu_barrier);
}

void emu_shutdown() {
    {
        std::lock_guard<std::mutex> lk(pool_mu);
        pool_quit = true;
    }
    pool_go.notify_all();
    for (auto& t : pool) t.join();
    pool.clear();
}

static int64_t rd(FILE* f) {
    int64_t v;
    if (fread(&v, 8, 1, f) != 1) exit(2);
    return v;
}

int emu_run_script(int argc, char** argv, int64_t (*dispatch)(const emu_call&)) {
    if (argc != 3) return 1;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const int64_t nbuf = rd(f);
    std::vector<char*> block(nbuf);
    std::vector<int64_t> bytes(nbuf), off(nbuf);
    for (int64_t k = 0; k < nbuf; ++k) {
        bytes[k] = rd(f);
        off[k] = rd(f);
        void* q = nullptr;
        if (posix_memalign(&q, 16, bytes[k] ? bytes[k] : 1)) return 5;
        block[k] = (char*)q;
        if (bytes[k] && fread(block[k], 1, bytes[k], f) != (size_t)bytes[k]) return 2;
    }
    const int64_t ncall = rd(f);
    std::vector<int64_t> rc;
    for (int64_t k = 0; k < ncall; ++k) {
        emu_call c;
        c.fn = (int)rd(f);
        c.i.resize(rd(f));
        for (auto& v : c.i) v = rd(f);
        c.d.resize(rd(f));
        for (auto& v : c.d)
            if (fread(&v, 8, 1, f) != 1) return 2;
        c.b.resize(rd(f));
        for (auto& v : c.b) {
            v = rd(f);
            if (v >= nbuf) return 2;
            c.ptr.push_back(v < 0 ? nullptr : block[v] + off[v]);
        }
        rc.push_back(dispatch(c));
    }
    fclose(f);
    emu_shutdown();
    f = fopen(argv[2], "wb");
    if (!f || fwrite(rc.data(), 8, rc.size(), f) != rc.size()) return 4;
    for (int64_t k = 0; k < nbuf; ++k) {
        if (bytes[k] && fwrite(block[k], 1, bytes[k], f) != (size_t)bytes[k]) return 4;
        free(block[k]);
    }
    fclose(f);
    return 0;
}
