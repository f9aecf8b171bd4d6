// Runs adh_wgrad_reduce_small of a host-compiled copy of csrc/conv_wgrad_reduce.hip on the streaming runtime (stream_rt.cpp: its
// lanes and launch; the script format is stream_rt.h's) -- the second program of tests/test_wgrad_reduce_hostemu_cpu.py, next to
// wgrad_reduce_main.cpp, which runs the other entry points one call a process.
//   0 adh_wgrad_reduce_small   i: nslabs KP NcP accumulate, then the nine fields of adh_wlayout   b: slab dst
#include "common.h"
#include "stream_rt.h"

// conv_wgrad32.hip's; adh_wgrad_reduce_wino32 is not called here
int adh_wgrad32_class_taps(const adh_conv_desc*, adh_wg32_taps*) { return 0; }

static int64_t dispatch(const emu_call& c) {
    if (c.fn != 0) return -1000;
    const adh_wlayout L = {c.I(4), c.I(5), c.I(6), c.I(7), c.I(8), c.I(9), c.I(10), c.I(11), c.I(12)};
    return adh_wgrad_reduce_small(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), &L, c.f(1), c.I(3));
}

int main(int argc, char** argv) { return emu_run_script(argc, argv, dispatch); }
