// Runs the entry points of a host-compiled copy of csrc/ciede2000.hip (common.h's ADH_HOST_EMU_STREAM section; the script format
// is stream_rt.h's).  The kernels reduce through LDS and barriers only, so they need nothing of the emulation beyond what the
// streaming files take.  Calls, with their integers `i` and buffers `b` in order:
//   0 adh_ciede2000             i: N H W lab_input nblk      b: pred target partial map mean     (map may be -1: NULL)
//   1 adh_ciede2000_num_blocks  i: pixels
#include "common.h"
#include "stream_rt.h"

static int64_t dispatch(const emu_call& c) {
    switch (c.fn) {
        case 0:
            return adh_ciede2000(nullptr, c.f(0), c.f(1), c.I(0), c.I(1), c.I(2), c.I(3), c.p<double>(2), c.I(4), c.f(3), c.f(4));
        case 1: return adh_ciede2000_num_blocks(c.i[0]);
    }
    return -1000;
}

int main(int argc, char** argv) { return emu_run_script(argc, argv, dispatch); }
