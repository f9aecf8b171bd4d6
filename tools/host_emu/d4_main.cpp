// Runs the entry point of a host-compiled copy of csrc/d4.hip (common.h's ADH_HOST_EMU_STREAM section; the script format is
// stream_rt.h's).  Calls, with their integers `i`, doubles `d` and buffers `b` in order:
//   0 adh_d4_apply   i: N C H W transpose flips accumulate      d: scale      b: src flip_ops dst
//   1 adh_d4_apply   i: N C H W transpose flips accumulate shift      d: scale      b: block
//     src and dst inside one block, dst `shift` floats behind src (shift < 0: in front of it; the earlier one is the block's start)
#include "common.h"
#include "stream_rt.h"

static int64_t dispatch(const emu_call& c) {
    switch (c.fn) {
        case 0:
            return adh_d4_apply(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.I(3), c.I(4), c.I(5), c.p<int32_t>(1), c.f(2), c.I(6),
                                (float)c.d[0]);
        case 1: {
            float* src = c.f(0) + (c.i[7] < 0 ? -c.i[7] : 0);
            float* dst = c.f(0) + (c.i[7] > 0 ? c.i[7] : 0);
            return adh_d4_apply(nullptr, src, c.I(0), c.I(1), c.I(2), c.I(3), c.I(4), c.I(5), nullptr, dst, c.I(6), (float)c.d[0]);
        }
    }
    return -1000;
}

int main(int argc, char** argv) { return emu_run_script(argc, argv, dispatch); }
