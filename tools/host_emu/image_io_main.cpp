// Runs the entry points of a host-compiled copy of csrc/image_io.hip (common.h's ADH_HOST_EMU_STREAM section; the script format
// is stream_rt.h's).  Calls, with their integers `i` and buffers `b` in order:
//   0 adh_u8_to_image   i: row_pitch image_pitch N H W C      b: src dst_nchw
//   1 adh_image_to_u8   i: N H W row_pitch image_pitch C      b: src_nchw dst
#include "common.h"
#include "stream_rt.h"

static int64_t dispatch(const emu_call& c) {
    switch (c.fn) {
        case 0: return adh_u8_to_image(nullptr, c.p<uint8_t>(0), c.i[0], c.i[1], c.I(2), c.I(3), c.I(4), c.I(5), c.f(1));
        case 1: return adh_image_to_u8(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.p<uint8_t>(1), c.i[3], c.i[4], c.I(5));
    }
    return -1000;
}

int main(int argc, char** argv) { return emu_run_script(argc, argv, dispatch); }
