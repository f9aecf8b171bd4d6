// Runs the entry point of a host-compiled copy of csrc/overlay.hip (common.h's ADH_HOST_EMU_STREAM section; the script format is
// stream_rt.h's).  Calls, with their integers `i` and buffers `b` in order:
//   0 adh_draw_boxes   i: row_pitch image_pitch N H W C M T G thickness scale alpha      b: img first boxes colors text glyphs
#include "common.h"
#include "stream_rt.h"

static int64_t dispatch(const emu_call& c) {
    switch (c.fn) {
        case 0:
            return adh_draw_boxes(nullptr, c.p<uint8_t>(0), c.i[0], c.i[1], c.I(2), c.I(3), c.I(4), c.I(5), c.p<int32_t>(1), c.I(6),
                                  c.f(2), c.p<uint8_t>(3), c.p<void>(4), c.I(7), c.p<uint8_t>(5), c.I(8), c.I(9), c.I(10), c.I(11));
    }
    return -1000;
}

int main(int argc, char** argv) { return emu_run_script(argc, argv, dispatch); }
