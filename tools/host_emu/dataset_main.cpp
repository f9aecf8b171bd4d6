// Runs the entry points of a host-compiled copy of csrc/dataset.hip (common.h's ADH_HOST_EMU_STREAM section: the float64
// butterfly of the grey-mean pass runs on the emulator's __shfl_xor(double); the script format is stream_rt.h's).
// Calls, with their integers `i`, doubles `d` and buffers `b` in order (a buffer index of -1 is a null pointer):
//   0 adh_u8_resize_bilinear   i: row_pitch H W C OH OW                     b: src dst
//   1 adh_batch_num_blocks     i: HW
//   2 adh_batch_from_u8        i: image_pitch M H W N nblk                  b: cache index params partial out
//   3 adh_batch_window_from_u8 i: cache_bytes N CH CW nblk                  b: cache window params partial out
//   4 adh_u16_resize_bilinear  i: src_pitch_bytes h w bytes_per_px OH OW    b: src dst
//   5 adh_batch_haze_from_u8   i: clear_bytes depth_bytes N CH CW nblk      d: depth_near depth_far
//                                                                           b: clear depth geom fog params partial out
//   6 adh_batch_nhhaze_from_u8 i: clear_bytes depth_bytes N CH CW nblk      d: depth_near depth_far
//                                                                           b: clear depth geom fog field params partial out
#include "common.h"
#include "stream_rt.h"

static int64_t dispatch(const emu_call& c) {
    switch (c.fn) {
        case 0: return adh_u8_resize_bilinear(nullptr, c.p<uint8_t>(0), c.i[0], c.I(1), c.I(2), c.I(3), c.p<uint8_t>(1), c.I(4), c.I(5));
        case 1: return adh_batch_num_blocks(c.i[0]);
        case 2:
            return adh_batch_from_u8(nullptr, c.p<uint8_t>(0), c.i[0], c.i[1], c.I(2), c.I(3), c.p<int64_t>(1), c.f(2), c.I(4),
                                     c.p<double>(3), c.I(5), c.f(4));
        case 3:
            return adh_batch_window_from_u8(nullptr, c.p<uint8_t>(0), c.i[0], c.p<int64_t>(1), c.f(2), c.I(1), c.I(2), c.I(3),
                                            c.p<double>(3), c.I(4), c.f(4));
        case 4:
            return adh_u16_resize_bilinear(nullptr, c.p<uint8_t>(0), c.i[0], c.I(1), c.I(2), c.I(3), c.p<void>(1), c.I(4), c.I(5));
        case 5:
            return adh_batch_haze_from_u8(nullptr, c.p<uint8_t>(0), c.i[0], c.p<void>(1), c.i[1], c.p<int64_t>(2), c.f(3), c.d[0],
                                          c.d[1], c.f(4), c.I(2), c.I(3), c.I(4), c.p<double>(5), c.I(5), c.f(6));
        case 6:
            return adh_batch_nhhaze_from_u8(nullptr, c.p<uint8_t>(0), c.i[0], c.p<void>(1), c.i[1], c.p<int64_t>(2), c.f(3),
                                            c.p<double>(4), c.d[0], c.d[1], c.f(5), c.I(2), c.I(3), c.I(4), c.p<double>(6), c.I(5),
                                            c.f(7));
    }
    return -1000;
}

int main(int argc, char** argv) { return emu_run_script(argc, argv, dispatch); }
