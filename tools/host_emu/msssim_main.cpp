// Runs the entry points of a host-compiled copy of csrc/msssim.hip (common.h's ADH_HOST_EMU_STREAM section; the script format is
// stream_rt.h's).  The kernels stage, filter and reduce through static LDS arrays and barriers only.  Calls, with their integers
// `i`, doubles `d` and buffers `b` in order (a buffer index of -1 is a null pointer):
//   0 adh_msssim_level_fwd  i: in_f64 N H W ntiles     d: data_range  b: pred target partial ssim cs pool_pred pool_target
//   1 adh_msssim_level_bwd  i: in_f64 N H W out_f64    d: data_range  b: pred target coef_a coef_b g_coarse g_out
//   2 adh_msssim_num_tiles  i: H W
#include "common.h"
#include "stream_rt.h"

static int64_t dispatch(const emu_call& c) {
    switch (c.fn) {
        case 0:
            return adh_msssim_level_fwd(nullptr, c.p<void>(0), c.p<void>(1), c.I(0), c.I(1), c.I(2), c.I(3), c.d[0], c.p<double>(2),
                                        c.I(4), c.p<double>(3), c.p<double>(4), c.p<double>(5), c.p<double>(6));
        case 1:
            return adh_msssim_level_bwd(nullptr, c.p<void>(0), c.p<void>(1), c.I(0), c.I(1), c.I(2), c.I(3), c.d[0], c.p<double>(2),
                                        c.p<double>(3), c.p<double>(4), c.p<void>(5), c.I(4));
        case 2: return adh_msssim_num_tiles(c.I(0), c.I(1));
    }
    return -1000;
}

int main(int argc, char** argv) { return emu_run_script(argc, argv, dispatch); }
