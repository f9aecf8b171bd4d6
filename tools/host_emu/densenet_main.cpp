// Runs the entry points of a host-compiled copy of csrc/densenet.hip (common.h's ADH_HOST_EMU_STREAM section; the script
// format is stream_rt.h's).  Calls, with their integers `i`, doubles `d` and buffers `b` in order:
//   0 adh_bn_slice_stats_num_blocks  i: P C
//   1 adh_bn_slice_stats             i: x_cs P C                          b: x partials
//   2 adh_bn_slice_moments           i: nblk pitch C    d: count          b: partials mean var
//   3 adh_bn_fold_moments            i: C               d: count eps momentum
//                                    b: mean var gamma beta running_mean running_var scale shift save_mean save_invstd nbt
//   4 adh_avgpool2_bwd               i: g_cs N H W C gx_cs accumulate     b: g gx
//   5 adh_bn_preact_bwd_accum        i: dA_cs x_cs training dbuf_cs P C accumulate  b: dA x ss mean invstd coef dbuf
#include "common.h"
#include "stream_rt.h"

static int64_t dispatch(const emu_call& c) {
    switch (c.fn) {
        case 0: return adh_bn_slice_stats_num_blocks(c.i[0], c.I(1));
        case 1: return adh_bn_slice_stats(nullptr, c.f(0), c.I(0), c.i[1], c.I(2), c.f(1));
        case 2: return adh_bn_slice_moments(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.d[0], c.p<double>(1), c.p<double>(2));
        case 3:
            return adh_bn_fold_moments(nullptr, c.I(0), c.p<double>(0), c.p<double>(1), c.d[0], c.f(2), c.f(3), (float)c.d[1],
                                       (float)c.d[2], c.f(4), c.f(5), c.f(6), c.f(7), c.f(8), c.f(9), c.p<int64_t>(10));
        case 4: return adh_avgpool2_bwd(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.I(3), c.I(4), c.f(1), c.I(5), c.I(6));
        case 5:
            return adh_bn_preact_bwd_accum(nullptr, c.f(0), c.I(0), c.f(1), c.I(1), c.f(2), c.f(3), c.f(4), c.f(5), c.I(2),
                                           c.f(6), c.I(3), c.i[4], c.I(5), c.I(6));
    }
    return -1000;
}

int main(int argc, char** argv) { return emu_run_script(argc, argv, dispatch); }
