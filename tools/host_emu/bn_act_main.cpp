// Runs the entry points of a host-compiled copy of csrc/bn_act.hip (common.h's ADH_HOST_EMU_STREAM section; the script format
// is stream_rt.h's).  Calls, with their integers `i`, doubles `d` and buffers `b` in order:
//   0 adh_bn_finalize               i: nblk NcP C        d: count eps momentum
//                                   b: partials gamma beta running_mean running_var scale shift save_mean save_invstd nbt
//   1 adh_bn_partial_sums           i: nblk pitch C      d: count        b: partials sums
//   2 adh_bn_finalize_sums          i: C                 d: eps momentum
//                                   b: sums gamma beta running_mean running_var scale shift save_mean save_invstd nbt
//   3 adh_bn_bwd_finalize_sums      i: C accumulate                      b: local_sums global_sums gamma invstd dgamma dbeta coef
//   4 adh_bn_fold_eval              i: C                 d: eps          b: gamma beta running_mean running_var conv_bias scale shift
//   5 adh_bn_apply                  i: y_cs res_cs act out_cs P C        b: y scale shift residual out mask_bits
//   6 adh_bn_bwd_num_blocks         i: P C
//   7 adh_bn_bwd_reduce             i: g_cs out_cs act y_cs P C          b: g_out out y mean invstd partials mask_ss mask_bits
//   8 adh_bn_bwd_finalize           i: nblk C accumulate d: count        b: partials gamma invstd dgamma dbeta coef
//   9 adh_bn_bwd_finalize_centered  i: nblk pitch C accumulate  d: count b: partials gamma invstd dgamma dbeta coef
//  10 adh_bn_bwd_apply              i: g_cs out_cs act y_cs training gy_cs gres_cs P C
//                                   b: g_out out y mean invstd coef g_y g_res mask_ss mask_bits
#include "common.h"
#include "stream_rt.h"

static int64_t dispatch(const emu_call& c) {
    switch (c.fn) {
        case 0:
            return adh_bn_finalize(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.d[0], c.f(1), c.f(2), (float)c.d[1], (float)c.d[2],
                                   c.f(3), c.f(4), c.f(5), c.f(6), c.f(7), c.f(8), c.p<int64_t>(9));
        case 1: return adh_bn_partial_sums(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.d[0], c.p<double>(1));
        case 2:
            return adh_bn_finalize_sums(nullptr, c.p<double>(0), c.I(0), c.f(1), c.f(2), (float)c.d[0], (float)c.d[1], c.f(3),
                                        c.f(4), c.f(5), c.f(6), c.f(7), c.f(8), c.p<int64_t>(9));
        case 3:
            return adh_bn_bwd_finalize_sums(nullptr, c.p<double>(0), c.p<double>(1), c.I(0), c.f(2), c.f(3), c.f(4), c.f(5),
                                            c.I(1), c.f(6));
        case 4: return adh_bn_fold_eval(nullptr, c.I(0), c.f(0), c.f(1), c.f(2), c.f(3), (float)c.d[0], c.f(4), c.f(5), c.f(6));
        case 5:
            return adh_bn_apply(nullptr, c.f(0), c.I(0), c.f(1), c.f(2), c.f(3), c.I(1), c.I(2), c.f(4), c.I(3), c.i[4], c.I(5),
                                c.p<uint8_t>(5));
        case 6: return adh_bn_bwd_num_blocks(c.i[0], c.I(1));
        case 7:
            return adh_bn_bwd_reduce(nullptr, c.f(0), c.I(0), c.f(1), c.I(1), c.I(2), c.f(2), c.I(3), c.f(3), c.f(4), c.f(5),
                                     c.i[4], c.I(5), c.f(6), c.p<uint8_t>(7));
        case 8:
            return adh_bn_bwd_finalize(nullptr, c.f(0), c.I(0), c.I(1), c.d[0], c.f(1), c.f(2), c.f(3), c.f(4), c.I(2), c.f(5));
        case 9:
            return adh_bn_bwd_finalize_centered(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.d[0], c.f(1), c.f(2), c.f(3), c.f(4),
                                                c.I(3), c.f(5));
        case 10:
            return adh_bn_bwd_apply(nullptr, c.f(0), c.I(0), c.f(1), c.I(1), c.I(2), c.f(2), c.I(3), c.f(3), c.f(4), c.f(5),
                                    c.I(4), c.f(6), c.I(5), c.f(7), c.I(6), c.i[7], c.I(8), c.f(8), c.p<uint8_t>(9));
    }
    return -1000;
}

int main(int argc, char** argv) { return emu_run_script(argc, argv, dispatch); }
