// Runs the entry points of a host-compiled copy of csrc/cbam.hip (common.h's ADH_HOST_EMU_STREAM section; the script format is
// stream_rt.h's).  Calls, with their integers `i` and buffers `b` in order:
//   0 adh_cbam_pool_num_blocks       i: HW
//   1 adh_cbam_pool                  i: x_cs N HW C nblk              b: x partial partial_idx pooled amax_idx
//   2 adh_cbam_mlp                   i: N C Ch                        b: pooled w1 w2 ca hidden
//   3 adh_cbam_spatial_stats         i: x_cs N HW C                   b: x ca smap cidx
//   4 adh_cbam_apply                 i: x_cs N H W C out_cs           b: x ca smap wsp sa out
//   5 adh_cbam_bwd_a                 i: g_cs x_cs N HW C              b: g x ca sa gsa_pre
//   6 adh_cbam_bwd_b_num_blocks      i: N H W
//   7 adh_cbam_bwd_b                 i: N H W nblk accumulate         b: gsa_pre smap wsp gsmap dwsp_partial dwsp
//   8 adh_cbam_bwd_c                 i: g_cs x_cs N HW C nblk         b: g x sa gsmap cidx gca_partial
//   9 adh_cbam_bwd_d_scratch_floats  i: N C Ch
//  10 adh_cbam_bwd_d                 i: nblk N C Ch accumulate        b: gca_partial ca pooled hidden w1 w2 gpool dw1 dw2 scratch
//  11 adh_cbam_bwd_e                 i: g_cs x_cs N HW C gx_cs        b: g x ca sa gsmap cidx gpool amax_idx gx
#include "common.h"
#include "stream_rt.h"

static int64_t dispatch(const emu_call& c) {
    typedef int32_t i32;
    switch (c.fn) {
        case 0: return adh_cbam_pool_num_blocks(c.I(0));
        case 1:
            return adh_cbam_pool(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.I(3), c.f(1), c.p<i32>(2), c.I(4), c.f(3), c.p<i32>(4));
        case 2: return adh_cbam_mlp(nullptr, c.f(0), c.f(1), c.f(2), c.I(0), c.I(1), c.I(2), c.f(3), c.f(4));
        case 3: return adh_cbam_spatial_stats(nullptr, c.f(0), c.I(0), c.f(1), c.I(1), c.I(2), c.I(3), c.f(2), c.p<i32>(3));
        case 4:
            return adh_cbam_apply(nullptr, c.f(0), c.I(0), c.f(1), c.f(2), c.f(3), c.I(1), c.I(2), c.I(3), c.I(4), c.f(4), c.f(5),
                                  c.I(5));
        case 5: return adh_cbam_bwd_a(nullptr, c.f(0), c.I(0), c.f(1), c.I(1), c.f(2), c.f(3), c.I(2), c.I(3), c.I(4), c.f(4));
        case 6: return adh_cbam_bwd_b_num_blocks(c.I(0), c.I(1), c.I(2));
        case 7:
            return adh_cbam_bwd_b(nullptr, c.f(0), c.f(1), c.f(2), c.I(0), c.I(1), c.I(2), c.f(3), c.f(4), c.I(3), c.f(5), c.I(4));
        case 8:
            return adh_cbam_bwd_c(nullptr, c.f(0), c.I(0), c.f(1), c.I(1), c.f(2), c.f(3), c.p<i32>(4), c.I(2), c.I(3), c.I(4),
                                  c.f(5), c.I(5));
        case 9: return adh_cbam_bwd_d_scratch_floats(c.I(0), c.I(1), c.I(2));
        case 10:
            return adh_cbam_bwd_d(nullptr, c.f(0), c.I(0), c.f(1), c.f(2), c.f(3), c.f(4), c.f(5), c.I(1), c.I(2), c.I(3), c.f(6),
                                  c.f(7), c.f(8), c.I(4), c.f(9));
        case 11:
            return adh_cbam_bwd_e(nullptr, c.f(0), c.I(0), c.f(1), c.I(1), c.f(2), c.f(3), c.f(4), c.p<i32>(5), c.f(6), c.p<i32>(7),
                                  c.I(2), c.I(3), c.I(4), c.f(8), c.I(5));
    }
    return -1000;
}

int main(int argc, char** argv) { return emu_run_script(argc, argv, dispatch); }
