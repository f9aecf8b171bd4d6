// Runs the entry points of a host-compiled copy of csrc/pointwise.hip (common.h's ADH_HOST_EMU_STREAM section; the script format
// is stream_rt.h's).  tests/test_pointwise_hostemu_cpu.py builds it twice: as the library is built, and with the grid caps
// (PW_MAXBLK_*, RED_ELEMS_PER_BLOCK) set small, so that every grid-stride loop makes several trips at a few hundred elements.
// Calls, with their integers `i`, doubles `d` and buffers `b` in order (a buffer index of -1 is a null pointer):
//    0 adh_version
//    1 adh_image_to_nhwc8             i: N H W                                   b: img out
//    2 adh_image_normalize_to_nhwc8   i: N H W                  d: m0 m1 m2 is0 is1 is2   b: img out
//    3 adh_image_normalize_bwd        i: g_cs N H W             d: is0 is1 is2   b: g g_img
//    4 adh_nchw_to_nhwc               i: N C H W dst_cs                          b: src dst
//    5 adh_nhwc_to_nchw               i: src_cs N C H W                          b: src dst
//    6 adh_head_blend                 i: mode r_cs gd_cs N H W                   b: x r gd alpha out
//    7 adh_head_blend_bwd_num_blocks  i: N H W
//    8 adh_head_blend_bwd             i: mode r_cs gd_cs N H W nblk              b: g x r gd alpha g_r g_gd galpha_partial
//    9 adh_softmax3                   i: N                      d: temperature   b: logits weights
//   10 adh_softmax3_bwd               i: nblk N                 d: temperature   b: weights gw_partial g_logits
//   11 adh_soft_blend                 i: N per                                   b: weights o0 o1 o2 out
//   12 adh_soft_blend_bwd             i: N per nblk                              b: weights g o0 o1 o2 g0 g1 g2 gw_partial
//   13 adh_argmax3                    i: N                                       b: logits idx
//   14 adh_route_compact              i: N                                       b: idx sel counts
//   15 adh_gather_images              i: count per                               b: src sel dst
//   16 adh_scatter_images             i: count per                               b: src sel dst
//   17 adh_reduce_num_blocks          i: n
//   18 adh_l1_partial                 i: n                                       b: a b partial
//   19 adh_mse_partial                i: n                                       b: a b partial
//   20 adh_sum_partials               i: nblk                   d: scale         b: partial out
//   21 adh_l1_bwd                     i: n                      d: gscale        b: a b upstream g_a
//   22 adh_mse_bwd                    i: n                      d: gscale        b: a b upstream g_a
//   23 adh_cross_entropy3             i: N                                       b: logits labels loss dlogits
//   24 adh_adam_step                  i: n step repeats         d: lr beta1 beta2 eps weight_decay   b: p g m v
//   25 adh_add_inplace                i: n                                       b: dst src
//   26 adh_axpby_strided              i: dst_cs src_cs P C      d: a b           b: dst src
//   27 adh_maxpool                    i: x_cs N H W C k stride pad out_cs        b: x out idx
//   28 adh_maxpool_bwd                i: g_cs N OH OW C k stride pad H W gx_cs   b: g idx gx
//   29 adh_avgpool                    i: x_cs N H W C k out_cs                   b: x out
//   30 adh_global_avgpool_bwd         i: N HW C gx_cs                            b: g gx
//   31 adh_mul                        i: n                                       b: dst a b
//   32 adh_bilinear                   i: x_cs N H W C OH OW align out_cs         b: x out
//   33 adh_bilinear_bwd               i: g_cs N H W C OH OW align gx_cs          b: g gx
#include "common.h"
#include "stream_rt.h"

static int64_t dispatch(const emu_call& c) {
    typedef int32_t i32;
    typedef int64_t i64;
    auto F = [&](int k) { return (float)c.d[k]; };
    switch (c.fn) {
        case 0: return adh_version();
        case 1: return adh_image_to_nhwc8(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.f(1));
        case 2: return adh_image_normalize_to_nhwc8(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), F(0), F(1), F(2), F(3), F(4), F(5), c.f(1));
        case 3: return adh_image_normalize_bwd(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.I(3), F(0), F(1), F(2), c.f(1));
        case 4: return adh_nchw_to_nhwc(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.I(3), c.f(1), c.I(4));
        case 5: return adh_nhwc_to_nchw(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.I(3), c.I(4), c.f(1));
        case 6: return adh_head_blend(nullptr, c.I(0), c.f(0), c.f(1), c.I(1), c.f(2), c.I(2), c.f(3), c.I(3), c.I(4), c.I(5), c.f(4));
        case 7: return adh_head_blend_bwd_num_blocks(c.I(0), c.I(1), c.I(2));
        case 8:
            return adh_head_blend_bwd(nullptr, c.I(0), c.f(0), c.f(1), c.f(2), c.I(1), c.f(3), c.I(2), c.f(4), c.I(3), c.I(4), c.I(5),
                                      c.f(5), c.f(6), c.f(7), c.I(6));
        case 9: return adh_softmax3(nullptr, c.f(0), F(0), c.I(0), c.f(1));
        case 10: return adh_softmax3_bwd(nullptr, c.f(0), c.f(1), c.I(0), F(0), c.I(1), c.f(2));
        case 11: return adh_soft_blend(nullptr, c.f(0), c.f(1), c.f(2), c.f(3), c.I(0), c.i[1], c.f(4));
        case 12:
            return adh_soft_blend_bwd(nullptr, c.f(0), c.f(1), c.f(2), c.f(3), c.f(4), c.I(0), c.i[1], c.f(5), c.f(6), c.f(7), c.f(8),
                                      c.I(2));
        case 13: return adh_argmax3(nullptr, c.f(0), c.I(0), c.p<i64>(1));
        case 14: return adh_route_compact(nullptr, c.p<i64>(0), c.I(0), c.p<i32>(1), c.p<i32>(2));
        case 15: return adh_gather_images(nullptr, c.f(0), c.p<i32>(1), c.I(0), c.i[1], c.f(2));
        case 16: return adh_scatter_images(nullptr, c.f(0), c.p<i32>(1), c.I(0), c.i[1], c.f(2));
        case 17: return adh_reduce_num_blocks(c.i[0]);
        case 18: return adh_l1_partial(nullptr, c.f(0), c.f(1), c.i[0], c.f(2));
        case 19: return adh_mse_partial(nullptr, c.f(0), c.f(1), c.i[0], c.f(2));
        case 20: return adh_sum_partials(nullptr, c.f(0), c.I(0), c.d[0], c.f(1));
        case 21: return adh_l1_bwd(nullptr, c.f(0), c.f(1), c.i[0], F(0), c.f(2), c.f(3));
        case 22: return adh_mse_bwd(nullptr, c.f(0), c.f(1), c.i[0], F(0), c.f(2), c.f(3));
        case 23: return adh_cross_entropy3(nullptr, c.f(0), c.p<i64>(1), c.I(0), c.f(2), c.f(3));
        case 24: return adh_adam_step(nullptr, c.f(0), c.f(1), c.f(2), c.f(3), c.i[0], c.I(1), F(0), F(1), F(2), F(3), F(4), c.I(2));
        case 25: return adh_add_inplace(nullptr, c.f(0), c.f(1), c.i[0]);
        case 26: return adh_axpby_strided(nullptr, c.f(0), c.I(0), c.f(1), c.I(1), c.i[2], c.I(3), F(0), F(1));
        case 27:
            return adh_maxpool(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.I(3), c.I(4), c.I(5), c.I(6), c.I(7), c.f(1), c.I(8),
                               c.p<i32>(2));
        case 28:
            return adh_maxpool_bwd(nullptr, c.f(0), c.I(0), c.p<i32>(1), c.I(1), c.I(2), c.I(3), c.I(4), c.I(5), c.I(6), c.I(7), c.I(8),
                                   c.I(9), c.f(2), c.I(10));
        case 29: return adh_avgpool(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.I(3), c.I(4), c.I(5), c.f(1), c.I(6));
        case 30: return adh_global_avgpool_bwd(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.f(1), c.I(3));
        case 31: return adh_mul(nullptr, c.f(0), c.f(1), c.f(2), c.i[0]);
        case 32:
            return adh_bilinear(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.I(3), c.I(4), c.I(5), c.I(6), c.I(7), c.f(1), c.I(8));
        case 33:
            return adh_bilinear_bwd(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.I(3), c.I(4), c.I(5), c.I(6), c.I(7), c.f(1), c.I(8));
    }
    return -1000;
}

int main(int argc, char** argv) { return emu_run_script(argc, argv, dispatch); }
