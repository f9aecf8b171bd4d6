// Runs the entry points of a host-compiled copy of csrc/depthwise.hip (common.h's ADH_HOST_EMU_STREAM section; the script
// format is stream_rt.h's).  Calls, with their integers `i` and buffers `b` in order:
//   0 adh_dwconv_pack_weights        i: C k                                           b: w wp
//   1 adh_dwconv_num_blocks          i: P C
//   2 adh_dwconv_fwd                 i: x_cs N IH IW C k stride out_cs OH OW act      b: x wp out scale shift stats
//   3 adh_dwconv_dgrad               i: g_cs N OH OW C k stride gx_cs IH IW accumulate  b: g wp gx
//   4 adh_dwconv_wgrad_num_blocks    i: P C
//   5 adh_dwconv_wgrad               i: x_cs N IH IW C k stride g_cs OH OW nblk accumulate  b: x g partials dw
//   6 adh_channel_scale              i: x_cs N HW C out_cs                            b: x s out
//   7 adh_channel_scale_bwd_num_blocks  i: HW C
//   8 adh_channel_scale_bwd          i: g_cs x_cs N HW C gx_cs nblk                   b: g x s gx partials gs
#include "common.h"
#include "stream_rt.h"

static int64_t dispatch(const emu_call& c) {
    switch (c.fn) {
        case 0: {
            adh_wlayout L = {};
            L.Nc = c.I(0);
            L.KHt = L.KWt = c.I(1);
            return adh_dwconv_pack_weights(nullptr, c.f(0), &L, c.f(1));
        }
        case 1: return adh_dwconv_num_blocks(c.i[0], c.I(1));
        case 2:
            return adh_dwconv_fwd(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.I(3), c.I(4), c.I(5), c.I(6), c.f(1), c.f(2), c.I(7),
                                  c.I(8), c.I(9), c.f(3), c.f(4), c.I(10), c.f(5));
        case 3:
            return adh_dwconv_dgrad(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.I(3), c.I(4), c.I(5), c.I(6), c.f(1), c.f(2),
                                    c.I(7), c.I(8), c.I(9), c.I(10));
        case 4: return adh_dwconv_wgrad_num_blocks(c.i[0], c.I(1));
        case 5:
            return adh_dwconv_wgrad(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), c.I(3), c.I(4), c.I(5), c.I(6), c.f(1), c.I(7),
                                    c.I(8), c.I(9), c.f(2), c.I(10), c.f(3), c.I(11));
        case 6: return adh_channel_scale(nullptr, c.f(0), c.I(0), c.f(1), c.I(1), c.I(2), c.I(3), c.f(2), c.I(4));
        case 7: return adh_channel_scale_bwd_num_blocks(c.I(0), c.I(1));
        case 8:
            return adh_channel_scale_bwd(nullptr, c.f(0), c.I(0), c.f(1), c.I(1), c.f(2), c.I(2), c.I(3), c.I(4), c.f(3), c.I(5),
                                         c.f(4), c.I(6), c.f(5));
    }
    return -1000;
}

int main(int argc, char** argv) { return emu_run_script(argc, argv, dispatch); }
