// Runs the entry points of a host-compiled copy of csrc/lpips.hip (common.h's ADH_HOST_EMU_STREAM section; the script format is
// stream_rt.h's).  Calls, with their integers `i`, doubles `d` and buffers `b` in order:
//   0 adh_lpips_s2d               i: N H W OHp OWp     d: a0 a1 a2 b0 b1 b2    b: img out
//   1 adh_lpips_s2d_bwd           i: N H W OHp OWp     d: a0 a1 a2             b: g g_img
//   2 adh_lpips_layer_num_blocks  i: HW
//   3 adh_lpips_layer             i: N HW C nblk                               b: fa fb w partial
//   4 adh_lpips_layer_bwd         i: N HW C                                    b: fa fb w g_val g_fa
//   5 adh_rows_sum                i: N nblk accumulate d: scale                b: partial out
#include "common.h"
#include "stream_rt.h"

static int64_t dispatch(const emu_call& c) {
    float a3[3] = {0.f, 0.f, 0.f}, b3[3] = {0.f, 0.f, 0.f};
    for (size_t k = 0; k < 3 && k < c.d.size(); ++k) a3[k] = (float)c.d[k];
    for (size_t k = 3; k < 6 && k < c.d.size(); ++k) b3[k - 3] = (float)c.d[k];
    switch (c.fn) {
        case 0: return adh_lpips_s2d(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), a3, b3, c.I(3), c.I(4), c.f(1));
        case 1: return adh_lpips_s2d_bwd(nullptr, c.f(0), c.I(0), c.I(1), c.I(2), a3, c.I(3), c.I(4), c.f(1));
        case 2: return adh_lpips_layer_num_blocks(c.I(0));
        case 3: return adh_lpips_layer(nullptr, c.f(0), c.f(1), c.f(2), c.I(0), c.I(1), c.I(2), c.f(3), c.I(3));
        case 4: return adh_lpips_layer_bwd(nullptr, c.f(0), c.f(1), c.f(2), c.f(3), c.I(0), c.I(1), c.I(2), c.f(4));
        case 5: return adh_rows_sum(nullptr, c.f(0), c.I(0), c.I(1), (float)c.d[0], c.f(1), c.I(2));
    }
    return -1000;
}

int main(int argc, char** argv) { return emu_run_script(argc, argv, dispatch); }
