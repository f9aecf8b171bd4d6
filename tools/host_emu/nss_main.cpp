// Runs the entry points of a host-compiled copy of csrc/nss.hip (common.h's ADH_HOST_EMU_STREAM section; the script format is
// stream_rt.h's).  The kernels stage and reduce through static LDS arrays and barriers only.  Calls, with their integers `i` and
// buffers `b` in order (a buffer index of -1 is a null pointer):
//   0 adh_nss_halve    i: src_rgb N H W Hc Wc                b: src dst
//   1 adh_nss_moments  i: src_rgb N H W Hc Wc rh rw ntiles   b: src partial out
#include "common.h"
#include "stream_rt.h"

static int64_t dispatch(const emu_call& c) {
    switch (c.fn) {
        case 0: return adh_nss_halve(nullptr, c.p<void>(0), c.I(0), c.I(1), c.I(2), c.I(3), c.I(4), c.I(5), c.p<double>(1));
        case 1:
            return adh_nss_moments(nullptr, c.p<void>(0), c.I(0), c.I(1), c.I(2), c.I(3), c.I(4), c.I(5), c.I(6), c.I(7),
                                   c.p<double>(1), c.I(8), c.p<double>(2));
    }
    return -1000;
}

int main(int argc, char** argv) { return emu_run_script(argc, argv, dispatch); }
