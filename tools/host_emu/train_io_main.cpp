// Runs the entry points of a host-compiled copy of csrc/train_io.hip (common.h's ADH_HOST_EMU_STREAM section: the float64
// butterflies run on the emulator's __shfl_xor(double); the script format is stream_rt.h's).  tests/test_train_io_hostemu_cpu.py
// builds it twice: as the library is built, and with the grid caps (TIO_MAXBLK_PIXELS, PSNR_*, AUG_*) set small.
// Calls, with their integers `i`, doubles `d` and buffers `b` in order (a buffer index of -1 is a null pointer):
//    0 adh_adam_chunk_elems
//    1 adh_adam_multi          i: nt nchunks dup_mode max_repeats calls_since_upload, then TABLE
//                              d: lr beta1 beta2 eps weight_decay grad_scale        b: chunks, then p g m v per tensor
//    2 adh_grad_sumsq          i: nt nchunks, then TABLE          d: grad_scale      b: chunks partials, then p g m v per tensor
//    3 adh_grad_guard_finalize i: nchunks skip_nonfinite          d: grad_scale max_norm   b: partials ctrl
//    4 adh_adam_multi_guarded  i: nt nchunks dup_mode max_repeats calls_since_upload, then TABLE
//                              d: lr beta1 beta2 eps weight_decay                   b: chunks ctrl, then p g m v per tensor
//    5 adh_apply_fog           i: N H W                                             b: clear beta airlight hazy
//    6 adh_psnr_num_blocks     i: per_image
//    7 adh_psnr                i: N per_image nblk                d: data_range      b: pred target partial mse psnr
//    8 adh_ssim_num_blocks     i: H W
//    9 adh_ssim_gray           i: N H W nblk                      d: data_range      b: pred target partial ssim
//   10 adh_augment_num_blocks  i: HW
//   11 adh_paired_augment      i: N H W nblk                                        b: x params partial out
// TABLE is, per tensor, n step repeats and the float offsets of p g m v into their buffers (a buffer is a block of exactly
// offset + n floats: offset 1 puts the tensor off 16-byte alignment, the kernels' scalar path).  The adh_adam_tensor table itself
// is a heap block of exactly nt * sizeof(adh_adam_tensor) bytes for the length of the call (nt < 0: a null table).
#include "common.h"
#include "stream_rt.h"

struct adam_table {
    adh_adam_tensor* t = nullptr;
    adam_table(const emu_call& c, int i0, int b0) {
        const int nt = c.I(0);
        if (nt < 0) return;
        t = (adh_adam_tensor*)malloc(nt ? nt * sizeof(adh_adam_tensor) : 1);
        for (int k = 0; k < nt; ++k) {
            const int64_t* e = &c.i[i0 + 7 * k];
            t[k].p = c.f(b0 + 4 * k) + e[3];
            t[k].g = c.f(b0 + 4 * k + 1) + e[4];
            t[k].m = c.f(b0 + 4 * k + 2) + e[5];
            t[k].v = c.f(b0 + 4 * k + 3) + e[6];
            t[k].n = e[0];
            t[k].step = (int32_t)e[1];
            t[k].repeats = (int32_t)e[2];
        }
    }
    ~adam_table() { free(t); }
};

static int64_t dispatch(const emu_call& c) {
    typedef int32_t i32;
    auto F = [&](int k) { return (float)c.d[k]; };
    switch (c.fn) {
        case 0: return adh_adam_chunk_elems();
        case 1: {
            adam_table T(c, 5, 1);
            return adh_adam_multi(nullptr, T.t, c.p<i32>(0), c.I(1), F(0), F(1), F(2), F(3), F(4), F(5), c.I(2), c.I(3), c.I(4));
        }
        case 2: {
            adam_table T(c, 2, 2);
            return adh_grad_sumsq(nullptr, T.t, c.p<i32>(0), c.I(1), F(0), c.p<double>(1));
        }
        case 3: return adh_grad_guard_finalize(nullptr, c.p<double>(0), c.I(0), F(0), c.d[1], c.I(1), c.p<void>(1));
        case 4: {
            adam_table T(c, 5, 2);
            return adh_adam_multi_guarded(nullptr, T.t, c.p<i32>(0), c.I(1), F(0), F(1), F(2), F(3), F(4), c.I(2), c.I(3), c.I(4),
                                          c.p<void>(1));
        }
        case 5: return adh_apply_fog(nullptr, c.f(0), c.f(1), c.f(2), c.I(0), c.I(1), c.I(2), c.f(3));
        case 6: return adh_psnr_num_blocks(c.i[0]);
        case 7: return adh_psnr(nullptr, c.f(0), c.f(1), c.I(0), c.i[1], F(0), c.p<double>(2), c.I(2), c.f(3), c.f(4));
        case 8: return adh_ssim_num_blocks(c.I(0), c.I(1));
        case 9: return adh_ssim_gray(nullptr, c.f(0), c.f(1), c.I(0), c.I(1), c.I(2), F(0), c.p<double>(2), c.I(3), c.f(3));
        case 10: return adh_augment_num_blocks(c.i[0]);
        case 11: return adh_paired_augment(nullptr, c.f(0), c.f(1), c.I(0), c.I(1), c.I(2), c.p<double>(2), c.I(3), c.f(3));
    }
    return -1000;
}

int main(int argc, char** argv) { return emu_run_script(argc, argv, dispatch); }
