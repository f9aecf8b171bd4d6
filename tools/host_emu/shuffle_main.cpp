// Self-test of the emulator's __shfl_xor and of csrc/wave.h on it (tests/test_hostemu_shuffle_cpu.py; the script format is
// stream_rt.h's).  No kernel file of the library is involved: the kernel below is written the way the library's are.
//   0 shuffle_selftest   i: nwg iters   b: in [nwg * 256] (integer-valued floats)  bad [nwg * 256] int32  sum64 [nwg * 256]
//                                          sum8 [nwg * 256]  bits [nwg * 256] uint32  sumd [nwg * 256] double
//                                          bitsd [nwg * 256] uint64
// Every lane checks every result of every iteration against what it computes serially from `in` and counts the mismatches in
// `bad`; the last iteration's results are written out for the test to check again in numpy.  Wave w of a workgroup makes
// iters + 3 w trips (cbam_mlp_kernel's waves make different numbers of wave_sum calls), the 8-lane group g makes g % 3 more
// 8-lane butterflies on its own after that (bn_apply_kernel's pairs shuffle in a loop others have left), and every trip
// interleaves the 64-lane butterflies, the 8-lane butterfly and the fixed-partner exchange with mask 1.  The float64 butterflies
// (csrc/train_io.hip's sums) are among them: a sum of integers near 2^32 that fp32 cannot hold, in which lane 9 of a wave adds
// -0.0, and an XOR of 64-bit patterns carried as doubles, in which lane 5 of a wave starts from a signalling NaN with a payload
// and lane 9 from -0.0; mask 1 also exchanges those two doubles as they are.
#include "common.h"
#include "stream_rt.h"

static inline uint32_t f2u(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static inline float u2f(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static inline uint32_t pattern(int t, int it) { return 0x9E3779B9u * (uint32_t)(t + 1) ^ (0x85EBCA6Bu * (uint32_t)(it + 1)); }
// a quiet or signalling NaN with a payload (never zero: that would be an infinity), or -0.0f / +0.0f
static inline uint32_t float_bits(int t, int it) {
    if ((t + it) % 3 == 0) return (t & 1) ? 0x80000000u : 0u;
    return 0x7F800000u | ((pattern(t, it) & 0x007FFFFFu) | 1u) | ((uint32_t)(t & 2) << 30);
}

static inline uint64_t d2u(double d) {
    uint64_t u;
    memcpy(&u, &d, 8);
    return u;
}
static inline double u2d(uint64_t u) {
    double d;
    memcpy(&d, &u, 8);
    return d;
}
// an integer of up to 39 bits, exact in float64 and not in fp32; -0.0 in lane 9 of a wave
static inline double dbl_term(float x, int t, int it) {
    if ((t & 63) == 9) return -0.0;
    return (double)x * 4294967311.0 + (double)(it & 7);
}
// 64 bits that travel as a double: a signalling NaN with a payload in lane 5 of a wave, -0.0 in lane 9, any pattern elsewhere
static inline uint64_t dbl_bits(int t, int it) {
    if ((t & 63) == 5) return 0x7FF4DEAD00000001ull | ((uint64_t)pattern(t, it) << 8 & 0x0000FFFFFFFFFF00ull);
    if ((t & 63) == 9) return 0x8000000000000000ull;
    return ((uint64_t)pattern(t, it) << 32) | pattern(t + 7, it + 3);
}

__global__ __launch_bounds__(256) void shuffle_selftest_kernel(const float* __restrict__ in, int iters, int* __restrict__ bad,
                                                               float* __restrict__ sum64, float* __restrict__ sum8,
                                                               uint32_t* __restrict__ bits, double* __restrict__ sumd,
                                                               uint64_t* __restrict__ bitsd) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, w0 = t - lane, g0 = t & ~7;
    const float* inb = in + (size_t)blockIdx.x * 256;
    int wrong = 0;
    float s64 = 0.f, s8 = 0.f;
    uint32_t bx = 0;
    double sd = 0.0;
    uint64_t bd = 0;
    const int trips = iters + 3 * wave;
    for (int it = 0; it < trips; ++it) {
        // 64-lane butterflies: a sum of small integers (exact in any order), a max, an XOR of bit patterns
        s64 = wave_sum(inb[t] + (float)(it & 7));
        const float m64 = wave_max(inb[t] - (float)((t * 7 + it) & 15));
        bx = pattern(t, it);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bx ^= __shfl_xor(bx, o, 64);
        // the fixed-partner exchange, int and float: NaN payloads and the sign of zero arrive bit for bit
        const int nb = __shfl_xor(t * 131 + it, 1, 64);
        const uint32_t fb = f2u(__shfl_xor(u2f(float_bits(t, it)), 1, 64));
        // an 8-lane butterfly
        s8 = inb[t] + (float)(it & 3);
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) s8 += __shfl_xor(s8, o, 64);
        const uint32_t far = f2u(__shfl_xor(u2f(float_bits(t, it + 1)), 32, 64));
        // the float64 butterflies, masks 32 ... 1, and the fixed-partner exchange of a double
        sd = dbl_term(inb[t], t, it);
        bd = dbl_bits(t, it);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sd += __shfl_xor(sd, o, 64);
            bd ^= d2u(__shfl_xor(u2d(bd), o, 64));
        }
        const uint64_t nd = d2u(__shfl_xor(u2d(dbl_bits(t, it + 2)), 1, 64));

        float e64 = 0.f, em = -INFINITY, e8 = 0.f;
        uint32_t ex = 0;
        double ed = 0.0;
        uint64_t exd = 0;
        for (int l = 0; l < 64; ++l) {
            ed += dbl_term(inb[w0 + l], w0 + l, it);
            exd ^= dbl_bits(w0 + l, it);
            e64 += inb[w0 + l] + (float)(it & 7);
            em = fmaxf(em, inb[w0 + l] - (float)(((w0 + l) * 7 + it) & 15));
            ex ^= pattern(w0 + l, it);
        }
        for (int l = 0; l < 8; ++l) e8 += inb[g0 + l] + (float)(it & 3);
        wrong += (s64 != e64) + (m64 != em) + (bx != ex) + (nb != (t ^ 1) * 131 + it) + (fb != float_bits(t ^ 1, it)) +
                 (s8 != e8) + (far != float_bits(t ^ 32, it + 1)) + (d2u(sd) != d2u(ed)) + (bd != exd) +
                 (nd != dbl_bits(t ^ 1, it + 2));
    }
    for (int k = 0; k < ((t >> 3) & 7) % 3; ++k) {
        float v = inb[t] * (float)(k + 2);
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        float e = 0.f;
        for (int l = 0; l < 8; ++l) e += inb[g0 + l] * (float)(k + 2);
        wrong += v != e;
    }
    const size_t at = (size_t)blockIdx.x * 256 + t;
    bad[at] = wrong;
    sum64[at] = s64;
    sum8[at] = s8;
    bits[at] = bx;
    sumd[at] = sd;
    bitsd[at] = bd;
}

static int64_t dispatch(const emu_call& c) {
    if (c.fn != 0 || c.i.size() != 2 || c.ptr.size() != 7) return -1000;   // (a script written for fewer outputs)
    hipLaunchKernelGGL(shuffle_selftest_kernel, dim3(c.I(0)), dim3(256), 0, nullptr, c.f(0), c.I(1), c.p<int>(1), c.f(2), c.f(3),
                       c.p<uint32_t>(4), c.p<double>(5), c.p<uint64_t>(6));
    return 0;
}

int main(int argc, char** argv) { return emu_run_script(argc, argv, dispatch); }
