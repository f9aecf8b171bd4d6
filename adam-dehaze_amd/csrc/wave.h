// The 64-lane butterfly reductions, said once.  common.h includes it, and so does tools/host_emu/common.h, which stands in for
// common.h in the host-emulation build (its __shfl_xor exchanges between OS threads): hipcc and the sanitizer runs compile this
// one text.  Every lane of the wave must call them, and every lane gets the result.
#pragma once

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
