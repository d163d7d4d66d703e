// draw.hpp — the counter-based random draws shared by the device kernels and the host library.
// Plain C++17 under g++ (the edsparser:: container) and __host__ __device__ under hipcc, so that the pattern sampler's
// host twin (EDS::generate_patterns with a seed) and k_pat_sample read one definition and cannot drift apart.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define EDSX_HD __host__ __device__ __forceinline__
#else
#define EDSX_HD inline
#endif

namespace edsx {

EDSX_HD unsigned long long mix64(unsigned long long x)
{   // splitmix64 finaliser
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
EDSX_HD unsigned long long hash3(unsigned long long seed, unsigned long long a, unsigned long long b)
{
    return mix64(seed ^ mix64(a ^ mix64(b + 0x632BE59BD9B4E019ull)));
}

// A value in [0, bound): the high 64 bits of r * bound (bound > 0).
EDSX_HD unsigned long long bounded64(unsigned long long r, unsigned long long bound)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(r, bound);
#else
    __extension__ typedef unsigned __int128 u128;
    return (unsigned long long)(((u128)r * bound) >> 64);
#endif
}

// Draw k of pattern i of the pattern sampler, in [0, bound): k = 0 picks the start position, k = 1, 2, ... the strings
// in walk order (the wrap phase continues the same counter).
EDSX_HD unsigned long long pattern_draw(unsigned long long seed, unsigned long long i, unsigned long long k,
                                        unsigned long long bound)
{
    return bounded64(hash3(seed, i, k), bound);
}

} // namespace edsx
