// byte_ops.hpp — plain bit operations on packed bytes and decimal digit counts, shared by the device kernels of every
// path (dev_util.hpp) and by the code that is also compiled for the host (vcf_walk.hpp).
#pragma once

#include <stdint.h>

#include "draw.hpp"                                        // EDSX_HD

namespace edsx {

typedef unsigned int u32;

// per-byte "a != b" mask of a dword pair as 4 bits
EDSX_HD u32 ne_bytes4(uint32_t a, uint32_t b)
{
    uint32_t x = a ^ b;
    // byte != 0  <=>  ((x & 0x7f7f7f7f) + 0x7f7f7f7f | x) & 0x80808080
    uint32_t t = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
    // gather bits 7,15,23,31 -> 0..3
    return ((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u);
}
EDSX_HD u32 eq_byte4(uint32_t a, uint32_t cccc) { return 0xFu ^ ne_bytes4(a, cccc); }

// decimal digits of v (v >= 1)
EDSX_HD u32 ndigits(u32 v)
{
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) +
           (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}

} // namespace edsx
