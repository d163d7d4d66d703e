// test_byte_ops.cpp — the host compilation of csrc/byte_ops.hpp against byte loops and snprintf (tests/test_primitives_cpu.py
// builds this with -fsanitize=address,undefined; tests/test_primitives_gpu.py runs the device compilation over the same
// structured cases).  Prints "byte_ops ok: <checks> checks" and exits 0, or the first mismatch and exits 1.
#include "byte_ops.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using edsx::u32;

static unsigned long long checks = 0;

static u32 ne_ref(uint32_t a, uint32_t b)
{
    u32 m = 0;
    for (int k = 0; k < 4; k++)
        if (((a >> (8 * k)) & 0xffu) != ((b >> (8 * k)) & 0xffu)) m |= 1u << k;
    return m;
}

static void pair(uint32_t a, uint32_t b)
{
    const u32 want = ne_ref(a, b), ne = edsx::ne_bytes4(a, b), eq = edsx::eq_byte4(a, b);
    if (ne != want || eq != (want ^ 0xFu)) {
        std::printf("ne_bytes4(%08x, %08x) = %x, eq_byte4 = %x, want %x and %x\n", a, b, ne, eq, want, want ^ 0xFu);
        std::exit(1);
    }
    checks++;
}

static void digits(u32 v)
{
    char buf[16];
    const int want = std::snprintf(buf, sizeof buf, "%u", v);
    if ((int)edsx::ndigits(v) != want) {
        std::printf("ndigits(%u) = %u, want %d\n", v, edsx::ndigits(v), want);
        std::exit(1);
    }
    checks++;
}

int main()
{
    unsigned long long r = 1;
    auto next = [&] { r = edsx::mix64(r); return (uint32_t)(r >> 16); };

    // every pair of values of one byte, the three other bytes random (equal in half of the pairs, so that the byte under
    // test decides its own bit next to neighbours of both kinds)
    for (int k = 0; k < 4; k++)
        for (uint32_t x = 0; x < 256; x++)
            for (uint32_t y = 0; y < 256; y++) {
                const uint32_t keep = ~(0xffu << (8 * k)), ra = next() & keep, rb = ((x + y) & 1 ? next() & keep : ra);
                pair(ra | (x << (8 * k)), rb | (y << (8 * k)));
            }
    for (int i = 0; i < 1000000; i++) { const uint32_t a = next(), b = next(); pair(a, b); }
    // the trick adds 0x7f to every byte: the values around its carry, alone and in every byte
    const uint32_t edge[][2] = {{0x00, 0x80}, {0x7f, 0xff}, {0x80, 0x80}, {0x00, 0x00}, {0xff, 0xff}, {0x00, 0xff}, {0x7f, 0x80}, {0x01, 0x00}, {0x80, 0x00}};
    for (const auto& e : edge) {
        for (int k = 0; k < 4; k++) {
            pair(e[0] << (8 * k), e[1] << (8 * k));
            pair(e[1] << (8 * k), e[0] << (8 * k));
            pair((e[0] << (8 * k)) | (0x55555555u & ~(0xffu << (8 * k))), (e[1] << (8 * k)) | (0x55555555u & ~(0xffu << (8 * k))));
        }
        pair(e[0] * 0x01010101u, e[1] * 0x01010101u);
    }
    pair(0x12345678u, 0x12345678u);                              // all bytes equal
    pair(0x12345678u, 0x87654321u);                              // all bytes different
    pair(0x00000000u, 0x80808080u);
    pair(0x7f7f7f7fu, 0xffffffffu);
    pair(0x80808080u, 0x80808080u);

    for (unsigned long long p = 10; p <= 1000000000ull; p *= 10) { digits((u32)(p - 1)); digits((u32)p); digits((u32)(p + 1)); }
    digits(1);
    digits(2);
    digits(4294967295u);
    digits(4294967294u);
    digits(2147483648u);
    for (int i = 0; i < 100000; i++) { const u32 v = next() >> (next() & 31); digits(v ? v : 1); }

    std::printf("byte_ops ok: %llu checks\n", checks);
    return 0;
}
