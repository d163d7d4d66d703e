// merge_scan.hpp — device scans of one byte range of an .eds / .seds text: what the symbol-range partition of the merge
// (merge_multi.hip, the C++ port of edsparser_amd/multigpu.py, MergeSharder) learns about a rank's slice.  The results
// equal multigpu.eds_scan_range / seds_scan_range, which are the spec (see merge_scan.hip).
#pragma once

#include "msa_device.hpp"

namespace edsx {

struct EdsRangeScan {
    bool ok = true;                 // no whitespace; braces alternate from the state at lo; commas inside braces only
    u64 strings = 0;                // string starts in [lo, hi): '{', ',' and the first byte of a bare run
    bool has_cut = false;           // (lo > 0 only) the first sentinel whose preceding '}' lies in [lo, hi)
    u64 sym_start = 0, sym_end = 0, strings_before = 0;   // its bytes, and the string starts in [lo, sym_start)
};

// length of a text without trailing whitespace (multigpu._text_end)
u64 text_end(const uint8_t* p, u64 n);

// One per rank thread / context.  Every call copies its window of the text to the device, never the whole buffer.
class RangeScanner {
public:
    // .eds bytes [lo, hi) (hi <= n); `end` = text_end(eds, n); l = context length.  Window on the device: one group in
    // front of lo (for lo > 0) and up to min(end, hi + 65536 + 4 l) behind it.
    EdsRangeScan eds(const uint8_t* eds, u64 n, u64 end, u64 lo, u64 hi, u32 l, hipStream_t st);
    // .seds bytes [lo, hi): ok (no whitespace) and the number of '{' (0 when not ok).  The slice and its per-block
    // prefixes stay in HBM for seds_locate.
    bool seds_count(const uint8_t* seds, u64 n, u64 lo, u64 hi, u64& braces, hipStream_t st);
    // absolute [p0[i], p1[i]) of the ordinals[i]-th '{' ... '}' of the last seds_count slice (ordinals count from lo);
    // p1 = find('}', p0) + 1 over the whole buffer, so 0 when no '}' follows
    void seds_locate(const u64* ordinals, size_t k, u64* p0, u64* p1, hipStream_t st);
    // bytes copied to the device since the last reset_h2d
    u64 eds_h2d() const { return eds_h2d_; }
    u64 seds_h2d() const { return seds_h2d_; }
    void reset_h2d() { eds_h2d_ = seds_h2d_ = 0; }

private:
    DevBuf raw_, cnt_, tmp_, ctl_, br_;                 // .eds window, 4 block counters, scan spine, control, brace list
    DevBuf sraw_, scnt_, stmp_, sctl_, sout_;           // .seds slice, its block prefixes, ...
    const uint8_t* s_host_ = nullptr;
    u64 s_n_ = 0, s_lo_ = 0, s_hi_ = 0, s_braces_ = 0;
    bool s_ok_ = false;
    u64 eds_h2d_ = 0, seds_h2d_ = 0;
};

} // namespace edsx
