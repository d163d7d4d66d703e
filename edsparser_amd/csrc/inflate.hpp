// inflate.hpp — the DEFLATE decoder core (RFC 1951) and the gzip / BGZF container walk (RFC 1952), one definition for
// the device kernel (bgzf_device.hip, hipcc) and the host library (g++): bit reader, stored / fixed / dynamic block
// headers, code-length decoding, canonical table construction and the literal/length/distance symbol step.
// Every read is bounded by the end of the member's compressed bytes and every write by the caller's output bound; a
// violation is an error code, never an access.  No compression library is linked anywhere.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "draw.hpp"

#include <stddef.h>
#include <stdint.h>

namespace edsx {
namespace gz {

typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned short u16;

enum InfStatus : u32 {
    INF_OK = 0,
    INF_E_INPUT = 1,       // the stream wants bytes beyond the end of its compressed range
    INF_E_STREAM = 2,      // not a DEFLATE stream (bad block type, bad code set, distance in front of the output, ...)
    INF_E_OUTPUT = 3       // the stream wants to write beyond the output bound
};

// ---- bit reader: LSB first, 64-bit window, never reads at or beyond `end` ----------------------------------
struct BitReader {
    const uint8_t* p;
    u64 pos, end;          // next byte to load, end of the compressed range
    u64 bits;
    u32 n;                 // valid bits in `bits`; the bits above them are zero
    u32 err;
    EDSX_HD void init(const uint8_t* base, u64 from, u64 to) { p = base; pos = from; end = to; bits = 0; n = 0; err = INF_OK; }
    // at least 32 valid bits afterwards (the longest step between two refills takes 28), or all that is left: one
    // 8-byte load while 8 bytes are left - the bits it puts above n are the stream's next bits, ORed in again by the
    // next load - and byte by byte at the end, where the bits above n stay zero
    EDSX_HD void refill()
    {
        if (n >= 32) return;
        if (end - pos >= 8) {
            u64 w;
            __builtin_memcpy(&w, p + pos, 8);
            bits |= w << n;
            const u32 adv = (63u - n) >> 3;
            pos += adv; n += adv * 8u;
            return;
        }
        while (n <= 56 && pos < end) { bits |= (u64)p[pos++] << n; n += 8; }
    }
    EDSX_HD u32 peek(u32 k) const { return (u32)bits & ((1u << k) - 1u); }             // k <= 16, after refill()
    EDSX_HD void drop(u32 k)
    {
        if (k > n) { if (!err) err = INF_E_INPUT; bits = 0; n = 0; }
        else { bits >>= k; n -= k; }
    }
    EDSX_HD u32 get(u32 k) { refill(); const u32 v = peek(k); drop(k); return v; }
    EDSX_HD void align() { drop(n & 7u); }
    EDSX_HD u64 byte_pos() const { return pos - (n >> 3); }                            // (after align())
    EDSX_HD void skip_bytes(u64 k)                                                     // (after align())
    {
        const u64 at = byte_pos();
        if (k > end - at) { if (!err) err = INF_E_INPUT; pos = end; } else pos = at + k;
        bits = 0; n = 0;
    }
};

// ---- canonical Huffman tables ------------------------------------------------------------------------------
// count / first / offs per code length, the symbols sorted by (length, symbol), and a direct table over the next FB
// bits of the stream: (symbol << 4) | length, 0 = longer than FB bits (or no such code): the canonical walk decides.
template <int N, int FB> struct Huff {
    u16 count[16], first[16], offs[16];
    u16 sym[N];
    u16 fast[1 << FB];
    static constexpr int fast_bits = FB;
    static constexpr int fast_size = 1 << FB;
};
typedef Huff<288, 10> LitTable;
typedef Huff<32, 8> DistTable;
typedef Huff<19, 7> ClenTable;

// serial part: 0 complete code, > 0 incomplete, < 0 over-subscribed
template <class H> EDSX_HD int huff_prepare(H& h, const uint8_t* lens, int n)
{
    for (int l = 0; l < 16; l++) h.count[l] = 0;
    for (int s = 0; s < n; s++) h.count[lens[s] & 15]++;
    int left = 1;
    for (int l = 1; l < 16; l++) {
        left <<= 1;
        left -= h.count[l];
        if (left < 0) return left;
    }
    u32 code = 0, off = 0;
    h.first[0] = 0; h.offs[0] = 0;
    for (int l = 1; l < 16; l++) {
        h.first[l] = (u16)code; h.offs[l] = (u16)off;
        code = (code + h.count[l]) << 1;
        off += h.count[l];
    }
    u16 next[16];
    for (int l = 0; l < 16; l++) next[l] = h.offs[l];
    for (int s = 0; s < n; s++) if (lens[s] & 15) h.sym[next[lens[s] & 15]++] = (u16)s;
    return left;
}
// parallel part: entries [from, ..) in steps of `stride` of the direct table are zeroed, then (behind a barrier where
// several lanes share the work) the sorted symbols [from, ..) in steps of `stride` write their entries
template <class H> EDSX_HD void huff_clear_fast(H& h, int from, int stride)
{
    for (int i = from; i < H::fast_size; i += stride) h.fast[i] = 0;
}
template <class H> EDSX_HD void huff_fill_fast(H& h, const uint8_t* lens, int from, int stride)
{
    int used = 0;
    for (int l = 1; l < 16; l++) used += h.count[l];
    for (int i = from; i < used; i += stride) {
        const u32 s = h.sym[i], l = lens[s] & 15u;
        if (l > (u32)H::fast_bits) continue;
        const u32 code = h.first[l] + ((u32)i - h.offs[l]);
        u32 r = 0;
        for (u32 b = 0; b < l; b++) r |= ((code >> b) & 1u) << (l - 1 - b);
        for (u32 k = r; k < (u32)H::fast_size; k += 1u << l) h.fast[k] = (u16)((s << 4) | l);
    }
}
// the next symbol, or -1 (no such code: INF_E_STREAM is set; out of input: INF_E_INPUT is set by the reader)
template <class H> EDSX_HD int huff_decode(BitReader& br, const H& h)
{
    br.refill();
    const u32 e = h.fast[br.peek(H::fast_bits)];
    if (e) { br.drop(e & 15u); return br.err ? -1 : (int)(e >> 4); }
    u32 v = br.peek(15), code = 0, first = 0, index = 0;
    for (u32 l = 1; l < 16; l++) {
        code |= v & 1u; v >>= 1;
        const u32 c = h.count[l];
        if (code < first + c) { br.drop(l); return br.err ? -1 : (int)h.sym[index + (code - first)]; }
        index += c; first += c;
        first <<= 1; code <<= 1;
    }
    if (!br.err) br.err = br.n < 15 ? INF_E_INPUT : INF_E_STREAM;
    return -1;
}

// ---- block headers -----------------------------------------------------------------------------------------
struct BlockHeader { u32 final_block, type; u32 stored_len; u32 nlen, ndist; };

// the three header bits, and for a stored block its LEN (the reader then stands on the first raw byte)
EDSX_HD void read_block_header(BitReader& br, BlockHeader& h)
{
    h.final_block = br.get(1);
    h.type = br.get(2);
    h.stored_len = 0; h.nlen = 0; h.ndist = 0;
    if (br.err) return;
    if (h.type == 3) { br.err = INF_E_STREAM; return; }
    if (h.type == 0) {
        br.align();
        const u32 len = br.get(16), nlen = br.get(16);
        if (br.err) return;
        if ((len ^ 0xffffu) != nlen) { br.err = INF_E_STREAM; return; }
        h.stored_len = len;
    }
}
// code lengths of the fixed codes: lens[0 .. 288) literal/length, lens[288 .. 318) distance; entries [from, ..) by stride
EDSX_HD void fixed_lengths(uint8_t* lens, int from, int stride)
{
    for (int s = from; s < 318; s += stride) lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
}
// a dynamic block's header: the code-length code, then lens[0 .. nlen) and lens[nlen .. nlen + ndist)
EDSX_HD void read_dynamic_lengths(BitReader& br, BlockHeader& h, ClenTable& ct, uint8_t* lens /* >= 320 */)
{
    const u32 nlen = br.get(5) + 257, ndist = br.get(5) + 1, ncode = br.get(4) + 4;
    if (br.err) return;
    if (nlen > 286 || ndist > 30) { br.err = INF_E_STREAM; return; }
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t cl[19];
    for (u32 i = 0; i < 19; i++) cl[i] = 0;
    for (u32 i = 0; i < ncode; i++) cl[order[i]] = (uint8_t)br.get(3);
    if (br.err) return;
    if (huff_prepare(ct, cl, 19) != 0) { br.err = INF_E_STREAM; return; }      // (complete code required)
    huff_clear_fast(ct, 0, 1);
    huff_fill_fast(ct, cl, 0, 1);
    u32 i = 0;
    while (i < nlen + ndist) {
        const int s = huff_decode(br, ct);
        if (s < 0) return;
        if (s < 16) { lens[i++] = (uint8_t)s; continue; }
        u32 rep, val = 0;
        if (s == 16) {
            if (i == 0) { br.err = INF_E_STREAM; return; }
            val = lens[i - 1]; rep = 3 + br.get(2);
        } else if (s == 17) rep = 3 + br.get(3);
        else rep = 11 + br.get(7);
        if (br.err) return;
        if (i + rep > nlen + ndist) { br.err = INF_E_STREAM; return; }
        while (rep--) lens[i++] = (uint8_t)val;
    }
    if (lens[256] == 0) { br.err = INF_E_STREAM; return; }                      // no end-of-block code
    h.nlen = nlen; h.ndist = ndist;
}
// validity of a block's two codes as prepared, by zlib's rule: an over-subscribed code is refused; an incomplete code is
// accepted only when it has exactly one symbol, of length 1, or - the distance code alone - no symbol at all (RFC 1951
// 3.2.7: a block of literals only; a length symbol met in such a block has no distance code to read and ends the stream
// in next_token).  read_dynamic_lengths has seen to the end-of-block code.
template <class H> EDSX_HD bool code_acceptable(int left, const H& h, u32 n, bool may_be_empty)
{
    if (left < 0) return false;
    if (left == 0) return true;
    const u32 used = n - h.count[0];
    return (used == 0 && may_be_empty) || (used == 1 && h.count[1] == 1);
}
EDSX_HD bool codes_acceptable(int lit_left, int dist_left, const LitTable& lit, const DistTable& dist, u32 nlen, u32 ndist, bool fixed)
{
    if (fixed) return true;
    return code_acceptable(lit_left, lit, nlen, false) && code_acceptable(dist_left, dist, ndist, true);
}

// ---- the symbol step ---------------------------------------------------------------------------------------
// literal: the byte; match: TOK_MATCH | length << 16 | distance (3..258, 1..32768); end of block: TOK_END;
// TOK_ERROR: br.err says why
constexpr u32 TOK_MATCH = 0x80000000u, TOK_END = 0x40000000u, TOK_ERROR = 0x20000000u;
EDSX_HD u32 tok_len(u32 t) { return (t >> 16) & 0x1ffu; }
EDSX_HD u32 tok_dist(u32 t) { return t & 0xffffu; }

EDSX_HD u32 next_token(BitReader& br, const LitTable& lit, const DistTable& dist)
{
    const u16 lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    const u16 dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
                           12289, 16385, 24577};
    const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    const int s = huff_decode(br, lit);
    if (s < 0) return TOK_ERROR;
    if (s < 256) return (u32)s;
    if (s == 256) return TOK_END;
    if (s > 285) { br.err = INF_E_STREAM; return TOK_ERROR; }
    const u32 len = lbase[s - 257] + br.get(lext[s - 257]);
    const int d = huff_decode(br, dist);
    if (d < 0) return TOK_ERROR;
    if (d > 29) { br.err = INF_E_STREAM; return TOK_ERROR; }
    const u32 dd = dbase[d] + br.get(dext[d]);
    if (br.err) return TOK_ERROR;
    return TOK_MATCH | (len << 16) | dd;
}

// ---- CRC-32 (the gzip trailer's), as polynomial arithmetic so that chunks combine ---------------------------
constexpr u32 CRC_POLY = 0xedb88320u;
EDSX_HD u32 crc_table_entry(u32 i)
{
    u32 c = i;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
    return c;
}
// a(x) * b(x) mod P (reflected representation: bit 31 is x^0)
EDSX_HD u32 crc_mulmod(u32 a, u32 b)
{
    u32 m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) { p ^= b; if ((a & (m - 1u)) == 0) break; }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
        if (m == 0) break;
    }
    return p;
}
// x2n[i] = x^(2^i) mod P, i < 32
EDSX_HD void crc_x2n_table(u32* x2n)
{
    u32 p = 1u << 30;
    x2n[0] = p;
    for (int i = 1; i < 32; i++) x2n[i] = p = crc_mulmod(p, p);
}
// x^(8 * nbytes) mod P
EDSX_HD u32 crc_xpow_bytes(const u32* x2n, u64 nbytes)
{
    u32 p = 1u << 31;
    for (u32 k = 3; nbytes; nbytes >>= 1, k++) if (nbytes & 1u) p = crc_mulmod(x2n[k & 31u], p);
    return p;
}

// ---- the gzip container ------------------------------------------------------------------------------------
enum GzHeaderStatus { GZH_OK = 0, GZH_TRUNCATED = 1, GZH_NOT_GZIP = 2 };
struct GzHeader {
    u64 header_len;        // bytes in front of the DEFLATE stream
    u32 flg;
    bool has_bsize;        // extra subfield 'B' 'C' of length 2
    u32 block_size;        // BSIZE + 1: the whole member, header and trailer included
};
inline GzHeaderStatus gz_parse_header(const uint8_t* p, u64 avail, GzHeader& h)
{
    h.header_len = 0; h.flg = 0; h.has_bsize = false; h.block_size = 0;
    if (avail >= 1 && p[0] != 0x1f) return GZH_NOT_GZIP;
    if (avail >= 2 && p[1] != 0x8b) return GZH_NOT_GZIP;
    if (avail < 10) return GZH_TRUNCATED;
    if (p[2] != 8 || (p[3] & 0xe0)) return GZH_NOT_GZIP;
    h.flg = p[3];
    u64 at = 10;
    if (h.flg & 4) {
        if (avail - at < 2) return GZH_TRUNCATED;
        const u64 xlen = p[at] | ((u64)p[at + 1] << 8);
        at += 2;
        if (avail - at < xlen) return GZH_TRUNCATED;
        for (u64 q = at; q + 4 <= at + xlen;) {
            const u64 slen = p[q + 2] | ((u64)p[q + 3] << 8);
            if (p[q] == 66 && p[q + 1] == 67 && slen == 2 && q + 6 <= at + xlen && !h.has_bsize) {
                h.has_bsize = true;
                h.block_size = (p[q + 4] | ((u32)p[q + 5] << 8)) + 1u;
            }
            q += 4 + slen;
        }
        at += xlen;
    }
    for (int field = 0; field < 2; field++)                      // FNAME, FCOMMENT: zero-terminated
        if (h.flg & (field == 0 ? 8 : 16)) {
            while (at < avail && p[at] != 0) at++;
            if (at >= avail) return GZH_TRUNCATED;
            at++;
        }
    if (h.flg & 2) {
        if (avail - at < 2) return GZH_TRUNCATED;
        at += 2;
    }
    h.header_len = at;
    return GZH_OK;
}

struct BgzfBlock { u64 comp_off, out_off; u32 comp_len, isize; };               // (the layout of edsx_bgzf_block)

// A member at `off` that meets every BGZF condition: CM 8, FLG 4, a BSIZE subfield, the block inside the file,
// ISIZE <= 65536.  Touches the header and the trailer only.
inline bool bgzf_member(const uint8_t* data, u64 size, u64 off, BgzfBlock& b)
{
    GzHeader h;
    if (size - off < 2 || data[off] != 0x1f || data[off + 1] != 0x8b) return false;
    if (gz_parse_header(data + off, size - off, h) != GZH_OK) return false;
    if (h.flg != 4 || !h.has_bsize) return false;
    if (h.block_size > size - off || h.block_size < h.header_len + 8) return false;
    const uint8_t* t = data + off + h.block_size - 4;
    const u32 isize = t[0] | ((u32)t[1] << 8) | ((u32)t[2] << 16) | ((u32)t[3] << 24);
    if (isize > 65536u) return false;
    b.comp_off = off; b.out_off = 0; b.comp_len = h.block_size; b.isize = isize;
    return true;
}

enum GzKind { GZ_PLAIN = 0, GZ_BGZF = 1, GZ_GZIP = 2 };

// Walk of all members.  GZ_BGZF: `visit(block)` saw every block, in order, with its out_off; text_size is their sum.
template <class Visit> inline GzKind gz_walk(const uint8_t* data, u64 size, u64& text_size, Visit visit)
{
    text_size = 0;
    if (size < 2 || data[0] != 0x1f || data[1] != 0x8b) return GZ_PLAIN;
    u64 off = 0, out = 0;
    while (off < size) {
        BgzfBlock b;
        if (!bgzf_member(data, size, off, b)) return GZ_GZIP;
        b.out_off = out;
        visit(b);
        out += b.isize;
        off += b.comp_len;
    }
    text_size = out;
    return GZ_BGZF;
}
inline GzKind gz_probe(const uint8_t* data, u64 size)
{
    u64 t;
    return gz_walk(data, size, t, [](const BgzfBlock&) {});
}

} // namespace gz
} // namespace edsx

// ---- host only: the serial inflater ------------------------------------------------------------------------
#include <string>
#include <vector>

namespace edsx {
namespace gz {

// One DEFLATE stream from data[from, to) appended to out, at most max_out bytes of it.  in_end: the byte behind the
// stream.  Distances reach back to out[base] only (a member's window is its own output).
inline u32 inflate_stream(const uint8_t* data, u64 from, u64 to, std::vector<uint8_t>& out, u64 max_out, u64& in_end)
{
    BitReader br;
    br.init(data, from, to);
    const size_t base = out.size();
    LitTable lit; DistTable dist; ClenTable ct;
    uint8_t lens[320];
    for (;;) {
        BlockHeader h;
        read_block_header(br, h);
        if (br.err) return br.err;
        if (h.type == 0) {
            const u64 at = br.byte_pos();
            br.skip_bytes(h.stored_len);
            if (br.err) return br.err;
            if (out.size() - base + h.stored_len > max_out) return INF_E_OUTPUT;
            out.insert(out.end(), data + at, data + at + h.stored_len);
        } else {
            const bool fixed = h.type == 1;
            if (fixed) { fixed_lengths(lens, 0, 1); h.nlen = 288; h.ndist = 30; }
            else {
                read_dynamic_lengths(br, h, ct, lens);
                if (br.err) return br.err;
            }
            const int ll = huff_prepare(lit, lens, (int)h.nlen), dl = huff_prepare(dist, lens + h.nlen, (int)h.ndist);
            if (!codes_acceptable(ll, dl, lit, dist, h.nlen, h.ndist, fixed)) return INF_E_STREAM;
            huff_clear_fast(lit, 0, 1); huff_fill_fast(lit, lens, 0, 1);
            huff_clear_fast(dist, 0, 1); huff_fill_fast(dist, lens + h.nlen, 0, 1);
            for (;;) {
                const u32 t = next_token(br, lit, dist);
                if (t == TOK_ERROR) return br.err ? br.err : (u32)INF_E_STREAM;
                if (t == TOK_END) break;
                const u64 have = out.size() - base;
                if (!(t & TOK_MATCH)) {
                    if (have + 1 > max_out) return INF_E_OUTPUT;
                    out.push_back((uint8_t)t);
                    continue;
                }
                const u32 len = tok_len(t), d = tok_dist(t);
                if (d > have) return INF_E_STREAM;
                if (have + len > max_out) return INF_E_OUTPUT;
                const size_t o = out.size();
                out.resize(o + len);
                for (u32 j = 0; j < len; j++) out[o + j] = out[o + j - d];
            }
        }
        if (h.final_block) break;
    }
    br.align();
    in_end = br.byte_pos();
    return INF_OK;
}

inline u32 crc32_bytes(const uint8_t* p, size_t n)
{
    static const struct Table { u32 t[256]; Table() { for (u32 i = 0; i < 256; i++) t[i] = crc_table_entry(i); } } T;
    u32 c = 0xffffffffu;
    for (size_t i = 0; i < n; i++) c = T.t[(c ^ p[i]) & 0xffu] ^ (c >> 8);
    return ~c;
}

inline std::string gz_error_text(const char* what, u64 block, u64 off, const char* reason)
{
    return std::string("Compressed ") + what + ": block " + std::to_string(block) + " at byte " + std::to_string(off) + ": " + reason;
}
// the reason for a decoder status inside a member whose end is known from BSIZE (bounded) or is the end of the file
inline const char* inflate_reason(u32 st, bool bounded)
{
    return st == INF_E_OUTPUT ? "length mismatch" : st == INF_E_INPUT && !bounded ? "truncated" : "invalid DEFLATE stream";
}

// All members of a gzip file of any shape, one after the other on this thread: what gzip.decompress returns.
// false: err holds "Compressed <what>: block <k> at byte <off>: <reason>".  blocks (optional): the members seen.
inline bool gz_inflate_host(const uint8_t* data, u64 size, std::vector<uint8_t>& out, const char* what, std::string& err, u64* blocks = nullptr)
{
    u64 off = 0, k = 0;
    while (off < size) {
        GzHeader h;
        const GzHeaderStatus hs = gz_parse_header(data + off, size - off, h);
        if (hs != GZH_OK) { err = gz_error_text(what, k, off, hs == GZH_TRUNCATED ? "truncated" : "not a gzip member"); return false; }
        u64 end = size;
        const bool bounded = h.has_bsize && h.flg == 4;
        if (bounded) {
            if (h.block_size > size - off) { err = gz_error_text(what, k, off, "block size beyond the end of the file"); return false; }
            if (h.block_size < h.header_len + 8) { err = gz_error_text(what, k, off, "invalid DEFLATE stream"); return false; }
            end = off + h.block_size;
        }
        if (end - off < h.header_len + 8) { err = gz_error_text(what, k, off, "truncated"); return false; }
        u64 max_out = ~0ull;
        if (bounded) { const uint8_t* t = data + end - 4; max_out = t[0] | ((u32)t[1] << 8) | ((u32)t[2] << 16) | ((u32)t[3] << 24); }
        const size_t o = out.size();
        u64 in_end = 0;
        const u32 st = inflate_stream(data, off + h.header_len, end - 8, out, max_out, in_end);
        if (st != INF_OK) { err = gz_error_text(what, k, off, inflate_reason(st, bounded)); return false; }
        if (bounded && in_end != end - 8) { err = gz_error_text(what, k, off, "invalid DEFLATE stream"); return false; }
        const uint8_t* t = data + in_end;
        const u32 crc = t[0] | ((u32)t[1] << 8) | ((u32)t[2] << 16) | ((u32)t[3] << 24);
        const u32 isize = t[4] | ((u32)t[5] << 8) | ((u32)t[6] << 16) | ((u32)t[7] << 24);
        if ((u32)(out.size() - o) != isize) { err = gz_error_text(what, k, off, "length mismatch"); return false; }
        if (crc32_bytes(out.data() + o, out.size() - o) != crc) { err = gz_error_text(what, k, off, "CRC mismatch"); return false; }
        off = in_end + 8;
        k++;
    }
    if (blocks) *blocks = k;
    return true;
}

} // namespace gz
} // namespace edsx
