// vcf_walk.hpp — the per-thread code of the VCF -> EDS overlay (vcf_device.hip, vcf_contig.hip): the byte window, the
// field walk of the tokeniser, the map from file offsets to reference positions, and the body of every kernel that is
// one thread per record or per group with no wave operation in it.  Plain functions over plain arrays: hipcc compiles
// them for the device, where each __global__ kernel is a one-line wrapper around its body, and g++ compiles them for
// tests/cpp/test_vcf_walk.cpp, which runs the whole transform on the CPU, one "thread" after another, under the address
// and undefined-behaviour sanitizers, on buffers of exactly the sizes below ("the host twin").
//
// A body takes (..., grid): grid.first() is the global index of the thread, grid.stride() the number of threads of the
// grid, grid.lead() holds for thread 0.  On the device they are the expressions over blockIdx / blockDim / threadIdx /
// gridDim that the kernels had inline (WalkGrid in vcf_device.hip), evaluated where the kernels evaluated them, so the
// wrappers compile to nearly what the kernels were (26 of the 31 kernels of vcf_device.hip have the registers and code
// size of before, five differ by a few registers or bytes: figures and timings in DESIGN 5); on the host they are two
// numbers (HostGrid).
// The sizes of the buffers these functions read and write are part of the definition (vcf_size::*, at the end):
// VcfPipeline allocates through them and so does the host program.
#pragma once

#include <stdint.h>

#include "byte_ops.hpp"

#if defined(__HIPCC__)
#define VCF_HD __host__ __device__ inline
#else
#define VCF_HD inline
#endif
#define VCF_HDF VCF_HD __attribute__((always_inline))      // what was __device__ __forceinline__

namespace edsx {

typedef unsigned long long u64;
typedef unsigned int u32;

// ne_bytes4 / eq_byte4 (per-byte compare masks of a dword) and ndigits: byte_ops.hpp

// the few atomics of these kernels: the HIP atomic on the device, a plain operation on the host (one thread there)
VCF_HDF void walk_atomic_min(u64* p, u64 v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin((unsigned long long*)p, (unsigned long long)v);
#else
    if (v < *p) *p = v;
#endif
}
VCF_HDF void walk_atomic_max(u64* p, u64 v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax((unsigned long long*)p, (unsigned long long)v);
#else
    if (v > *p) *p = v;
#endif
}

// 16 aligned bytes of text
#if defined(__HIPCC__)
typedef uint4 Chunk16;
#else
struct alignas(16) Chunk16 { uint32_t x, y, z, w; };
#endif

struct HostGrid { u64 f, s; u64 first() const { return f; } u64 stride() const { return s; } bool lead() const { return f == 0; } };

struct VtCtl { u64 n, bad, nrec, max_samples, t_alt, t_altc, t_pair, t_all, oob; };

// The control block of a VcfPipeline (ctl_, vcf_size::ctl() bytes in HBM): what the host and the kernels of one run()
// tell each other.  Every word has one name and one meaning; the host addresses a field as &ctl->field and reads the
// block back as a whole.  Who writes what: DESIGN 5.
struct VcfCtl {
    u64 n;                       // element count of the scan in flight (blocks, records, groups)
    u64 refc_n, max_end, ngrp, nraw, rawchars, bitwords, eds, seds;   // totals of the scans, in the order run() makes them
    u64 cpos;                    // k_cpos: place of the tail's first base in refc
    u64 rec_end, rest_bytes;     // k_fa_record_end (atomicMin from fasta_n), k_fa_seq_bytes: bytes of the later lines
    u64 oob;                     // window mode: VcfDev::oob points here
    VtCtl vt;                    // the tokeniser's own (tokenize_device, tokenize_lines, index_device)
};

// The bytes of the VCF text through 8-byte aligned loads.  A thread walks its line from left to right, so seven of
// eight byte reads come out of the register window instead of a one-byte load each (k_vt_count 0.80 -> 0.65 ms,
// k_vt_fill 0.96 -> 0.75 ms per 10^6 records, round 2).  Bounds: the text buffer starts 256-byte aligned (hipMalloc) and
// is allocated with at least 16 bytes of slack behind its n bytes (vcf_size::text), so the aligned word that
// holds a byte i < n - the only bytes ever asked for - ends at most 7 bytes behind n, inside the allocation.
struct ByteWindow {
    const u64* words; u64 nbytes; u64 at = ~0ull; u64 v = 0; u64 oob = 0;
    VCF_HDF ByteWindow(const uint8_t* raw, u64 n) : words(reinterpret_cast<const u64*>(raw)), nbytes(n) {}
    VCF_HDF uint8_t operator[](u64 i)
    {
        if (i >= nbytes) { oob = i | (1ull << 63); return (uint8_t)'\n'; }   // never asked for by a correct walk: reported, not read
        const u64 wi = i >> 3;
        if (wi != at) { at = wi; v = words[wi]; }
        return (uint8_t)(v >> ((i & 7u) * 8u));
    }
};

// Record-line starts without a flag and an index word per input BYTE (that scratch, 16 B per byte, sent VCFs of more than
// a few GB to the host tokeniser): a wave owns 1024 bytes of the text (16 per lane); pass 1 counts the line starts of
// every such block, a scan over the BLOCK counts (8 B per KB of text) numbers them, pass 2 finds them again and writes
// their positions.  A byte starts a record line iff it follows a newline (or is the first byte) and is neither a
// newline nor '#'.
constexpr u64 VT_BLOCK = 1024;
VCF_HDF u32 chunk_eq16b(const Chunk16& a, uint32_t cccc)      // bit i: byte i equals c
{
    return eq_byte4(a.x, cccc) | (eq_byte4(a.y, cccc) << 4) | (eq_byte4(a.z, cccc) << 8) | (eq_byte4(a.w, cccc) << 12);
}
VCF_HDF u32 vt_line_start_mask(const uint8_t* __restrict__ raw, u64 n, u64 i0, bool& saw_cr)
{
    if (i0 >= n) return 0;
    const Chunk16 v = *reinterpret_cast<const Chunk16*>(raw + i0);        // (the text buffer is 256-byte aligned, 16 bytes of slack)
    const u32 nl = chunk_eq16b(v, 0x0a0a0a0au), hash = chunk_eq16b(v, 0x23232323u);
    if (chunk_eq16b(v, 0x0d0d0d0du) & (n - i0 >= 16 ? 0xffffu : (1u << (n - i0)) - 1u)) saw_cr = true;
    const u32 prev_nl = ((nl << 1) | (i0 == 0 || raw[i0 - 1] == '\n' ? 1u : 0u)) & 0xffffu;
    u32 m = prev_nl & ~nl & ~hash;
    if (n - i0 < 16) m &= (1u << (n - i0)) - 1u;
    return m;
}

// ---- the reference stream and the records, as every kernel sees them -----------------------------------------
struct VcfDev {
    // reference
    const uint8_t* fasta; u64 fasta_n; u64 seq_start, seq_size, lw;   // fasta[i]: file byte cbase + i
    const uint8_t* refc; u64 refc_n; const u64* blkpre;
    u64 cbase, wend;               // file offsets: refc / blkpre begin at cbase (seq_start, or the window's first byte), the
                                   // device holds the file up to wend (fasta_n, or the window's end)
    u64* oob;                      // window mode: a read outside the window is reported here (file offset | flags), not clamped
    // records
    u64 nrec; const u64* start; const u64* reflen; const u64* alt0; const u64* altstr_off; const uint8_t* altchars;
    const u64* pair0;          // per record: first (record,sample) pair; pair0[nrec] = #pairs
    const u64* pair_a0;        // per pair: first allele; pair_a0[#pairs] = #alleles
    const int* alleles;
    // groups
    u64 ngrp; const u64* grp_r0;   // first record of group g, grp_r0[ngrp] = nrec
    const u64* incl_end;           // inclusive max-scan of record ends
    u64 cur0;                      // reference position the walk starts at (0 unless this is a later position range)
};

VCF_HDF u64 fa_cpos(const VcfDev& d, u64 file_off)
{   // position in refc of file offset file_off (>= cbase); offsets past EOF map to refc_n
    if (file_off >= d.fasta_n) return d.refc_n;
    if (file_off < d.cbase || file_off >= d.wend) {      // (whole file: never)
        if (d.oob && file_off != d.wend) *d.oob = file_off | (1ull << 63);
        return d.refc_n;
    }
    const u64 rel = file_off - d.cbase;
    u64 c = d.blkpre[rel >> 8];
    // sequence bytes in [block start, file_off): eight bytes per (unaligned) load, line breaks counted with an exact
    // SWAR zero-byte test; the buffer has 16 bytes of slack behind wend, bytes at or past file_off are masked out
    u64 f = rel & ~255ull;
    u64 breaks = 0;
    while (f < rel) {
        u64 w;
        __builtin_memcpy(&w, d.fasta + f, 8);
        const u64 left = rel - f;
        const u64 keep = left >= 8 ? ~0ull : ((1ull << (8 * left)) - 1ull);
        const u64 a = w ^ 0x0a0a0a0a0a0a0a0aull, b = w ^ 0x0d0d0d0d0d0d0d0dull;
        const u64 nza = (((a & 0x7f7f7f7f7f7f7f7full) + 0x7f7f7f7f7f7f7f7full) | a) & 0x8080808080808080ull;   // high bit = byte != '\n'
        const u64 nzb = (((b & 0x7f7f7f7f7f7f7f7full) + 0x7f7f7f7f7f7f7f7full) | b) & 0x8080808080808080ull;
        breaks += __builtin_popcountll(~(nza & nzb) & 0x8080808080808080ull & keep);
        f += 8;
    }
    return c + (rel - (rel & ~255ull)) - breaks;
}

// seq_size of parse_fasta_metadata (:69-84) on the device: the record ends at the first later line that starts with
// '>' (or at EOF); its size is the number of bytes that are not '\n' from the first sequence line on ('\r' counts,
// as in the reference's getline loop).
template <class G> VCF_HDF void fa_record_end_body(const uint8_t* f, u64 n, u64 from, u64* rec_end, G grid)
{
    u64 best = ~0ull;
    for (u64 i = from + grid.first(); i < n; i += grid.stride())
        if (f[i] == '>' && f[i - 1] == '\n') { best = i; break; }
    if (best != ~0ull) walk_atomic_min(rec_end, best);
}

// ---- grouping -------------------------------------------------------------------------------------
template <class G> VCF_HDF void rec_ends_body(const u64* start, const u64* reflen, u64 n,
                           u64* ends, G grid)
{
    for (u64 j = grid.first(); j < n; j += grid.stride())
        ends[j] = start[j] + reflen[j];
}
// a record opens a group iff its start is not below the largest end seen before it (:510)
template <class G> VCF_HDF void mark_groups_body(const u64* start, const u64* incl_end, u64 n,
                              u64* flag, G grid)
{
    for (u64 j = grid.first(); j < n; j += grid.stride())
        flag[j] = (j == 0) || !(start[j] < incl_end[j - 1]);
}
template <class G> VCF_HDF void group_firsts_body(const u64* flag, const u64* gidx, u64 n,
                               u64* grp_r0, const u64* ngrp, G grid)
{
    for (u64 j = grid.first(); j < n; j += grid.stride())
        if (flag[j]) grp_r0[gidx[j]] = j;
    if (grid.lead()) grp_r0[*ngrp] = n;
}

// ---- per group: thread per group ---------------------------------------------------------------------
struct GrpArrays {
    u64* gs; u64* spanlen; u64* cs;          // span start (sequence position), clamped length, refc position
    u64* nraw; u64* rawchars;                // raw haplotypes (1 + sum of alts) and their total length
    u64* ndist;                              // distinct haplotypes
    u64* bitwords;                           // ndist * sample words
    u64* eds_len; u64* seds_len;             // group symbol + preceding common region
    u64* commonlen; u64* cur_after;          // common region before the group, reference position after it
};

// apply_variant_to_span :356-390: span.substr(0, off) + alt + (off + |ref| < |span| ? span.substr(off + |ref|) : "").
// substr(0, n) never throws: an offset beyond the span (records at or below POS 0 with a long REF, groups
// past the end of the reference) just takes the whole span; off + reflen wraps like the reference's size_t.
VCF_HDF u64 hap_len(u64 off, u64 altlen, u64 reflen, u64 spanlen)
{
    u64 len = (off < spanlen ? off : spanlen) + altlen;
    if (off + reflen < spanlen) len += spanlen - (off + reflen);
    return len;
}

template <class G> VCF_HDF void grp_count_body(VcfDev d, GrpArrays a, G grid)
{
    for (u64 g = grid.first(); g < d.ngrp; g += grid.stride()) {
        const u64 r0 = d.grp_r0[g], r1 = d.grp_r0[g + 1];
        const u64 gs = d.start[r0], ge = d.incl_end[r1 - 1];
        u64 spanlen = 0, cs = d.refc_n;
        if (gs < d.seq_size) {                                 // read_fasta_region :102-109
            u64 length = ge - gs;
            if (gs + length > d.seq_size) length = d.seq_size - gs;
            cs = fa_cpos(d, d.seq_start + gs + gs / d.lw);
            spanlen = length < d.refc_n - cs ? length : d.refc_n - cs;
            if (d.oob && spanlen < length) *d.oob = (d.seq_start + gs + gs / d.lw) | (1ull << 62);   // the window is too short
        }
        a.gs[g] = gs; a.spanlen[g] = spanlen; a.cs[g] = cs;
        u64 nraw = 1, chars = spanlen;
        for (u64 v = r0; v < r1; v++) {
            const u64 off = d.start[v] - gs;
            const u64 nalt = d.alt0[v + 1] - d.alt0[v];
            for (u64 x = d.alt0[v]; x < d.alt0[v + 1]; x++)
                chars += hap_len(off, d.altstr_off[x + 1] - d.altstr_off[x], d.reflen[v], spanlen);
            nraw += nalt;
        }
        a.nraw[g] = nraw; a.rawchars[g] = chars;
    }
}

struct HapArrays {
    const u64* raw0; const u64* rawc0;       // exclusive scans of nraw / rawchars
    u64* rawlen; u64* rawoff; u32* canon;    // per raw haplotype: length, offset in hapchars, canonical index
    uint8_t* hapchars;
    const u64* bit0;                         // exclusive scan of bitwords
    u64* carried;                            // bit matrix [canonical hap][sample word]
    u32 sw;                                  // sample words = ceil(max_samples / 64)
};

// materialise the raw haplotypes (span first, then every ALT applied alone: :416-435) and
// deduplicate them keeping the first occurrence
template <class G> VCF_HDF void grp_haps_body(VcfDev d, GrpArrays a, HapArrays h, G grid)
{
    for (u64 g = grid.first(); g < d.ngrp; g += grid.stride()) {
        const u64 r0 = d.grp_r0[g], r1 = d.grp_r0[g + 1];
        const u64 gs = a.gs[g], spanlen = a.spanlen[g], cs = a.cs[g];
        const uint8_t* span = d.refc + cs;
        u64 hi = h.raw0[g];
        u64 co = h.rawc0[g];
        // raw hap 0 = the reference span
        h.rawlen[hi] = spanlen; h.rawoff[hi] = co;
        for (u64 i = 0; i < spanlen; i++) h.hapchars[co + i] = span[i];
        co += spanlen; hi++;
        const u64 nraw = a.nraw[g];
        for (u64 v = r0; v < r1 && hi < h.raw0[g] + nraw; v++) {
            const u64 off = d.start[v] - gs, rl = d.reflen[v];
            for (u64 x = d.alt0[v]; x < d.alt0[v + 1]; x++) {
                const u64 al = d.altstr_off[x + 1] - d.altstr_off[x];
                const u64 len = hap_len(off, al, rl, spanlen);
                h.rawlen[hi] = len; h.rawoff[hi] = co;
                uint8_t* dst = h.hapchars + co;
                const u64 pre = off < spanlen ? off : spanlen;
                for (u64 i = 0; i < pre; i++) *dst++ = span[i];
                for (u64 i = 0; i < al; i++) *dst++ = d.altchars[d.altstr_off[x] + i];
                if (off + rl < spanlen) for (u64 i = off + rl; i < spanlen; i++) *dst++ = span[i];
                co += len; hi++;
            }
        }
        // dedup, first occurrence wins
        const u64 h0 = h.raw0[g];
        u32 nd = 0;
        for (u64 x = 0; x < nraw; x++) {
            u32 c = 0xffffffffu;
            for (u64 y = 0; y < x; y++) {
                if (h.rawlen[h0 + y] != h.rawlen[h0 + x] || h.canon[h0 + y] & 0x80000000u) continue;
                const uint8_t* p = h.hapchars + h.rawoff[h0 + x];
                const uint8_t* q = h.hapchars + h.rawoff[h0 + y];
                bool eq = true;
                for (u64 i = 0; i < h.rawlen[h0 + x]; i++) if (p[i] != q[i]) { eq = false; break; }
                if (eq) { c = h.canon[h0 + y]; break; }
            }
            // bit 31 marks "duplicate of an earlier one" so that only first occurrences are compared against
            h.canon[h0 + x] = c == 0xffffffffu ? nd++ : (c | 0x80000000u);
        }
        a.ndist[g] = nd;
        a.bitwords[g] = (u64)nd * h.sw;
    }
}

// which samples carry which haplotype (:438-473) and the text sizes (:570-651)
template <class G> VCF_HDF void grp_samples_body(VcfDev d, GrpArrays a, HapArrays h, G grid)
{
    for (u64 g = grid.first(); g < d.ngrp; g += grid.stride()) {
        const u64 r0 = d.grp_r0[g], r1 = d.grp_r0[g + 1];
        const u64 h0 = h.raw0[g];
        const u64 nd = a.ndist[g];
        u64* bits = h.carried + h.bit0[g];
        for (u64 i = 0; i < nd * h.sw; i++) bits[i] = 0;
        const u64 nsamp = d.pair0[r0 + 1] - d.pair0[r0];       // samples of the group's first record (:407)
        for (u64 s = 0; s < nsamp; s++) {
            bool any = false;
            u64 rawbase = 1;
            for (u64 v = r0; v < r1; v++) {
                const u64 nalt = d.alt0[v + 1] - d.alt0[v];
                const u64 ns_v = d.pair0[v + 1] - d.pair0[v];
                if (s < ns_v) {
                    const u64 pr = d.pair0[v] + s;
                    for (u64 t = d.pair_a0[pr]; t < d.pair_a0[pr + 1]; t++) {
                        const int al = d.alleles[t];
                        u32 idx = 0;                           // allele 0 or out of range -> the span
                        if (al >= 1 && (u64)al <= nalt) idx = h.canon[h0 + rawbase + (u64)(al - 1)] & 0x7fffffffu;
                        bits[(u64)idx * h.sw + (s >> 6)] |= 1ull << (s & 63);
                        any = true;
                    }
                }
                rawbase += nalt;
            }
            if (!any) bits[(s >> 6)] |= 1ull << (s & 63);      // no allele at all: reference (:466-468)
        }
        // sizes
        const u64 gs = a.gs[g], spanlen = a.spanlen[g];
        u64 eds = 2, seds = 0, nemit = 0;
        if (nsamp == 0) {                                      // no genotype columns: all haplotypes, one {0} (:603-615)
            for (u64 x = 0; x < a.nraw[g]; x++)
                if (!(h.canon[h0 + x] & 0x80000000u)) { eds += h.rawlen[h0 + x]; nemit++; }
            seds = 3;
        } else {
            for (u64 x = 0; x < a.nraw[g]; x++) {
                const u32 c = h.canon[h0 + x];
                if (c & 0x80000000u) continue;
                u64 cnt = 0, digits = 0;
                for (u64 s = 0; s < nsamp; s++)
                    if (bits[(u64)c * h.sw + (s >> 6)] >> (s & 63) & 1) { cnt++; digits += ndigits((u32)s + 1); }
                if (!cnt) continue;
                eds += h.rawlen[h0 + x]; nemit++;
                seds += 2 + digits + (cnt - 1);
            }
        }
        eds += nemit ? nemit - 1 : 0;
        a.eds_len[g] = eds; a.seds_len[g] = seds;
        a.cur_after[g] = gs + spanlen;                         // group.end_pos (:404)
    }
}

// the reference flushed before group g: [end of group g-1, gs) (:570-578); thread per group, after k_grp_samples
template <class G> VCF_HDF void grp_common_body(VcfDev d, GrpArrays a, G grid)
{
    for (u64 g = grid.first(); g < d.ngrp; g += grid.stride()) {
        const u64 cur = g ? a.cur_after[g - 1] : d.cur0;
        const u64 gs = a.gs[g];
        u64 clen = 0;
        if (gs > cur && cur < d.seq_size) {
            u64 length = gs - cur;
            if (cur + length > d.seq_size) length = d.seq_size - cur;
            const u64 c0 = fa_cpos(d, d.seq_start + cur + cur / d.lw);
            clen = length < d.refc_n - c0 ? length : d.refc_n - c0;
            if (d.oob && clen < length) *d.oob = (d.seq_start + cur + cur / d.lw) | (1ull << 62);
        }
        a.commonlen[g] = clen;
        if (clen) { a.eds_len[g] += clen + 2; a.seds_len[g] += 3; }
    }
}

struct EmitArrays { const u64* eds_off; const u64* seds_off; uint8_t* eds; uint8_t* seds; };

// the group symbols: short texts behind a chain of dependent loads, so one THREAD per group — a million independent
// chains in flight hide the latency that one lane per wave could not (3.7 ms -> see DESIGN section 5)
template <class G> VCF_HDF void grp_emit_body(VcfDev d, GrpArrays a, HapArrays h, EmitArrays e, G grid)
{
    for (u64 g = grid.first(); g < d.ngrp; g += grid.stride()) {
        uint8_t* eo = e.eds + e.eds_off[g];
        uint8_t* so = e.seds + e.seds_off[g];
        const u64 clen = a.commonlen[g];
        if (clen) { eo += clen + 2; so += 3; }
        const u64 r0 = d.grp_r0[g];
        const u64 h0 = h.raw0[g];
        const u64 nsamp = d.pair0[r0 + 1] - d.pair0[r0];
        const u64* bits = h.carried + h.bit0[g];
        *eo++ = '{';
        bool first_hap = true;
        for (u64 x = 0; x < a.nraw[g]; x++) {
            const u32 c = h.canon[h0 + x];
            if (c & 0x80000000u) continue;
            // carriers of this haplotype: one load per 64 samples (a per-sample load could not be kept in a register
            // across the byte stores below, which may alias it as far as the compiler knows)
            const u64* bw = bits + (u64)c * h.sw;
            const u32 nw = (u32)((nsamp + 63) >> 6);
            u64 cnt = 0;
            if (nsamp) {
                for (u32 w = 0; w < nw; w++) {
                    const u64 rem = nsamp - 64ull * w;
                    cnt += __builtin_popcountll(bw[w] & (rem >= 64 ? ~0ull : ((1ull << rem) - 1ull)));
                }
                if (!cnt) continue;
            }
            if (!first_hap) *eo++ = ',';
            first_hap = false;
            const uint8_t* src = h.hapchars + h.rawoff[h0 + x];
            for (u64 i = 0; i < h.rawlen[h0 + x]; i++) *eo++ = src[i];
            if (nsamp) {
                *so++ = '{';
                for (u32 w = 0; w < nw; w++) {
                    const u64 rem = nsamp - 64ull * w;
                    u64 v = bw[w] & (rem >= 64 ? ~0ull : ((1ull << rem) - 1ull));
                    while (v) {
                        const u32 id = w * 64u + (u32)__builtin_ctzll(v) + 1u, nd = ndigits(id);
                        v &= v - 1;
                        u32 xx = id;
                        for (int dd = (int)nd - 1; dd >= 0; dd--) { so[dd] = (uint8_t)('0' + xx % 10); xx /= 10; }
                        so += nd;
                        *so++ = ',';
                    }
                }
                so[-1] = '}';
            }
        }
        *eo++ = '}';
        if (!nsamp) { so[0] = '{'; so[1] = '0'; so[2] = '}'; }
    }
}

template <class G> VCF_HDF void cpos_body(VcfDev d, u64 file_off, u64* out, G) { *out = fa_cpos(d, file_off); }

// tail flush (:658-665)
template <class G> VCF_HDF void tail_body(VcfDev d, u64 cur, u64 clen, uint8_t* eo, uint8_t* so, G grid)
{
    const u64 c0 = fa_cpos(d, d.seq_start + cur + cur / d.lw);
    if (grid.lead()) { eo[0] = '{'; eo[clen + 1] = '}'; so[0] = '{'; so[1] = '0'; so[2] = '}'; }
    for (u64 i = grid.first(); i < clen; i += grid.stride()) eo[1 + i] = d.refc[c0 + i];
}

// ---- device tokeniser (parse_vcf_line :232-326, parse_alt_field :142-176, parse_genotype :190-216) -------
// The VCF text goes to HBM as it is; record lines are found with a flag scan, a thread per record line walks its
// fields twice (count, then fill in sorted order) and writes the record SoA above — no host records, no uploads
// of eight arrays.  The kernels accept the *plain* spelling only: tab-separated lines without empty fields and
// with at least five of them, POS all digits (<= 19), no symbolic ALT other than <DEL>/<INS>, genotype alleles
// that are "." or all digits (<= 9), no '\r'.  Anything else — the whitespace-separated fallback of :262-279,
// malformed lines, unsupported structural variants (their warnings are in file order), signs or junk that
// std::stoull/stoi would swallow, POS 0 — raises `bad`, and the host tokeniser takes the whole file.

struct VtSink {                      // fill pass: where record j's pieces go
    u64* altoff; u64 altc_base; uint8_t* altchars; u64* pa0; u64 all_base; int* alleles;
};
struct VtCounts { u64 pos; u64 reflen, nalt, altc, ngt, nall; };

template <bool FILL>
VCF_HD bool vt_parse(ByteWindow& raw, u64 lo, u64 hi, VtCounts& c, const VtSink& k)
{
    c = VtCounts{0, 0, 0, 0, 0, 0};
    u64 fs = lo, ref_lo = 0;
    int f = 0;
    for (u64 i = lo; i <= hi; i++) {
        if (i < hi && raw[i] != '\t') continue;
        const u64 fe = i;
        if (fe == fs) return false;                                      // empty token: the reference drops it (:262-268)
        if (f == 1) {
            if (fe - fs > 19) return false;
            u64 v = 0;
            for (u64 t = fs; t < fe; t++) { const uint8_t ch = raw[t]; if (ch < '0' || ch > '9') return false; v = v * 10 + (ch - '0'); }
            c.pos = v;
        } else if (f == 3) { ref_lo = fs; c.reflen = fe - fs; }
        else if (f == 4) {
            u64 t = fs;
            while (t < fe) {                                             // std::getline(ss, a, ',')
                u64 e = t;
                while (e < fe && raw[e] != ',') e++;
                const u64 len = e - t;
                u64 src = t;                                             // index of the allele's first byte in the text
                u64 alen = len;
                if (len && raw[t] == '<' && raw[e - 1] == '>') {
                    if (len == 5 && raw[t + 1] == 'D' && raw[t + 2] == 'E' && raw[t + 3] == 'L') alen = 0;
                    else if (len == 5 && raw[t + 1] == 'I' && raw[t + 2] == 'N' && raw[t + 3] == 'S') { src = ref_lo; alen = c.reflen; }
                    else return false;                                   // unsupported SV: warning + skip on the host
                }
                if (FILL) {
                    k.altoff[c.nalt] = k.altc_base + c.altc;
                    for (u64 x = 0; x < alen; x++) k.altchars[k.altc_base + c.altc + x] = raw[src + x];
                }
                c.nalt++; c.altc += alen;
                t = e + 1;
            }
        } else if (f >= 9) {
            u64 ge = fs;
            bool slash = false;
            while (ge < fe && raw[ge] != ':') { slash |= raw[ge] == '/'; ge++; }
            const uint8_t delim = slash ? '/' : '|';
            if (FILL) k.pa0[c.ngt] = k.all_base + c.nall;
            u64 t = fs;
            while (t < ge) {
                u64 e = t;
                while (e < ge && raw[e] != delim) e++;
                const u64 len = e - t;
                if (len && !(len == 1 && raw[t] == '.')) {
                    if (len > 9) return false;
                    int v = 0;
                    for (u64 x = t; x < e; x++) { const uint8_t ch = raw[x]; if (ch < '0' || ch > '9') return false; v = v * 10 + (ch - '0'); }
                    if (FILL) k.alleles[k.all_base + c.nall] = v;
                    c.nall++;
                }
                t = e + 1;
            }
            c.ngt++;
        }
        f++;
        fs = i + 1;
    }
    return f >= 5;
}

VCF_HDF u64 vt_line_end(ByteWindow& raw, u64 lo, u64 n)
{
    u64 hi = lo;
    while (hi < n && raw[hi] != '\n') hi++;
    return hi;
}
struct VtRec { u64* pos; u64* reflen; u64* nalt; u64* altc; u64* ngt; u64* nall; u64* linelen; /* may be null */ };
template <class G> VCF_HDF void vt_count_body(const uint8_t* raw, u64 n, const u64* lstart, u64 nrec,
                           VtRec r, VtCtl* ctl, G grid)
{
    bool bad = false;
    u64 mx = 0;
    for (u64 j = grid.first(); j < nrec; j += grid.stride()) {
        ByteWindow win(raw, n);
        const u64 lo = lstart[j], hi = vt_line_end(win, lo, n);
        VtCounts c;
        if (lo >= n) { ctl->oob = lo | (1ull << 62); bad = true; continue; }
        if (!vt_parse<false>(win, lo, hi, c, VtSink{})) bad = true;
        if (win.oob) ctl->oob = win.oob;
        if (r.linelen) r.linelen[j] = hi - lo;                               // index pass of a partitioned run
        else if (c.pos == 0 || c.pos - 1 + c.reflen < c.pos - 1) bad = true; // wrapped positions: host sweep (see run)
        r.pos[j] = c.pos; r.reflen[j] = c.reflen; r.nalt[j] = c.nalt; r.altc[j] = c.altc; r.ngt[j] = c.ngt; r.nall[j] = c.nall;
        mx = c.ngt > mx ? c.ngt : mx;
    }
    if (bad) ctl->bad = 1;
    if (mx) walk_atomic_max(&ctl->max_samples, mx);
}
// strictly ascending positions: the reference's std::sort leaves such an array as it is (no two keys compare equal,
// so its result is THE sorted order) and the host sort, with its two PCIe trips, is skipped
template <class G> VCF_HDF void vt_ascending_body(const u64* pos, u64 nrec, VtCtl* ctl, G grid)
{
    bool un = false;
    for (u64 j = grid.first(); j + 1 < nrec; j += grid.stride()) un |= pos[j] >= pos[j + 1];
    if (un) ctl->t_alt = 1;                                      // scratch until the offset scans overwrite it
}
// counts in sorted order (inputs of the four offset scans)
template <class G> VCF_HDF void vt_gather_body(VtRec r, const u32* order, u64 nrec, u64* a,
                            u64* b, u64* c, u64* d, G grid)
{
    for (u64 j = grid.first(); j < nrec; j += grid.stride()) {
        const u64 i = order ? order[j] : j;
        a[j] = r.nalt[i]; b[j] = r.altc[i]; c[j] = r.ngt[i]; d[j] = r.nall[i];
    }
}
struct VtOut { u64* start; u64* reflen; u64* alt0; u64* altoff; uint8_t* altchars; u64* pair0; u64* pa0; int* alleles;
               const u64* altc0; const u64* gtc0; };
template <class G> VCF_HDF void vt_fill_body(const uint8_t* raw, u64 n, const u64* lstart,
                          const u32* order, u64 nrec, VtOut o, VtCtl* ctl, G grid)
{
    for (u64 j = grid.first(); j < nrec; j += grid.stride()) {
        const u64 lo = lstart[order ? order[j] : j];
        VtCounts c;
        VtSink k{o.altoff + o.alt0[j], o.altc0[j], o.altchars, o.pa0 + o.pair0[j], o.gtc0[j], o.alleles};
        ByteWindow win(raw, n);
        const u64 hi = vt_line_end(win, lo, n);
        if (lo < n) vt_parse<true>(win, lo, hi, c, k);
        else ctl->oob = lo | (1ull << 62);
        if (win.oob) ctl->oob = win.oob;
        o.start[j] = c.pos - 1;
        o.reflen[j] = c.reflen;
    }
    if (grid.lead()) {
        o.alt0[nrec] = ctl->t_alt; o.altoff[ctl->t_alt] = ctl->t_altc;
        o.pair0[nrec] = ctl->t_pair; o.pa0[ctl->t_pair] = ctl->t_all;
    }
}

// ---- what VcfPipeline allocates for the arrays above, in bytes --------------------------------------------------
// (the 8- and 16-byte loads of ByteWindow, vt_line_start_mask and fa_cpos rest on the slack of the two texts; the
// "+ 1" and "+ 2" entries hold the closing offsets of the CSR arrays.)
namespace vcf_size {
inline u64 text(u64 n) { return n + 16; }                          // vt_raw_: the VCF text
inline u64 line_blocks(u64 n) { return (n + VT_BLOCK - 1) / VT_BLOCK; }
inline u64 line_counts(u64 nblk) { return 8 * (nblk + 2); }         // vt_idx_: line starts per block of the text
inline u64 line_starts(u64 nr) { return 8 * (nr + 1); }             // vt_lstart_
inline u64 per_record(u64 nr) { return 8 * (nr + 2); }              // every u64-per-record array (counts, scans, SoA, grouping)
inline u64 order(u64 nr) { return 4 * (nr + 1); }                   // vt_order_
inline u64 altoff(u64 t_alt) { return 8 * (t_alt + 2); }
inline u64 altchars(u64 t_altc) { return t_altc + 16; }
inline u64 pa0(u64 t_pair) { return 8 * (t_pair + 2); }
inline u64 alleles(u64 t_all) { return 4 * (t_all + 4); }
inline u64 fasta(u64 up_n) { return up_n + 16; }                    // d_fasta_: the file, or the window of a position range
inline u64 ref_blocks(u64 body) { return (body + 255) / 256; }
inline u64 blkpre(u64 nblk) { return 8 * (nblk + 2); }
inline u64 refc(u64 body) { return body + 16; }
constexpr u64 ctl() { return 8 * 32; }                             // ctl_: one VcfCtl
inline u64 per_group(u64 ngrp) { return 8 * (ngrp + 2); }           // every u64-per-group array
inline u64 per_raw(u64 nraw_total) { return 8 * (nraw_total + 2); } // rawlen_, rawoff_
inline u64 canon(u64 nraw_total) { return 4 * (nraw_total + 2); }
inline u64 hapchars(u64 rawchars_total) { return rawchars_total + 16; }
inline u64 carried(u64 bitwords_total) { return 8 * (bitwords_total + 2); }
inline u64 eds(u64 total) { return total + 16; }                    // d_eds_, d_seds_
}
static_assert(sizeof(VcfCtl) <= vcf_size::ctl(), "VcfCtl must fit the control buffer");

} // namespace edsx
