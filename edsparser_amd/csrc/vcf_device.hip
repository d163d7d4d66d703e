// vcf_device.hip — VCF (+ reference FASTA) -> EDS / sEDS on gfx950: the variant-overlay walk.
//
// Host (vcf_host.hpp, plain C++): FASTA metadata, std::sort by POS, and the VCF tokeniser for files the device
// tokeniser does not accept — the text-parsing front end of src/cpp/lib/transforms/vcf_transforms.cpp
// (:51-86, :142-326, :715-718).  Plain files are tokenised on the device (k_vt_*).  This file: the kernels and
// VcfPipeline, which launches them; run() is a sequence of stages.
// Device (HIP kernels): everything from the sorted records on —
//   group_overlapping_variants :482-534   -> max-scan of the record ends + k_mark_groups
//   read_fasta_region :98-129             -> k_fa_count/k_fa_compact (newline-free reference stream)
//   merge_variant_group :396-476          -> k_grp_count / k_grp_haps / k_grp_samples
//   generate_eds_from_variants :554-668   -> k_grp_sizes / k_grp_emit
//
// Data layout in HBM
//   refc            the FASTA bytes from the first sequence line to EOF with '\n' and '\r' removed
//                   (exactly the characters read_fasta_region can return), blkpre[] = kept bytes
//                   before every 256-byte block, so any file offset maps to a position in refc.
//   records (SoA)   start (0-based), reflen, alt range -> alt strings, per (record, sample) allele
//                   lists (two-level CSR), all in sorted order.
//   groups          first record, span [gs, gs+spanlen) in refc, raw haplotypes materialised once in
//                   hapchars, canonical (deduplicated) index per raw haplotype, carried[hap][sample]
//                   bit matrix.
#include "vcf_device.hpp"
#include "vcf_text_kernels.hpp"
#include "vcf_walk.hpp"

#include <algorithm>
#include <cstring>
#include <sstream>
#include <chrono>
#include <thread>

namespace edsx {

// VcfDev, fa_cpos and the bodies of the thread-per-item kernels below: vcf_walk.hpp

// WalkGrid / WALK_THREAD, the grid argument of those bodies: vcf_text_kernels.hpp

// ---- reference stream ---------------------------------------------------------------------------
__global__ void k_fa_count(const uint8_t* __restrict__ f, u64 n, u64 seq_start, u64* __restrict__ blkcnt, u64 nblk)
{
    const u32 lane = threadIdx.x & 63;
    const u64 wave = (blockIdx.x * (u64)blockDim.x + threadIdx.x) >> 6, nw = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 b = wave; b < nblk; b += nw) {
        const u64 base = seq_start + b * 256 + lane * 4;
        u32 c = 0;
        for (int i = 0; i < 4; i++) if (base + i < n) { uint8_t ch = f[base + i]; c += (ch != '\n' && ch != '\r'); }
        for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
        if (lane == 0) blkcnt[b] = c;
    }
}
__global__ void k_fa_compact(const uint8_t* __restrict__ f, u64 n, u64 seq_start, const u64* __restrict__ blkpre,
                             u64 nblk, uint8_t* __restrict__ refc)
{
    const u32 lane = threadIdx.x & 63;
    const u64 wave = (blockIdx.x * (u64)blockDim.x + threadIdx.x) >> 6, nw = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 b = wave; b < nblk; b += nw) {
        const u64 base = seq_start + b * 256 + lane * 4;
        uint8_t ch[4];
        u32 c = 0;
        for (int i = 0; i < 4; i++) {
            ch[i] = base + i < n ? f[base + i] : (uint8_t)'\n';
            c += (ch[i] != '\n' && ch[i] != '\r');
        }
        u32 incl = c;
        for (int o = 1; o < 64; o <<= 1) { u32 a = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += a; }
        u64 o = blkpre[b] + incl - c;
        for (int i = 0; i < 4; i++) if (ch[i] != '\n' && ch[i] != '\r') refc[o++] = ch[i];
    }
}

// seq_size of parse_fasta_metadata (:69-84) on the device: the record ends at the first later line that starts with
// '>' (or at EOF); its size is the number of bytes that are not '\n' from the first sequence line on ('\r' counts,
// as in the reference's getline loop).
__global__ void k_fa_record_end(const uint8_t* __restrict__ f, u64 n, u64 from, u64* __restrict__ rec_end)
{
    fa_record_end_body(f, n, from, rec_end, WALK_THREAD);
}
__global__ void k_fa_seq_bytes(const uint8_t* __restrict__ f, u64 from, const u64* __restrict__ rec_end, u64* __restrict__ count)
{
    const u64 hi = *rec_end;
    u64 c = 0;
    for (u64 i = from + blockIdx.x * (u64)blockDim.x + threadIdx.x; i < hi; i += (u64)gridDim.x * blockDim.x) c += f[i] != '\n';
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd((unsigned long long*)count, (unsigned long long)c);
}

// The same two passes over one slice [a, b) of the FASTA body (partitioned runs: every rank scans its slice; the slices'
// results are put together on the host, vcf_multi.hip).  s[i] is file byte s0 + i, s0 = a - 1 (the byte in front of the
// slice decides whether a '>' at a starts a line).  k_fa_slice_end: the first "\n>" with its '>' in [from, b).
__global__ void k_fa_slice_end(const uint8_t* __restrict__ s, u64 s0, u64 from, u64 b, u64* __restrict__ rec_end)
{
    u64 best = ~0ull;
    for (u64 i = from + blockIdx.x * (u64)blockDim.x + threadIdx.x; i < b; i += (u64)gridDim.x * blockDim.x)
        if (s[i - s0] == '>' && s[i - 1 - s0] == '\n') { best = i; break; }
    if (best != ~0ull) atomicMin((unsigned long long*)rec_end, (unsigned long long)best);
}
// [a, min(rec_end, b)): bytes that are not '\n' (k_fa_seq_bytes) and what breaks the line grid of a regular file: the
// byte at (i - seq_start) % (lw + 1) == lw is '\n' and no other is; no '\r'.  A thread takes 16 consecutive bytes.
// out[0] count, out[1] flags (1: '\r', 2: grid byte that is not '\n'), out[2] first '\n' off the grid
__global__ void k_fa_slice_scan(const uint8_t* __restrict__ s, u64 s0, u64 a, u64 b, const u64* __restrict__ rec_end, u64 seq_start,
                                u64 lw, u64* __restrict__ out)
{
    const u64 re = *rec_end, hi = re < b ? re : b, period = lw + 1;
    u64 cnt = 0, flags = 0, off = ~0ull;
    for (u64 c0 = a + 16 * (blockIdx.x * (u64)blockDim.x + threadIdx.x); c0 < hi; c0 += 16 * (u64)gridDim.x * blockDim.x) {
        const u64 c1 = c0 + 16 < hi ? c0 + 16 : hi;
        u64 m = (c0 - seq_start) % period;
        for (u64 i = c0; i < c1; i++) {
            const uint8_t ch = s[i - s0];
            const bool grid = m == lw;
            cnt += ch != '\n';
            if (ch == '\r') flags |= 1;
            if (grid && ch != '\n') flags |= 2;
            if (!grid && ch == '\n' && i < off) off = i;
            if (++m == period) m = 0;
        }
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd((unsigned long long*)&out[0], (unsigned long long)cnt);
    if (flags) atomicOr((unsigned long long*)&out[1], (unsigned long long)flags);
    if (off != ~0ull) atomicMin((unsigned long long*)&out[2], (unsigned long long)off);
}

// ---- grouping -------------------------------------------------------------------------------------
__global__ void k_rec_ends(const u64* __restrict__ start, const u64* __restrict__ reflen, u64 n, u64* __restrict__ ends)
{
    rec_ends_body(start, reflen, n, ends, WALK_THREAD);
}
__global__ void k_mark_groups(const u64* __restrict__ start, const u64* __restrict__ incl_end, u64 n, u64* __restrict__ flag)
{
    mark_groups_body(start, incl_end, n, flag, WALK_THREAD);
}
__global__ void k_group_firsts(const u64* __restrict__ flag, const u64* __restrict__ gidx, u64 n, u64* __restrict__ grp_r0,
                               const u64* __restrict__ ngrp)
{
    group_firsts_body(flag, gidx, n, grp_r0, ngrp, WALK_THREAD);
}

// ---- per group: thread per group (bodies and the arrays' meaning: vcf_walk.hpp) ------------------------------
__global__ void k_grp_count(VcfDev d, GrpArrays a) { grp_count_body(d, a, WALK_THREAD); }
__global__ void k_grp_haps(VcfDev d, GrpArrays a, HapArrays h) { grp_haps_body(d, a, h, WALK_THREAD); }
__global__ void k_grp_samples(VcfDev d, GrpArrays a, HapArrays h) { grp_samples_body(d, a, h, WALK_THREAD); }
__global__ void k_grp_common(VcfDev d, GrpArrays a) { grp_common_body(d, a, WALK_THREAD); }

// common text in front of every group (the bandwidth part of the output).  A wave takes 64 consecutive groups: every
// lane fetches the numbers of one group (length, offsets, position in refc - one round of dependent loads for 64
// groups instead of one per group) and writes its brackets and "{0}"; then the wave copies the texts one group after the
// other, 16 bytes per lane (unaligned loads and stores), the ragged end byte by byte.
__device__ __forceinline__ u64 readlane64(u64 v, int l)
{
    const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)v, l), hi = (u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), l);
    return (u64)lo | ((u64)hi << 32);
}
__global__ void __launch_bounds__(256) k_grp_emit_common(VcfDev d, GrpArrays a, EmitArrays e)
{
    const u32 lane = threadIdx.x & 63;
    const u64 wave = (blockIdx.x * (u64)blockDim.x + threadIdx.x) >> 6, nw = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 gb = wave * 64; gb < d.ngrp; gb += nw * 64) {
        const u64 g = gb + lane;
        u64 clen = 0, eoff = 0, c0 = 0;
        if (g < d.ngrp) clen = a.commonlen[g];
        if (clen) {
            eoff = e.eds_off[g];
            uint8_t* eo = e.eds + eoff;
            uint8_t* so = e.seds + e.seds_off[g];
            const u64 cur = g ? a.cur_after[g - 1] : d.cur0;
            c0 = fa_cpos(d, d.seq_start + cur + cur / d.lw);
            eo[0] = '{'; eo[clen + 1] = '}'; so[0] = '{'; so[1] = '0'; so[2] = '}';
        }
        u64 todo = ballot64(clen != 0);
        while (todo) {
            const int l = __builtin_ctzll(todo);
            todo &= todo - 1;
            const u64 cl = readlane64(clen, l);
            uint8_t* dst = e.eds + readlane64(eoff, l) + 1;
            const uint8_t* src = d.refc + readlane64(c0, l);
            const u64 full = cl & ~15ull;
            for (u64 i = (u64)lane * 16; i < full; i += 1024) {
                const uint4 v = load16u(src + i);
                U128u w{v.x, v.y, v.z, v.w};
                __builtin_memcpy(dst + i, &w, 16);
            }
            if (lane < (u32)(cl - full)) dst[full + lane] = src[full + lane];
        }
    }
}

__global__ void __launch_bounds__(256) k_grp_emit(VcfDev d, GrpArrays a, HapArrays h, EmitArrays e) { grp_emit_body(d, a, h, e, WALK_THREAD); }
__global__ void k_cpos(VcfDev d, u64 file_off, u64* out) { cpos_body(d, file_off, out, WALK_THREAD); }
__global__ void k_tail(VcfDev d, u64 cur, u64 clen, uint8_t* eo, uint8_t* so) { tail_body(d, cur, clen, eo, so, WALK_THREAD); }

// ---- device tokeniser: vt_parse and the bodies are in vcf_walk.hpp ---------------------------------------------
__global__ void k_vt_count(const uint8_t* __restrict__ raw, u64 n, const u64* __restrict__ lstart, u64 nrec, VtRec r, VtCtl* ctl)
{
    vt_count_body(raw, n, lstart, nrec, r, ctl, WALK_THREAD);
}
__global__ void k_vt_ascending(const u64* __restrict__ pos, u64 nrec, VtCtl* ctl) { vt_ascending_body(pos, nrec, ctl, WALK_THREAD); }
__global__ void k_vt_gather(VtRec r, const u32* __restrict__ order, u64 nrec, u64* __restrict__ a, u64* __restrict__ b,
                            u64* __restrict__ c, u64* __restrict__ d)
{
    vt_gather_body(r, order, nrec, a, b, c, d, WALK_THREAD);
}
__global__ void k_vt_fill(const uint8_t* __restrict__ raw, u64 n, const u64* __restrict__ lstart, const u32* __restrict__ order,
                          u64 nrec, VtOut o, VtCtl* ctl)
{
    vt_fill_body(raw, n, lstart, order, nrec, o, ctl, WALK_THREAD);
}
#undef WALK_THREAD

// ---- host ------------------------------------------------------------------------------------------
template <class T> static void upload(DevBuf& b, const std::vector<T>& v, hipStream_t st)
{
    b.ensure(sizeof(T) * (v.size() + 1) + 16);
    if (!v.empty()) EDSX_HIP(hipMemcpyAsync(b.ptr, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, st));
}
// Tokenise on the device (kernels above).  false: the file is not plain; the caller runs the host tokeniser.  On success
// the record SoA (sorted order) is in place in HBM and the counters are set.
bool VcfPipeline::tokenize_device(const uint8_t* vcf, size_t n, bool presorted, hipStream_t st, u64& nrec, u64& max_samples,
                                  VcfCounters& stats)
{
    { const char* e = getenv("EDSX_HOST_TOKENIZER"); if (e && atoi(e)) return false; }      // A/B switch for the parity tests
    nrec = 0; max_samples = 0;
    if (n == 0 || !device_scratch_fits(6 * n)) return false;   // raw text + the record arrays (a dozen u64 per record line)
    vt_raw_.ensure(vcf_size::text(n));
    EDSX_HIP(hipMemcpyAsync(vt_raw_.ptr, vcf, n, hipMemcpyHostToDevice, st));
    vcf_h2d_ = n;
    const uint8_t* raw = vt_raw_.as<uint8_t>();
    vt_line_starts_reset(n, vt_ctl(), vt_idx_, scan_tmp_, st);
    const u64 nr = vt_line_starts(raw, n, vt_ctl(), vt_idx_, vt_lstart_, scan_tmp_, st);
    if (nr == VT_NOT_PLAIN) return false;
    return tokenize_lines(raw, n, vt_lstart_.as<u64>(), nr, presorted, st, nrec, max_samples, stats);
}

// The tokeniser proper: text that is in HBM (n bytes, 256-byte aligned, 16 bytes of slack behind them) and the starts of
// the nr record lines to take from it, in file order.  tokenize_device hands over the whole file it has just uploaded, a
// contig session (vcf_contig.hip) one contig's slice of its regrouped line starts.
bool VcfPipeline::tokenize_lines(const uint8_t* raw, u64 n, const u64* lstart, u64 nr, bool presorted, hipStream_t st, u64& nrec,
                                 u64& max_samples, VcfCounters& stats)
{
    nrec = 0; max_samples = 0;
    stats.total_variants = stats.processed_variants = nr;
    if (nr == 0) return true;
    if (nr >= 0xffffffffull) return false;
    scan_tmp_.ensure(8 * ((nr + 2) / SCAN_TILE + 4));
    VtCtl* ctl = vt_ctl();
    VtCtl h{};
    EDSX_HIP(hipMemcpyAsync(ctl, &h, sizeof(h), hipMemcpyHostToDevice, st));
    for (DevBuf* b : {&vt_pos_, &vt_reflen_, &vt_nalt_, &vt_altc_, &vt_ngt_, &vt_nall_, &vt_s1_, &vt_s2_, &vt_s3_, &vt_s4_}) b->ensure(vcf_size::per_record(nr));
    VtRec rec{vt_pos_.as<u64>(), vt_reflen_.as<u64>(), vt_nalt_.as<u64>(), vt_altc_.as<u64>(), vt_ngt_.as<u64>(), vt_nall_.as<u64>(), nullptr};
    TraceSpan count_span(st, "tokeniser count pass", 0);
    hipLaunchKernelGGL(k_vt_count, dim3(2048), dim3(256), 0, st, raw, (u64)n, lstart, nr, rec, ctl);
    count_span.end();
    hipLaunchKernelGGL(k_vt_ascending, dim3(1024), dim3(256), 0, st, vt_pos_.as<u64>(), nr, ctl);
    EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    if (h.oob) throw DeviceError("VCF tokeniser: byte index " + std::to_string(h.oob & ((1ull << 62) - 1)) + " outside the text of " +
                                 std::to_string(n) + " bytes (flags " + std::to_string(h.oob >> 62) + ")");
    if (h.bad) return false;
    // The reference's unstable std::sort (:715-718) on (pos, file index) pairs, as on the host path — unless the
    // positions already ascend strictly (the usual VCF) or the caller hands the records over in final order.
    const u32* d_order = nullptr;
    std::vector<u32> order;
    bool need_host_sort = !presorted && h.t_alt;
    if (need_host_sort) {
        // Not ascending.  If the positions are pairwise distinct there is exactly one sorted order, so a device radix
        // sort gives the reference's permutation; equal positions (checked on the sorted keys) need the host's
        // std::sort, whose unstable permutation of them is part of the output.
        vt_s2_.ensure(vcf_size::per_record(nr)); vt_order_.ensure(vcf_size::order(nr));
        {   // eight passes: positions -> tmp -> (vt_s2_, vt_order_) -> tmp ... the last pass ends in (vt_s2_, vt_order_)
            const u64 ntiles = (nr + RS_TILE - 1) / RS_TILE, nbins = 256 * ntiles;
            vt_sorttmp_.ensure(12 * (nr + 2) + 8 * (nbins + 2) + 64);
            u64* tkeys = vt_sorttmp_.as<u64>();
            u32* tvals = reinterpret_cast<u32*>(tkeys + nr + 2);
            u64* table = reinterpret_cast<u64*>(vt_sorttmp_.as<uint8_t>() + ((12 * (nr + 2) + 15) & ~(size_t)15));
            scan_tmp_.ensure(8 * (nbins / SCAN_TILE + 4));
            EDSX_HIP(hipMemcpyAsync(&ctl->n, &nbins, 8, hipMemcpyHostToDevice, st));
            const unsigned grid = (unsigned)std::min<u64>(ntiles, 1u << 16);
            for (u32 pass = 0; pass < 8; pass++) {
                const u64* kin = pass == 0 ? vt_pos_.as<u64>() : (pass & 1) ? tkeys : vt_s2_.as<u64>();
                const u32* vin = pass == 0 ? nullptr : (pass & 1) ? tvals : vt_order_.as<u32>();
                u64* kout = (pass & 1) ? vt_s2_.as<u64>() : tkeys;
                u32* vout = (pass & 1) ? vt_order_.as<u32>() : tvals;
                hipLaunchKernelGGL(k_rs_hist, dim3(grid), dim3(64), 0, st, kin, nr, 8 * pass, ntiles, table);
                exclusive_scan_u64(table, table, &ctl->n, &ctl->nrec, scan_tmp_.as<u64>(), st);
                hipLaunchKernelGGL(k_rs_scatter, dim3(grid), dim3(64), 0, st, kin, vin, nr, 8 * pass, ntiles, table, kout, vout);
            }
        }
        VtCtl z{};
        EDSX_HIP(hipMemcpyAsync(&ctl->t_alt, &z.t_alt, 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_vt_ascending, dim3(1024), dim3(256), 0, st, vt_s2_.as<u64>(), nr, ctl);   // sorted keys: strict?
        EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        if (!h.t_alt) { need_host_sort = false; d_order = vt_order_.as<u32>(); }
    }
    if (need_host_sort) {
        std::vector<u64> hpos(nr);
        EDSX_HIP(hipMemcpy(hpos.data(), vt_pos_.ptr, 8 * nr, hipMemcpyDeviceToHost));
        order.resize(nr);
        const auto ts0 = std::chrono::steady_clock::now();
        vcf_sort_order(hpos.data(), nr, order.data());
        { const char* e = getenv("EDSX_TRACE");
          if (e && atoi(e)) fprintf(stderr, "[edsx vcf]   std::sort of %llu positions %8.3f ms\n", (unsigned long long)nr,
                                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ts0).count()); }
        vt_order_.ensure(vcf_size::order(nr));
        EDSX_HIP(hipMemcpyAsync(vt_order_.ptr, order.data(), 4 * nr, hipMemcpyHostToDevice, st));
        d_order = vt_order_.as<u32>();
    }
    h.n = nr;
    EDSX_HIP(hipMemcpyAsync(&ctl->n, &h.n, 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_vt_gather, dim3(2048), dim3(256), 0, st, rec, d_order, nr, vt_s1_.as<u64>(), vt_s2_.as<u64>(),
                       vt_s3_.as<u64>(), vt_s4_.as<u64>());
    for (DevBuf* b : {&alt0_, &pair0_, &start_, &reflen_}) b->ensure(vcf_size::per_record(nr));
    exclusive_scan_u64(vt_s1_.as<u64>(), alt0_.as<u64>(), &ctl->n, &ctl->t_alt, scan_tmp_.as<u64>(), st);
    exclusive_scan_u64(vt_s2_.as<u64>(), vt_s2_.as<u64>(), &ctl->n, &ctl->t_altc, scan_tmp_.as<u64>(), st);
    exclusive_scan_u64(vt_s3_.as<u64>(), pair0_.as<u64>(), &ctl->n, &ctl->t_pair, scan_tmp_.as<u64>(), st);
    exclusive_scan_u64(vt_s4_.as<u64>(), vt_s4_.as<u64>(), &ctl->n, &ctl->t_all, scan_tmp_.as<u64>(), st);
    EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));                          // also: `order` stays alive until its upload is done
    altoff_.ensure(vcf_size::altoff(h.t_alt)); altchars_.ensure(vcf_size::altchars(h.t_altc)); pa0_.ensure(vcf_size::pa0(h.t_pair));
    alleles_.ensure(vcf_size::alleles(h.t_all));
    VtOut o{start_.as<u64>(), reflen_.as<u64>(), alt0_.as<u64>(), altoff_.as<u64>(), altchars_.as<uint8_t>(), pair0_.as<u64>(),
            pa0_.as<u64>(), alleles_.as<int>(), vt_s2_.as<u64>(), vt_s4_.as<u64>()};
    hipLaunchKernelGGL(k_vt_fill, dim3(2048), dim3(256), 0, st, raw, (u64)n, lstart, d_order, nr, o, ctl);
    EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    if (h.oob) throw DeviceError("VCF tokeniser (fill): byte index " + std::to_string(h.oob & ((1ull << 62) - 1)) + " outside the text of " +
                                 std::to_string(n) + " bytes (flags " + std::to_string(h.oob >> 62) + ")");
    nrec = nr;
    max_samples = h.max_samples;
    return true;
}

// Index pass of a partitioned run on the device: the first half of tokenize_device (line starts, count pass) with the
// line lengths kept.  false: not a plain file, the host index pass takes it (wrapped positions are fine here: the
// planner decides what to do with them).
bool VcfPipeline::index_device(const uint8_t* vcf, size_t n, hipStream_t st, std::vector<u64>& pos, std::vector<u64>& reflen,
                               std::vector<u64>& line_off, std::vector<u64>& line_len, VcfCounters& stats)
{
    { const char* e = getenv("EDSX_HOST_TOKENIZER"); if (e && atoi(e)) return false; }
    if (n == 0 || !device_scratch_fits(6 * n)) return false;
    vt_raw_.ensure(vcf_size::text(n));
    EDSX_HIP(hipMemcpyAsync(vt_raw_.ptr, vcf, n, hipMemcpyHostToDevice, st));
    const uint8_t* raw = vt_raw_.as<uint8_t>();
    VtCtl* ctl = vt_ctl();
    vt_line_starts_reset(n, ctl, vt_idx_, scan_tmp_, st);
    const u64 nr = vt_line_starts(raw, n, ctl, vt_idx_, vt_lstart_, scan_tmp_, st);
    if (nr == VT_NOT_PLAIN) return false;
    stats = VcfCounters();
    stats.total_variants = stats.processed_variants = nr;
    pos.assign(nr, 0); reflen.assign(nr, 0); line_off.assign(nr, 0); line_len.assign(nr, 0);
    if (nr == 0) return true;
    for (DevBuf* b : {&vt_pos_, &vt_reflen_, &vt_nalt_, &vt_altc_, &vt_ngt_, &vt_nall_, &vt_s1_}) b->ensure(vcf_size::per_record(nr));
    VtRec rec{vt_pos_.as<u64>(), vt_reflen_.as<u64>(), vt_nalt_.as<u64>(), vt_altc_.as<u64>(), vt_ngt_.as<u64>(), vt_nall_.as<u64>(),
              vt_s1_.as<u64>()};
    hipLaunchKernelGGL(k_vt_count, dim3(2048), dim3(256), 0, st, raw, (u64)n, vt_lstart_.as<u64>(), nr, rec, ctl);
    EDSX_HIP(hipMemcpyAsync(pos.data(), vt_pos_.ptr, 8 * nr, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipMemcpyAsync(reflen.data(), vt_reflen_.ptr, 8 * nr, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipMemcpyAsync(line_off.data(), vt_lstart_.ptr, 8 * nr, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipMemcpyAsync(line_len.data(), vt_s1_.ptr, 8 * nr, hipMemcpyDeviceToHost, st));
    VtCtl h{};
    EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    return !h.bad;
}

FaSlice VcfPipeline::fasta_slice(const uint8_t* fasta, u64 a, u64 b, u64 seq_start, u64 rest_from, u64 lw, hipStream_t st, u64& h2d)
{
    FaSlice r{~0ull, 0, 0, ~0ull};
    h2d = 0;
    if (a >= b) return r;
    if (a == 0 || a < seq_start) throw ParamError("fasta_slice: the slice must lie behind the header line");
    const u64 s0 = a - 1, n = b - s0;
    d_slice_.ensure(n + 16);
    slice_ctl_.ensure(8 * 8);
    FaSlice* ctl = slice_ctl_.as<FaSlice>();
    EDSX_HIP(hipMemcpyAsync(d_slice_.ptr, fasta + s0, n, hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemcpyAsync(ctl, &r, sizeof(r), hipMemcpyHostToDevice, st));
    h2d = n;
    const uint8_t* sl = d_slice_.as<uint8_t>();
    const u64 from = std::max(a, rest_from);
    if (from < b) hipLaunchKernelGGL(k_fa_slice_end, dim3(1024), dim3(256), 0, st, sl, s0, from, b, &ctl->rec_end);
    hipLaunchKernelGGL(k_fa_slice_scan, dim3(1024), dim3(256), 0, st, sl, s0, a, b, &ctl->rec_end, seq_start, lw, &ctl->count);
    EDSX_HIP(hipMemcpyAsync(&r, ctl, sizeof(r), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    return r;
}

// ---- the stages of run(): each takes the state of the call (VcfWalk) and leaves the stream synchronised ---------------
void VcfPipeline::read_ctl(hipStream_t st)
{
    EDSX_HIP(hipMemcpyAsync(&hctl_, ctl_.ptr, sizeof(hctl_), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
}
void VcfPipeline::set_scan_count(u64 n, hipStream_t st)
{
    hctl_.n = n;
    EDSX_HIP(hipMemcpyAsync(&ctl_.as<VcfCtl>()->n, &hctl_.n, 8, hipMemcpyHostToDevice, st));
}
void VcfPipeline::window_check(const VcfWalk& k, u64 v) const
{
    if (v) throw DeviceError("VCF reference window: read at file offset " + std::to_string(v & ((1ull << 62) - 1)) +
                             " outside the window [" + std::to_string(k.w.up0) + ", " + std::to_string(k.w.up1) + ") (flags " +
                             std::to_string(v >> 62) + ")");
}

// The reference stream on the device: the whole file, or the window of this position range (reference_window), compacted
// into refc / blkpre; without metadata from the caller, seq_size is counted here (first line + the later lines).
// d_resident: the record is in HBM already.  Resets the control block.
void VcfPipeline::reference_stream(VcfWalk& k, const uint8_t* fasta, u64 rest_from, const FastaMeta* meta, const VcfRange& range,
                                   const uint8_t* d_resident, hipStream_t st)
{
    VcfDev& d = k.d;
    const u64 fasta_n = d.fasta_n, seq_start = d.seq_start;
    k.w = reference_window(range, meta, seq_start, d.lw, fasta_n);
    const bool window = k.w.window;
    const u64 up_n = k.w.up1 - k.w.up0;
    if (!d_resident) {
        d_fasta_.ensure(vcf_size::fasta(up_n));
        if (up_n) EDSX_HIP(hipMemcpyAsync(d_fasta_.ptr, fasta + k.w.up0, up_n, hipMemcpyHostToDevice, st));
        fasta_h2d_ = up_n;
    }
    const uint8_t* const dfa = d_resident ? d_resident : d_fasta_.as<uint8_t>();
    const u64 body = window ? up_n : fasta_n > seq_start ? fasta_n - seq_start : 0;
    const u64 nblk = vcf_size::ref_blocks(body);
    ctl_.ensure(vcf_size::ctl());
    VcfCtl* ctl = ctl_.as<VcfCtl>();
    blkpre_.ensure(vcf_size::blkpre(nblk));
    scan_tmp_.ensure(8 * ((std::max<u64>(nblk, d.nrec) + 2) / SCAN_TILE + 4));
    refc_.ensure(vcf_size::refc(body));
    hctl_ = VcfCtl{};
    hctl_.n = nblk;
    hctl_.rec_end = fasta_n;                                 // (atomicMin)
    EDSX_HIP(hipMemcpyAsync(ctl, &hctl_, sizeof(hctl_), hipMemcpyHostToDevice, st));
    if (!meta && rest_from < fasta_n) {
        hipLaunchKernelGGL(k_fa_record_end, dim3(1024), dim3(256), 0, st, dfa, (u64)fasta_n, rest_from, &ctl->rec_end);
        hipLaunchKernelGGL(k_fa_seq_bytes, dim3(1024), dim3(256), 0, st, dfa, rest_from, &ctl->rec_end, &ctl->rest_bytes);
    }
    if (nblk) {
        // (window: the buffer is the window, compacted from its first byte)
        const u64 kn = window ? up_n : fasta_n, ks = window ? 0 : seq_start;
        hipLaunchKernelGGL(k_fa_count, dim3(1024), dim3(256), 0, st, dfa, kn, ks, blkpre_.as<u64>(), nblk);
        exclusive_scan_u64(blkpre_.as<u64>(), blkpre_.as<u64>(), &ctl->n, &ctl->refc_n, scan_tmp_.as<u64>(), st);
        hipLaunchKernelGGL(k_fa_compact, dim3(1024), dim3(256), 0, st, dfa, kn, ks, blkpre_.as<u64>(), nblk,
                           refc_.as<uint8_t>());
    }
    read_ctl(st);
    d.fasta = dfa + (k.w.cbase - k.w.up0);
    d.seq_size = meta ? meta->seq_size : d.lw + hctl_.rest_bytes;
    d.refc = refc_.as<uint8_t>(); d.refc_n = nblk ? hctl_.refc_n : 0; d.blkpre = blkpre_.as<u64>();
    d.cbase = k.w.cbase; d.wend = k.w.up1; d.oob = window ? &ctl->oob : nullptr;       // (zero from the upload above)
}

// records of the host tokeniser -> the SoA in HBM (s stays the caller's until the stream is synchronised)
void VcfPipeline::host_records(VcfWalk& k, const VcfSoA& s, hipStream_t st)
{
    upload(start_, s.start, st); upload(reflen_, s.reflen, st); upload(alt0_, s.alt0, st); upload(altoff_, s.altoff, st);
    upload(altchars_, s.altchars, st); upload(pair0_, s.pair0, st); upload(pa0_, s.pa0, st); upload(alleles_, s.alleles, st);
    k.max_samples = std::max(k.max_samples, s.max_samples);
}

// group_overlapping_variants: max-scan of the record ends + k_mark_groups, or (host: the SoA of a file whose positions
// wrap, see positions_wrap) the reference's sweep on the host; then the first record of every group
void VcfPipeline::grouping(VcfWalk& k, const VcfSoA* host, hipStream_t st)
{
    VcfDev& d = k.d;
    const u64 nrec = d.nrec;
    VcfCtl* ctl = ctl_.as<VcfCtl>();
    d.start = start_.as<u64>(); d.reflen = reflen_.as<u64>(); d.alt0 = alt0_.as<u64>(); d.altstr_off = altoff_.as<u64>();
    d.altchars = altchars_.as<uint8_t>(); d.pair0 = pair0_.as<u64>(); d.pair_a0 = pa0_.as<u64>(); d.alleles = alleles_.as<int>();
    for (DevBuf* b : {&ends_, &flag_, &gidx_, &grp_r0_}) b->ensure(vcf_size::per_record(nrec));
    set_scan_count(nrec, st);
    if (!(host && positions_wrap(host->start, host->reflen))) {      // (the device tokeniser refuses wrapped positions)
        hipLaunchKernelGGL(k_rec_ends, dim3(1024), dim3(256), 0, st, d.start, d.reflen, nrec, ends_.as<u64>());
        inclusive_max_scan_u64(ends_.as<u64>(), ends_.as<u64>(), &ctl->n, &ctl->max_end, scan_tmp_.as<u64>(), st);
        hipLaunchKernelGGL(k_mark_groups, dim3(1024), dim3(256), 0, st, d.start, ends_.as<u64>(), nrec, flag_.as<u64>());
    } else {
        std::vector<u64> hflag, hend;
        sweep_groups(host->start, host->reflen, hflag, hend);
        EDSX_HIP(hipMemcpyAsync(flag_.ptr, hflag.data(), 8 * nrec, hipMemcpyHostToDevice, st));
        EDSX_HIP(hipMemcpyAsync(ends_.ptr, hend.data(), 8 * nrec, hipMemcpyHostToDevice, st));
        EDSX_HIP(hipStreamSynchronize(st));                    // the vectors go out of scope
    }
    exclusive_scan_u64(flag_.as<u64>(), gidx_.as<u64>(), &ctl->n, &ctl->ngrp, scan_tmp_.as<u64>(), st);
    hipLaunchKernelGGL(k_group_firsts, dim3(1024), dim3(256), 0, st, flag_.as<u64>(), gidx_.as<u64>(), nrec,
                       grp_r0_.as<u64>(), &ctl->ngrp);
    read_ctl(st);
    k.ngrp = hctl_.ngrp;
    d.ngrp = k.ngrp; d.grp_r0 = grp_r0_.as<u64>(); d.incl_end = ends_.as<u64>();
}

// merge_variant_group per group (thread per group) and the sizes of the texts: E, Q, and where the last group ends
void VcfPipeline::haplotypes_and_sizes(VcfWalk& k, hipStream_t st)
{
    const VcfDev& d = k.d;
    const u64 ngrp = k.ngrp;
    VcfCtl* ctl = ctl_.as<VcfCtl>();
    for (DevBuf* b : {&g_gs_, &g_spanlen_, &g_cs_, &g_nraw_, &g_rawchars_, &g_ndist_, &g_bitwords_, &g_eds_, &g_seds_,
                      &g_common_, &g_cur_, &raw0_, &rawc0_, &bit0_}) b->ensure(vcf_size::per_group(ngrp));
    GrpArrays& ga = k.ga;
    ga = GrpArrays{g_gs_.as<u64>(), g_spanlen_.as<u64>(), g_cs_.as<u64>(), g_nraw_.as<u64>(), g_rawchars_.as<u64>(),
                   g_ndist_.as<u64>(), g_bitwords_.as<u64>(), g_eds_.as<u64>(), g_seds_.as<u64>(), g_common_.as<u64>(),
                   g_cur_.as<u64>()};
    scan_tmp_.ensure(8 * ((ngrp + 2) / SCAN_TILE + 4));
    set_scan_count(ngrp, st);
    hipLaunchKernelGGL(k_grp_count, dim3(1024), dim3(256), 0, st, d, ga);
    exclusive_scan_u64(ga.nraw, raw0_.as<u64>(), &ctl->n, &ctl->nraw, scan_tmp_.as<u64>(), st);
    exclusive_scan_u64(ga.rawchars, rawc0_.as<u64>(), &ctl->n, &ctl->rawchars, scan_tmp_.as<u64>(), st);
    read_ctl(st);
    const u64 nraw_total = hctl_.nraw, rawchars_total = hctl_.rawchars;
    const u32 sw = (u32)std::max<u64>(1, (k.max_samples + 63) / 64);
    rawlen_.ensure(vcf_size::per_raw(nraw_total)); rawoff_.ensure(vcf_size::per_raw(nraw_total)); canon_.ensure(vcf_size::canon(nraw_total));
    hapchars_.ensure(vcf_size::hapchars(rawchars_total));
    HapArrays& ha = k.ha;
    ha = HapArrays{raw0_.as<u64>(), rawc0_.as<u64>(), rawlen_.as<u64>(), rawoff_.as<u64>(), canon_.as<u32>(),
                   hapchars_.as<uint8_t>(), bit0_.as<u64>(), nullptr, sw};
    hipLaunchKernelGGL(k_grp_haps, dim3(1024), dim3(256), 0, st, d, ga, ha);
    exclusive_scan_u64(ga.bitwords, bit0_.as<u64>(), &ctl->n, &ctl->bitwords, scan_tmp_.as<u64>(), st);
    read_ctl(st);
    carried_.ensure(vcf_size::carried(hctl_.bitwords));
    ha.carried = carried_.as<u64>();
    hipLaunchKernelGGL(k_grp_samples, dim3(1024), dim3(256), 0, st, d, ga, ha);
    hipLaunchKernelGGL(k_grp_common, dim3(1024), dim3(256), 0, st, d, ga);
    exclusive_scan_u64(ga.eds_len, ga.eds_len, &ctl->n, &ctl->eds, scan_tmp_.as<u64>(), st);
    exclusive_scan_u64(ga.seds_len, ga.seds_len, &ctl->n, &ctl->seds, scan_tmp_.as<u64>(), st);
    EDSX_HIP(hipMemcpyAsync(&hctl_, ctl, sizeof(hctl_), hipMemcpyDeviceToHost, st));
    u64 last_cur = 0;
    EDSX_HIP(hipMemcpyAsync(&last_cur, g_cur_.as<u64>() + (ngrp - 1), 8, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    k.E = hctl_.eds; k.Q = hctl_.seds; k.cur = last_cur;
    if (k.w.window) window_check(k, hctl_.oob);
}

// tail (:658-665, tail_length): its place in the newline-free stream comes from the device map (one thread)
void VcfPipeline::tail(VcfWalk& k, u64 next_start, hipStream_t st)
{
    const VcfDev& d = k.d;
    const u64 length = tail_length(k.cur, d.seq_size, next_start);
    if (!length) return;
    VcfCtl* ctl = ctl_.as<VcfCtl>();
    const u64 off = d.seq_start + k.cur + k.cur / d.lw;
    hipLaunchKernelGGL(k_cpos, dim3(1), dim3(1), 0, st, d, off, &ctl->cpos);
    u64 c0 = 0;
    EDSX_HIP(hipMemcpyAsync(&c0, &ctl->cpos, 8, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    k.tail = tail_clamp(length, d.refc_n, c0);
    if (k.w.window && k.tail < length) window_check(k, off | (1ull << 62));
}

void VcfPipeline::emit(const VcfWalk& k, hipStream_t st)
{
    d_eds_.ensure(vcf_size::eds(k.Etot())); d_seds_.ensure(vcf_size::eds(k.Qtot()));
    if (k.ngrp) {
        EmitArrays ea{g_eds_.as<u64>(), g_seds_.as<u64>(), d_eds_.as<uint8_t>(), d_seds_.as<uint8_t>()};
        hipLaunchKernelGGL(k_grp_emit_common, dim3(2048), dim3(256), 0, st, k.d, k.ga, ea);
        hipLaunchKernelGGL(k_grp_emit, dim3(2048), dim3(256), 0, st, k.d, k.ga, k.ha, ea);
    }
    if (k.tail)
        hipLaunchKernelGGL(k_tail, dim3(1024), dim3(256), 0, st, k.d, k.cur, k.tail, d_eds_.as<uint8_t>() + k.E, d_seds_.as<uint8_t>() + k.Q);
}

void VcfPipeline::download(const VcfWalk& k, HostBytes& eds, HostBytes& seds, hipStream_t st)
{
    // malloc'ed, not value-initialised: the pages are first touched by the copy itself (a zero-filling
    // std::string::resize costs as much as the whole device part for a 134 MB output)
    eds.take(k.Etot());
    seds.take(k.Qtot());
    PinnedDownload::copy(eds.data, d_eds_.ptr, k.Etot(), st);
    PinnedDownload::copy(seds.data, d_seds_.ptr, k.Qtot(), st);
    u64 oob = 0;
    if (k.w.window) EDSX_HIP(hipMemcpyAsync(&oob, &ctl_.as<VcfCtl>()->oob, 8, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    window_check(k, oob);
}

bool VcfPipeline::run(const uint8_t* vcf, size_t vcf_n, const uint8_t* fasta, size_t fasta_n, HostBytes& eds,
                      HostBytes& seds, VcfCounters& stats, hipStream_t st, const VcfRange& range, const VcfResident* res)
{
    // EDSX_TRACE=1: wall-clock of the host-visible stages on stderr (every mark follows a stream synchronisation)
    static const bool trace = [] { const char* e = getenv("EDSX_TRACE"); return e && atoi(e); }();
    auto t_last = std::chrono::steady_clock::now();
    auto mark = [&](const char* what) {
        if (!trace) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[edsx vcf] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    stats = VcfCounters();
    fasta_h2d_ = 0; vcf_h2d_ = 0;
    VcfWalk k;
    // ---- FASTA metadata (:51-86); seq_size: + the later lines, counted on the device (reference_stream)
    u64 rest_from = 0;
    fasta_head(fasta, fasta_n, k.d.seq_start, k.d.lw, rest_from);
    k.d.fasta_n = fasta_n;
    const FastaMeta* meta = range.fasta;
    FastaMeta res_meta;
    const bool fasta_resident = res && res->d_fasta;
    if (fasta_resident) { res_meta.seq_size = res->seq_size; res_meta.regular = false; meta = &res_meta; }   // (the index counted it)
    mark("fasta metadata");
    // ---- VCF records (:690-712) and the unstable sort (:715-718)
    u64 dev_nrec = 0;
    const bool lines_resident = res && res->d_vcf;
    const bool on_device = lines_resident ? tokenize_lines(res->d_vcf, res->vcf_n, res->d_lstart, res->nrec, range.presorted, st,
                                                           dev_nrec, k.max_samples, stats)
                                          : tokenize_device(vcf, vcf_n, range.presorted, st, dev_nrec, k.max_samples, stats);
    tokenised_on_device_ = on_device;
    if (lines_resident && !on_device) { stats = VcfCounters(); return false; }   // the caller builds the text on the host
    mark(on_device ? "device tokenise" : "device tokenise attempt");
    std::vector<VcfPart> parts;
    std::vector<u64> part_base;                              // first global record index of every part
    std::vector<std::pair<u64, u32>> order;                  // (pos, global index in file order), sorted by pos
    if (!on_device) {
        stats = VcfCounters();
        tokenise(vcf, vcf_n, parts, part_base, stats, false);
        mark("host tokenise");
        order = host_order(parts, part_base, range.presorted);
    }
    k.d.nrec = on_device ? dev_nrec : order.size();
    k.d.cur0 = k.cur = range.cur0;

    // a reference with an empty first line has no addressable positions; the reference divides by
    // line_width (UB), refuse instead
    if (k.d.lw == 0) throw FormatError("Invalid FASTA format: empty first sequence line");

    reference_stream(k, fasta, rest_from, meta, range, fasta_resident ? res->d_fasta : nullptr, st);
    mark("fasta upload, metadata, compaction");
    if (k.d.nrec) {
        VcfSoA soa;                                          // host path only
        if (!on_device) { soa = build_soa(parts, part_base, order); host_records(k, soa, st); }
        grouping(k, on_device ? nullptr : &soa, st);
        haplotypes_and_sizes(k, st);
        mark("groups, haplotypes, sizes");
    }
    tail(k, range.next_start, st);
    emit(k, st);
    mark("tail");
    download(k, eds, seds, st);
    stats.variant_groups = k.ngrp;                           // :724-726
    mark("emit + download");
    return true;
}

} // namespace edsx
