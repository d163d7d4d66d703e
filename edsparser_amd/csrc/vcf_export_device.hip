// vcf_export_device.hip — an EDS and its sources as VCF 4.2 text plus the reference FASTA on gfx950 (edsx_eds_vcf).
//
// Semantics: include/edsx.h, "eds2vcf".  Every symbol with two strings or more is one record; allele 0 is its reference
// string, the other strings follow in file order; the cell of path p lists the alleles whose source set holds p or 0.
// The kernels read the context's DeviceEds through its view and write nothing to it.
//
// Count -> scan -> fill, every offset 64-bit:
//   symbols i   k_vcf_sym       reference string (the first one, or the first that holds ref_path: a search over the
//                               symbol's strings in word ref_path / 64), its length, the record flag, "has an empty string";
//                               one scan of two arrays -> refpos (n + 1 entries, [n] = L) and the record rank
//               k_vcf_anchor    the records in order (recsym); the anchor base of a record with an empty string, found by
//                               bisection in refpos
//   records     k_vcf_fixedlen  bytes of the fixed part, a closed form (vcf_text.hpp), into a table laid out
//                               [record][fixed, tile 0, tile 1, ...]; counts the records that overlap the one before
//   (record, tile of 256 path ids = 4 bitset words)
//               k_vcf_count     a wave takes one word: per string ONE load of bits[j W + w] | -(bits[j W] & 1) serves its
//                               64 lanes, lane l tests bit l (path 64 w + l; id 0 and ids above P are idle lanes); cell
//                               bytes per lane, wave reduction, one entry per (record, tile)
//   one exclusive scan over the table gives every offset and the body's size; the limit is checked before the body is
//   allocated
// Fill:
//   k_vcf_fixed   a lane per aligned 16-byte chunk of the OUTPUT: a chunk that lies inside one string is one 16-byte load
//                 from the pool and one store, anything else is assembled byte by byte from the closed form.  A wave takes
//                 16 records at a time, 4 lanes each (a SNP record's fixed part has about 30 bytes); a fixed part of more
//                 than 256 bytes is then taken by the whole wave, so a 100 000-character allele spreads over 64 lanes,
//                 1 KiB per step
//   k_vcf_cells   recomputes the cell bytes, wave prefix (__shfl_up) and cross-wave prefix in LDS give every cell its
//                 offset; the tile's text is assembled in LDS, shifted so that 16-byte chunks of LDS are aligned 16-byte
//                 chunks of the output, and streamed out with aligned 16-byte stores, byte stores only at the two ragged
//                 ends.  A tile whose text does not fit the stage (paths that sit in many strings) is written by bytes
//   k_vcf_ref     the shape of k_path_copy: a workgroup per 16 KiB of the FASTA body, its symbol range by bisection in
//                 refpos, 16 bytes of output per lane with the line feeds put in on the way
#include "vcf_export_device.hpp"

#include <string>

namespace edsx {

namespace {

constexpr int VT = 256;                        // threads per block
constexpr u32 STAGE = 4096;                    // LDS bytes for the text of one (record, tile): 16 per cell
constexpr u32 REF_TILE = 16384;                // FASTA bytes per block step: 4 chunks of 16 bytes per lane
enum { CT_N1, CT_L, CT_RECS, CT_ERRREF, CT_ERRANC, CT_ANCH, CT_OVER, CT_TABN, CT_BODY, CT_COUNT };

__global__ void __launch_bounds__(VT) k_vcf_or(const u64* __restrict__ bits, u32 W, u64 m, u64* __restrict__ orbits)
{
    const u64 t0 = blockIdx.x * (u64)blockDim.x + threadIdx.x, step = (u64)gridDim.x * blockDim.x;
    for (u32 w = 0; w < W; w++) {
        u64 o = 0;
        for (u64 k = t0; k < m; k += step) o |= bits[k * W + w];
        for (int sh = 32; sh > 0; sh >>= 1) o |= __shfl_xor(o, sh, 64);
        if ((threadIdx.x & 63) == 0 && o) atomicOr((unsigned long long*)&orbits[w], (unsigned long long)o);
    }
}

// reflen, recflag: n + 1 entries ([n] = 0) for the scans; anchor[i] = 1 when the symbol is a record with an empty string
__global__ void __launch_bounds__(VT) k_vcf_sym(const u64* __restrict__ size, const u64* __restrict__ ent_off,
                                                const u64* __restrict__ str_off, const u64* __restrict__ bits, u32 W, u64 n,
                                                u64 ref_path, u64* __restrict__ refidx, u64* __restrict__ reflen,
                                                u64* __restrict__ recflag, u64* __restrict__ anchor, u64* __restrict__ ctl)
{
    const u64 w = ref_path >> 6, bit = 1ull << (ref_path & 63);
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i <= n; i += (u64)gridDim.x * blockDim.x) {
        if (i == n) { refidx[n] = 0; reflen[n] = 0; recflag[n] = 0; anchor[n] = 0; continue; }
        const u64 e0 = ent_off[i], k = size[i];
        u64 r = 0, empty = 0;
        if (ref_path) {
            r = vcf::NONE;
            for (u64 q = 0; q < k; q++) {
                const u64* b = bits + (e0 + q) * W;
                if ((b[0] & 1) || (b[w] & bit)) { r = q; break; }
            }
            if (r == vcf::NONE) { atomicMin((unsigned long long*)&ctl[CT_ERRREF], (unsigned long long)i); r = 0; }
        }
        if (k >= 2)
            for (u64 q = 0; q < k; q++) if (str_off[e0 + q + 1] == str_off[e0 + q]) { empty = 1; break; }
        refidx[i] = r;
        reflen[i] = k ? str_off[e0 + r + 1] - str_off[e0 + r] : 0;
        recflag[i] = k >= 2 ? 1 : 0;
        anchor[i] = empty;
    }
}

// t.anchor is written here (every lane its own symbol's entry)
__global__ void __launch_bounds__(VT) k_vcf_anchor(vcf::Tab t, const u64* __restrict__ rank, u64* __restrict__ anchor,
                                                   u64* __restrict__ recsym, u64* __restrict__ ctl)
{
    const u64 L = t.refpos[t.n];
    for (u64 base = blockIdx.x * (u64)blockDim.x; base < t.n; base += (u64)gridDim.x * blockDim.x) {     // block-uniform
        const u64 i = base + threadIdx.x;
        bool anch = false;
        if (i < t.n) {
            const u64 r = rank[i];
            if (rank[i + 1] != r) recsym[r] = i;
            if (anchor[i]) {
                u64 q, mode;
                if (t.refpos[i] > 0) { q = t.refpos[i] - 1; mode = vcf::ANC_FRONT; }
                else { q = t.refpos[i + 1]; mode = vcf::ANC_BACK; }
                if (q >= L) { atomicMin((unsigned long long*)&ctl[CT_ERRANC], (unsigned long long)i); anchor[i] = 0; }
                else { anchor[i] = ((u64)vcf::ref_char(t, q) << 8) | mode; anch = true; }
            }
        }
        const u64 b = ballot64(anch);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd((unsigned long long*)&ctl[CT_ANCH], (unsigned long long)__popcll(b));
    }
}

__global__ void __launch_bounds__(VT) k_vcf_fixedlen(vcf::Tab t, const u64* __restrict__ recsym, u64 R, u64 NT,
                                                     u64* __restrict__ table, u64* __restrict__ ctl)
{
    for (u64 base = blockIdx.x * (u64)blockDim.x; base < R; base += (u64)gridDim.x * blockDim.x) {       // block-uniform
        const u64 rr = base + threadIdx.x;
        bool over = false;
        if (rr < R) {
            const vcf::Rec c = vcf::rec_of(t, recsym[rr]);
            table[rr * (1 + NT)] = vcf::fixed_bytes(t, c, NT == 0);
            if (rr) {
                const vcf::Rec p = vcf::rec_of(t, recsym[rr - 1]);
                over = c.pos <= p.pos + p.reflen + p.anc - 1;            // not behind the last base of the previous REF
            }
        }
        const u64 b = ballot64(over);
        if ((threadIdx.x & 63) == 0 && b) atomicAdd((unsigned long long*)&ctl[CT_OVER], (unsigned long long)__popcll(b));
    }
}

// blockDim = 64 * min(4, W): wave v of the block owns word 4 * tile + v
__global__ void __launch_bounds__(VT) k_vcf_count(vcf::Tab t, const u64* __restrict__ recsym, u64 R, u64 NT, u64* __restrict__ table)
{
    __shared__ u32 wsum[VT / 64];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const u64 work = R * NT;
    for (u64 wi = blockIdx.x; wi < work; wi += gridDim.x) {
        const u64 rr = wi / NT, tile = wi - rr * NT;
        const vcf::Rec c = vcf::rec_of(t, recsym[rr]);
        const u64 w = 4 * tile + wave, p = 64 * w + lane;
        u32 nb = (p >= 1 && p <= t.P) ? vcf::cell_bytes(t, c, (u32)w, lane) : 0;
        for (int o = 32; o > 0; o >>= 1) nb += __shfl_down(nb, o, 64);
        if (lane == 0) wsum[wave] = nb;
        __syncthreads();
        if (threadIdx.x == 0) {
            u64 s = tile == NT - 1 ? 1 : 0;                              // the line feed
            for (u32 k = 0; k < nw; k++) s += wsum[k];
            table[rr * (1 + NT) + 1 + tile] = s;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void store_chunk(uint8_t* out, u64 c0, u64 lo, u32 nb, const vcf::B16& x)
{
    if (nb == 16) {                                                  // (lo == c0: the buffer is aligned, so is the chunk)
        *reinterpret_cast<uint4*>(out + c0) = make_uint4((u32)x.lo, (u32)(x.lo >> 32), (u32)x.hi, (u32)(x.hi >> 32));
    } else {
        for (u32 b = 0; b < nb; b++) out[lo + b] = (uint8_t)((b < 8 ? x.lo >> (8u * b) : x.hi >> (8u * (b - 8u))) & 0xffu);
    }
}

// chunks of the fixed part [d0, d1) of record c: lane `sub` of `lanes` takes every lanes-th aligned 16-byte chunk
__device__ __forceinline__ void fixed_chunks(const vcf::Tab& t, const vcf::Rec& c, u64 d0, u64 d1, u32 sub, u32 lanes,
                                             uint8_t* __restrict__ out)
{
    for (u64 c0 = (d0 & ~15ull) + 16ull * sub; c0 < d1; c0 += 16ull * lanes) {
        const u64 lo = max(c0, d0), hi = min(c0 + 16, d1);
        const u32 nb = (u32)(hi - lo);
        vcf::B16 x;
        u64 pool = 0;
        if (vcf::fixed_chunk(t, c, lo - d0, nb, x, pool)) {
            const uint4 v = load16u(t.chars + pool);
            x.lo = ((u64)v.y << 32) | v.x; x.hi = ((u64)v.w << 32) | v.z;
        }
        store_chunk(out, c0, lo, nb, x);
    }
}

// A wave takes FIX_RECS records at a time, FIX_LANES lanes each: a fixed part of up to FIX_SHORT bytes (nearly all of
// them: a SNP record has about 30) is written by its lanes alone; the longer ones of the batch are then taken one after
// the other by the whole wave, 1 KiB per step.
constexpr u32 FIX_LANES = 4, FIX_RECS = 64 / FIX_LANES, FIX_SHORT = 256;

__global__ void __launch_bounds__(VT) k_vcf_fixed(vcf::Tab t, const u64* __restrict__ recsym, u64 R, u64 NT,
                                                  const u64* __restrict__ table, uint8_t* __restrict__ out)
{
    const u32 lane = threadIdx.x & 63, sub = lane % FIX_LANES, grp = lane / FIX_LANES;
    const u64 waves = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 r0 = ((blockIdx.x * (u64)blockDim.x + threadIdx.x) >> 6) * FIX_RECS; r0 < R; r0 += waves * FIX_RECS) {    // wave-uniform
        const u64 rr = r0 + grp;
        bool is_long = false;
        if (rr < R) {
            const vcf::Rec c = vcf::rec_of(t, recsym[rr]);
            const u64 d0 = table[rr * (1 + NT)], d1 = d0 + vcf::fixed_bytes(t, c, NT == 0);
            is_long = d1 - d0 > FIX_SHORT;
            if (!is_long) fixed_chunks(t, c, d0, d1, sub, FIX_LANES, out);
        }
        u64 longs = ballot64(is_long && sub == 0);
        while (longs) {
            const u64 rl = r0 + (u32)(__ffsll((unsigned long long)longs) - 1) / FIX_LANES;
            longs &= longs - 1;
            const vcf::Rec c = vcf::rec_of(t, recsym[rl]);
            const u64 d0 = table[rl * (1 + NT)];
            fixed_chunks(t, c, d0, d0 + vcf::fixed_bytes(t, c, NT == 0), lane, 64, out);
        }
    }
}

// blockDim as k_vcf_count
__global__ void __launch_bounds__(VT) k_vcf_cells(vcf::Tab t, const u64* __restrict__ recsym, u64 R, u64 NT,
                                                  const u64* __restrict__ table, uint8_t* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[STAGE + 16];
    __shared__ u32 wsum[VT / 64];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const u64 work = R * NT;
    for (u64 wi = blockIdx.x; wi < work; wi += gridDim.x) {
        const u64 rr = wi / NT, tile = wi - rr * NT;
        const vcf::Rec c = vcf::rec_of(t, recsym[rr]);
        const u64 w = 4 * tile + wave, p = 64 * w + lane;
        const bool act = p >= 1 && p <= t.P;
        const u32 nb = act ? vcf::cell_bytes(t, c, (u32)w, lane) : 0;
        u32 incl = nb;
        for (int o = 1; o < 64; o <<= 1) { const u32 a = __shfl_up(incl, o, 64); if ((int)lane >= o) incl += a; }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        u32 woff = 0, total = 0;
        for (u32 k = 0; k < nw; k++) { if (k < wave) woff += wsum[k]; total += wsum[k]; }
        const u32 off = woff + incl - nb;
        const bool last = tile == NT - 1;
        const u64 d0 = table[rr * (1 + NT) + 1 + tile];
        const u32 bytes = total + (last ? 1u : 0u);
        uint8_t* dst = out + d0;
        if (bytes <= STAGE) {
            const u32 sh = (u32)(d0 & 15);                               // stage[sh + x] is dst[x]: chunks align in both
            if (act) vcf::cell_write(t, c, (u32)w, lane, stage + sh + off);
            if (last && threadIdx.x == 0) stage[sh + total] = '\n';
            __syncthreads();
            const u32 head = min(bytes, (16u - sh) & 15u);
            if (threadIdx.x < head) dst[threadIdx.x] = stage[sh + threadIdx.x];
            const u32 nfull = (bytes - head) >> 4;
            for (u32 q = threadIdx.x; q < nfull; q += blockDim.x)
                *reinterpret_cast<uint4*>(dst + head + 16 * q) = *reinterpret_cast<const uint4*>(stage + sh + head + 16 * q);
            const u32 t0 = head + 16 * nfull;
            if (threadIdx.x < bytes - t0) dst[t0 + threadIdx.x] = stage[sh + t0 + threadIdx.x];
        } else {                                                         // the slow path: every lane its cell, by bytes
            if (act) vcf::cell_write(t, c, (u32)w, lane, dst + off);
            if (last && threadIdx.x == 0) dst[total] = '\n';
        }
        __syncthreads();
    }
}

typedef unsigned __int128 u128;

// body: L characters in lines of lw (>= 1), each ended by a line feed; per = lw + 1
__global__ void __launch_bounds__(VT) k_vcf_ref(vcf::Tab t, u64 L, u64 lw, u64 body, uint8_t* __restrict__ out)
{
    __shared__ u64 si[2];
    const u64 per = lw + 1, last = body - 1, tiles = (body + REF_TILE - 1) / REF_TILE;
    for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const u64 o0 = tile * REF_TILE, o1 = min(body, o0 + (u64)REF_TILE);
        const u64 q0 = o0 - o0 / per, q1 = min(L, o1 - o1 / per);           // this step spells characters [q0, q1)
        __syncthreads();
        if (q0 < q1 && (threadIdx.x == 0 || threadIdx.x == 64))
            si[threadIdx.x >> 6] = vcf::ref_find(t.refpos, 0, t.n - 1, threadIdx.x ? q1 - 1 : q0);
        __syncthreads();
        const u64 iA = si[0], iB = si[1];
        auto sym = [&](u64 i, u64& end, u64& base) {                       // where symbol i's string ends; pool minus position
            end = t.refpos[i + 1];
            base = t.str_off[t.ent_off[i] + t.refidx[i]] - t.refpos[i];
        };
        for (u64 o = o0 + (u64)threadIdx.x * 16; o < o1; o += (u64)VT * 16) {
            const u32 nb = (u32)min((u64)16, o1 - o);
            uint8_t* dst = out + o;
            u64 q = o - o / per;                                           // first character at or behind output byte o
            const u64 nl1 = min((o / per + 1) * per - 1, last);            // first line feed at or behind o
            u32 nn = 0;
            if (nl1 < o + nb) {
                nn = 1;
                if (nl1 < last && min(nl1 + per, last) < o + nb) nn = 2;
            }
            if (nn == 1 && nb == 1) { dst[0] = '\n'; continue; }
            u64 i = vcf::ref_find(t.refpos, iA, iB, q), end, base;
            sym(i, end, base);
            u128 x = 0;
            if (nn <= 1 && q + (nb - nn) <= end) {                         // the chunk comes out of one string
                const uint4 v = load16u(t.chars + (base + q));               // (the pool ends in 16 bytes of slack)
                x = ((u128)(((u64)v.w << 32) | v.z) << 64) | (((u64)v.y << 32) | v.x);
                if (nn) {
                    const u32 sh = 8u * (u32)(nl1 - o);
                    const u128 mask = ((u128)1 << sh) - 1;
                    x = (x & mask) | ((u128)'\n' << sh) | ((x & ~mask) << 8);
                }
            } else {                                                       // byte by byte across strings and short lines
                u64 nl = nl1;
                for (u32 b = 0; b < nb; b++) {
                    u32 ch = '\n';
                    if (o + b == nl) nl = nl == last ? vcf::NONE : min(nl + per, last);
                    else {
                        while (q >= end && i + 1 < t.n) { i++; sym(i, end, base); }
                        ch = q < end ? t.chars[(u64)(base + q)] : (u32)'?';
                        q++;
                    }
                    x |= (u128)ch << (8u * b);
                }
            }
            if (nb == 16) {
                const u64 lo = (u64)x, hi = (u64)(x >> 64);
                *reinterpret_cast<uint4*>(dst) = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
            } else {
                for (u32 b = 0; b < nb; b++) dst[b] = (uint8_t)(x >> (8u * b));
            }
        }
    }
}

bool is_space(char ch) { return ch == ' ' || (ch >= '\t' && ch <= '\r'); }

} // namespace

void VcfExportPipeline::run(DeviceEds& de, const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n,
                            const VcfExportOpts& opts, HostBytes& vcf_out, HostBytes* fasta, VcfExportInfo& info, hipStream_t st)
{
    info = VcfExportInfo{};
    TimedRuns timed(st, &times_);

    bool bad_chrom = opts.chrom.empty();
    for (char ch : opts.chrom) bad_chrom = bad_chrom || is_space(ch);
    if (bad_chrom) throw ParamError("Chromosome name is empty or holds whitespace");
    const bool with_gt = seds != nullptr;
    if (opts.ref_path && !with_gt) throw ParamError("A reference path needs sources (.seds)");

    de.load(eds, eds_n, seds, seds_n, with_gt, st);
    const u64 n = de.n(), m = de.m();
    info.symbols = n; info.strings = m;

    // ---- counts
    u64 hctl[CT_COUNT] = {};
    hctl[CT_ERRREF] = hctl[CT_ERRANC] = vcf::NONE;
    u64 P = 0, NT = 0;
    vcf::Tab t{};
    if (m) {
        const EdsView v = de.view();
        const u32 W = v.W;
        for (DevBuf* b : {&refidx_, &refpos_, &rank_, &anchor_, &recsym_}) b->ensure(8 * (n + 1));
        ctl_.ensure(8 * CT_COUNT);
        scan_tmp_.ensure(8 * 2 * ((n + 1) / SCAN_TILE + 8));
        chrom_.ensure(opts.chrom.size());
        EDSX_HIP(hipMemcpyAsync(chrom_.ptr, opts.chrom.data(), opts.chrom.size(), hipMemcpyHostToDevice, st));
        if (with_gt) {
            orb_.ensure(8 * (size_t)W);
            EDSX_HIP(hipMemsetAsync(orb_.ptr, 0, 8 * (size_t)W, st));
            timed.run("k_vcf_or", [&] { hipLaunchKernelGGL(k_vcf_or, dim3(1024), dim3(VT), 0, st, v.bits, W, m, orb_.as<u64>()); });
            std::vector<u64> orb(W, 0);
            EDSX_HIP(hipMemcpyAsync(orb.data(), orb_.ptr, 8 * (size_t)W, hipMemcpyDeviceToHost, st));
            EDSX_HIP(hipStreamSynchronize(st));
            for (u32 w = 0; w < W; w++)
                if (orb[w]) P = 64ull * w + 63 - (u64)__builtin_clzll(orb[w]);
        }
        info.paths = P;
        if (opts.ref_path > P) {
            timed.harvest();
            throw ParamError("Path id " + std::to_string(opts.ref_path) + " out of range (1.." + std::to_string(P) + ")");
        }
        NT = with_gt && P ? P / vcf::TILE_PATHS + 1 : 0;
        hctl[CT_N1] = n + 1;
        u64 *ctl = ctl_.as<u64>(), *tmp = scan_tmp_.as<u64>(), *refidx = refidx_.as<u64>(), *refpos = refpos_.as<u64>(),
            *rank = rank_.as<u64>(), *anchor = anchor_.as<u64>(), *recsym = recsym_.as<u64>();
        EDSX_HIP(hipMemcpyAsync(ctl, hctl, sizeof(hctl), hipMemcpyHostToDevice, st));
        timed.run("k_vcf_sym", [&] {
            hipLaunchKernelGGL(k_vcf_sym, dim3(grid_for(n + 1, 8192)), dim3(VT), 0, st, v.sym.size, v.sym.ent_off, v.str_off, v.bits, W, n,
                               opts.ref_path, refidx, refpos, rank, anchor, ctl);
        });
        timed.run("scan_symbols", [&] {
            ScanSet<2> ss{{refpos, rank}, {refpos, rank}, {ctl + CT_L, ctl + CT_RECS}};
            exclusive_scan_multi<2>(ss, ctl + CT_N1, tmp, st);
        });
        t = vcf::Tab{v.sym.size, v.sym.ent_off, v.str_off, v.chars, v.bits, W, refidx, refpos, anchor, n, P,
                     chrom_.as<uint8_t>(), (u32)opts.chrom.size(), with_gt ? 1u : 0u};
        timed.run("k_vcf_anchor", [&] {
            hipLaunchKernelGGL(k_vcf_anchor, dim3(grid_for(n, 8192)), dim3(VT), 0, st, t, rank, anchor, recsym, ctl);
        });
        EDSX_HIP(hipMemcpyAsync(hctl, ctl, sizeof(hctl), hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        EDSX_HIP(hipGetLastError());
        if (hctl[CT_ERRREF] != vcf::NONE) {
            timed.harvest();
            throw ParamError("Path " + std::to_string(opts.ref_path) + " takes no string of symbol " + std::to_string(hctl[CT_ERRREF]));
        }
        if (hctl[CT_ERRANC] != vcf::NONE) {
            timed.harvest();
            throw FormatError("Symbol " + std::to_string(hctl[CT_ERRANC]) + " has an empty string and no reference base to anchor it");
        }
        const u64 R = hctl[CT_RECS];
        if (R) {
            const u64 tabn = R * (1 + NT);
            table_.ensure(8 * (tabn + 1));
            scan_tmp_.ensure(8 * 2 * ((n + 1) / SCAN_TILE + tabn / SCAN_TILE + 8));
            tmp = scan_tmp_.as<u64>();
            u64* table = table_.as<u64>();
            EDSX_HIP(hipMemcpyAsync(ctl + CT_TABN, &tabn, 8, hipMemcpyHostToDevice, st));
            timed.run("k_vcf_fixedlen", [&] {
                hipLaunchKernelGGL(k_vcf_fixedlen, dim3(grid_for(R, 8192)), dim3(VT), 0, st, t, recsym, R, NT, table, ctl);
            });
            if (NT)
                timed.run("k_vcf_count", [&] {
                    hipLaunchKernelGGL(k_vcf_count, dim3((unsigned)std::min<u64>(R * NT, 1u << 18)), dim3(64 * std::min<u32>(4, W)), 0, st,
                                       t, recsym, R, NT, table);
                });
            timed.run("scan_table", [&] { exclusive_scan_u64(table, table, ctl + CT_TABN, ctl + CT_BODY, tmp, st); });
            EDSX_HIP(hipMemcpyAsync(hctl, ctl, sizeof(hctl), hipMemcpyDeviceToHost, st));
            EDSX_HIP(hipStreamSynchronize(st));
            EDSX_HIP(hipGetLastError());
        }
    } else if (opts.ref_path) {
        throw ParamError("Path id " + std::to_string(opts.ref_path) + " out of range (1..0)");
    }
    const u64 L = hctl[CT_L], R = hctl[CT_RECS], body = hctl[CT_BODY];
    info.records = R; info.anchored = hctl[CT_ANCH]; info.overlapping = hctl[CT_OVER]; info.ref_length = L; info.body_bytes = body;

    // ---- header, on the host
    if (opts.names && opts.n_names != P)
        throw ParamError("Expected " + std::to_string(P) + " sample names, got " + std::to_string(opts.n_names));
    std::string head = "##fileformat=VCFv4.2\n##source=eds2vcf\n##contig=<ID=" + opts.chrom + ",length=" + std::to_string(L) + ">\n";
    if (with_gt) head += "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n";
    head += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO";
    if (with_gt) {
        head += "\tFORMAT";
        for (u64 p = 1; p <= P; p++) {
            const std::string name = opts.names ? std::string(opts.names[p - 1]) : opts.prefix + std::to_string(p);
            if (name.empty() || name.find_first_of("\t\n") != std::string::npos)
                throw ParamError("Sample name " + std::to_string(p - 1) + " is not a VCF sample name");
            head += "\t" + name;
        }
    }
    head += "\n";
    info.header_bytes = head.size();
    if (opts.max_bytes && body > opts.max_bytes) {
        timed.harvest();
        throw LimitError("VCF body of " + std::to_string(body) + " bytes is above the limit of " + std::to_string(opts.max_bytes));
    }

    // ---- fill: the body is sized exactly (+ 16 bytes of slack as every output buffer here)
    if (body) {
        out_.ensure(body + 16);
        uint8_t* o = out_.as<uint8_t>();
        const u64* table = table_.as<u64>();
        const u64* recsym = recsym_.as<u64>();
        timed.run("k_vcf_fixed", [&] {
            hipLaunchKernelGGL(k_vcf_fixed, dim3(grid_for(R * FIX_LANES, 1u << 16)), dim3(VT), 0, st, t, recsym, R, NT, table, o);
        });
        if (NT)
            timed.run("k_vcf_cells", [&] {
                hipLaunchKernelGGL(k_vcf_cells, dim3((unsigned)std::min<u64>(R * NT, 1u << 18)), dim3(64 * std::min<u32>(4, t.W)), 0, st, t,
                                   recsym, R, NT, table, o);
            });
    }
    const std::string fhead = ">" + opts.chrom + "\n";
    const u64 lw = (opts.line_width == 0 || opts.line_width > L) ? std::max<u64>(L, 1) : opts.line_width;
    const u64 fbody = L ? L + (L + lw - 1) / lw : 0;
    if (fasta && fbody) {
        fa_.ensure(fbody + 16);
        timed.run("k_vcf_ref", [&] {
            hipLaunchKernelGGL(k_vcf_ref, dim3((unsigned)std::min<u64>((fbody + REF_TILE - 1) / REF_TILE, 1u << 16)), dim3(VT), 0, st, t, L, lw,
                               fbody, fa_.as<uint8_t>());
        });
    }
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    timed.harvest();
    vcf_out.take(head.size() + body);
    std::memcpy(vcf_out.data, head.data(), head.size());
    PinnedDownload::copy(vcf_out.data + head.size(), out_.ptr, body, st);
    if (fasta) {
        fasta->take(fhead.size() + fbody);
        std::memcpy(fasta->data, fhead.data(), fhead.size());
        PinnedDownload::copy(fasta->data + fhead.size(), fa_.ptr, fbody, st);
    }
}

} // namespace edsx
