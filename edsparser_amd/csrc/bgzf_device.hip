// bgzf_device.hip — BGZF input inflated on the device.
//
// A BGZF file is a chain of gzip members of at most 64 KiB of text each, every one an independent DEFLATE stream: the
// blocks supply the parallelism (10^4 - 10^6 of them in a real input), the Huffman chain inside one block is serial.
//
//   k_bgzf_inflate   one wave per BGZF block.  Per DEFLATE block the wave builds the decode tables in LDS (lane 0 reads
//                    the code lengths and sorts the symbols, all lanes fill the direct tables); then, batch after batch,
//                    lane 0 walks the bit stream into a token list (literal | length, distance) and the whole wave places
//                    the batch: output offsets from a wave scan, literals by one store per lane, matches by all lanes,
//                    dist < len handled by the period of the overlap.  The output window is a 32 KiB ring in LDS
//                    (DEFLATE's reach): matches read the ring, never global memory the wave has just written, and the
//                    ring goes to HBM in 16-byte stores.  37 928 bytes (37.0 KiB) of LDS per wave: 4 waves per CU.
//   k_bgzf_crc       CRC-32 of every block's text: 64 lanes take 1 KiB chunks, chunk i is multiplied by
//                    x^(8 * bytes behind it) mod the CRC polynomial, the products are XORed and compared with the trailer.
//
// Both kernels write one status word per block; the host reports the lowest failing block.  Every compressed read is
// bounded by the block's end (BitReader), every write by its ISIZE (checked per token before it enters the list).
#include "bgzf_device.hpp"
#include "dev_util.hpp"

#include <chrono>

namespace edsx {

using namespace gz;

namespace {

constexpr u32 RING = 32768, RMASK = RING - 1, MAXTOK = 256, BATCH_OUT = 4096;
enum : u32 { ST_OK = 0, ST_STREAM = 2, ST_LENGTH = 3, ST_CRC = 4 };
enum : u32 { C_KIND = 0, C_FINAL, C_A, C_B, C_NTOK, C_EOB, C_ERR, C_OUT };

struct InflShared {
    uint8_t ring[RING];
    u32 tok[MAXTOK];
    LitTable lit;
    DistTable dist;
    ClenTable clen;
    uint8_t lens[320];
    u32 ctl[8];
};
static_assert(sizeof(InflShared) <= 40 * 1024, "4 waves per CU: 160 KiB of LDS");

} // namespace

// ring bytes [flushed, produced) to out: bytes up to the first 16-byte boundary of the global address (a16), then
// 16-byte stores (the ring is read as aligned dwords and shifted), and at the end of the block the last bytes
__device__ __forceinline__ void flush_ring(const uint8_t* ring, uint8_t* __restrict__ out, u32& flushed, u32 produced, u32 a16, bool last,
                                           u32 lane)
{
    if (flushed < a16) {
        const u32 e = a16 < produced ? a16 : produced;
        for (u32 j = flushed + lane; j < e; j += 64) out[j] = ring[j & RMASK];
        flushed = e;
        if (flushed < a16) return;
    }
    const u32* r32 = reinterpret_cast<const u32*>(ring);
    const u32 nvec = (produced - flushed) >> 4, sh = (flushed & 3u) * 8u;
    for (u32 k = lane; k < nvec; k += 64) {
        const u32 pos = flushed + 16u * k, w = (pos & RMASK) >> 2;
        u32 d[5];
#pragma unroll
        for (u32 t = 0; t < 5; t++) d[t] = r32[(w + t) & (RING / 4 - 1)];
        uint4 v;
        if (sh == 0) v = make_uint4(d[0], d[1], d[2], d[3]);
        else v = make_uint4((d[0] >> sh) | (d[1] << (32 - sh)), (d[1] >> sh) | (d[2] << (32 - sh)), (d[2] >> sh) | (d[3] << (32 - sh)),
                            (d[3] >> sh) | (d[4] << (32 - sh)));
        *reinterpret_cast<uint4*>(out + pos) = v;
    }
    flushed += 16u * nvec;
    if (last) {
        for (u32 j = flushed + lane; j < produced; j += 64) out[j] = ring[j & RMASK];
        flushed = produced;
    }
}

static __global__ void __launch_bounds__(64) k_bgzf_inflate(const uint8_t* __restrict__ comp, const BgzfBlock* __restrict__ tab, u64 nblocks,
                                                            uint8_t* __restrict__ text, u32* __restrict__ status)
{
    __shared__ __attribute__((aligned(16))) InflShared sh;
    const u32 lane = threadIdx.x;
    for (u64 b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const BgzfBlock blk = tab[b];
        const uint8_t* p = comp + blk.comp_off;
        uint8_t* out = text + blk.out_off;
        const u32 isize = blk.isize;
        const u32 a16 = (16u - (u32)(blk.out_off & 15u)) & 15u;
        u32 err = ST_OK, produced = 0, flushed = 0;
        u64 cbeg = 0, cend = 0;
        if (blk.comp_len < 20) err = ST_STREAM;
        else {
            cbeg = 12ull + (p[10] | ((u32)p[11] << 8));
            cend = blk.comp_len - 8;
            if (cbeg > cend) err = ST_STREAM;
        }
        BitReader br;                                           // (lane 0's copy walks the stream)
        br.init(p, cbeg, err ? cbeg : cend);
        u32 pending = 0;
        bool has_pending = false, done = err != ST_OK;
        while (!done) {
            // ---- block header, and a dynamic block's code lengths: lane 0
            if (lane == 0) {
                BlockHeader h;
                read_block_header(br, h);
                u32 a = 0, c = 0;
                if (!br.err) {
                    if (h.type == 0) {
                        a = (u32)br.byte_pos(); c = h.stored_len;
                        br.skip_bytes(h.stored_len);
                    } else if (h.type == 2) {
                        read_dynamic_lengths(br, h, sh.clen, sh.lens);
                        a = h.nlen; c = h.ndist;
                    } else { a = 288; c = 30; }
                }
                sh.ctl[C_KIND] = h.type; sh.ctl[C_FINAL] = h.final_block; sh.ctl[C_A] = a; sh.ctl[C_B] = c;
                sh.ctl[C_ERR] = br.err ? ST_STREAM : ST_OK;
            }
            __syncthreads();
            const u32 kind = sh.ctl[C_KIND], fin = sh.ctl[C_FINAL], ca = sh.ctl[C_A], cb = sh.ctl[C_B];
            err = sh.ctl[C_ERR];
            if (err) break;
            if (kind == 0) {
                // ---- stored: the raw bytes through the ring, a batch at a time
                if (produced + cb > isize) { err = ST_LENGTH; break; }
                for (u32 c = 0; c < cb; c += BATCH_OUT) {
                    const u32 m = cb - c < BATCH_OUT ? cb - c : BATCH_OUT;
                    for (u32 j = lane; j < m; j += 64) sh.ring[(produced + j) & RMASK] = p[ca + c + j];
                    __syncthreads();
                    produced += m;
                    flush_ring(sh.ring, out, flushed, produced, a16, false, lane);
                    __syncthreads();
                }
            } else {
                // ---- the two codes: symbols sorted by lane 0, direct tables filled by all lanes
                if (kind == 1) fixed_lengths(sh.lens, (int)lane, 64);
                __syncthreads();
                if (lane == 0) {
                    const int ll = huff_prepare(sh.lit, sh.lens, (int)ca), dl = huff_prepare(sh.dist, sh.lens + ca, (int)cb);
                    sh.ctl[C_ERR] = codes_acceptable(ll, dl, sh.lit, sh.dist, ca, cb, kind == 1) ? ST_OK : ST_STREAM;
                }
                huff_clear_fast(sh.lit, (int)lane, 64);
                huff_clear_fast(sh.dist, (int)lane, 64);
                __syncthreads();
                err = sh.ctl[C_ERR];
                if (err) break;
                huff_fill_fast(sh.lit, sh.lens, (int)lane, 64);
                huff_fill_fast(sh.dist, sh.lens + ca, (int)lane, 64);
                __syncthreads();
                for (;;) {
                    // ---- lane 0: the next batch of tokens.  A batch ends at MAXTOK tokens, BATCH_OUT bytes, the end of the
                    // block, or where a literal placed with the batch would land on ring bytes one of its matches still
                    // has to read (batch end <= match position - distance + RING; a match that breaks this alone goes alone)
                    if (lane == 0) {
                        u32 nt = 0, bo = 0, eob = 0, e = ST_OK, limit = 0xffffffffu;
                        while (nt < MAXTOK && bo < BATCH_OUT) {
                            u32 t;
                            if (has_pending) { t = pending; has_pending = false; }
                            else t = next_token(br, sh.lit, sh.dist);
                            if (t == TOK_ERROR) { e = ST_STREAM; break; }
                            if (t == TOK_END) { eob = 1; break; }
                            const u32 pos = produced + bo;
                            u32 l = 1, nl = limit;
                            if (t & TOK_MATCH) {
                                l = tok_len(t);
                                const u32 d = tok_dist(t);
                                if (d > pos) { e = ST_STREAM; break; }
                                const u32 lim = pos - d + RING;
                                nl = lim < limit ? lim : limit;
                            }
                            if (pos + l > isize) { e = ST_LENGTH; break; }
                            if (pos + l > nl) {
                                if (nt) { pending = t; has_pending = true; }
                                else { sh.tok[nt++] = t; bo += l; }
                                break;
                            }
                            limit = nl;
                            sh.tok[nt++] = t; bo += l;
                        }
                        sh.ctl[C_NTOK] = nt; sh.ctl[C_EOB] = eob; sh.ctl[C_ERR] = e; sh.ctl[C_OUT] = bo;
                    }
                    __syncthreads();
                    const u32 ntok = sh.ctl[C_NTOK], eob = sh.ctl[C_EOB], bout = sh.ctl[C_OUT];
                    err = sh.ctl[C_ERR];
                    if (err) break;
                    // ---- the wave places the batch: offsets by a scan over the token lengths, literals first
                    u32 tk[4], off[4];
                    u32 base = produced;
#pragma unroll
                    for (u32 r = 0; r < 4; r++) {
                        const u32 i = r * 64 + lane;
                        const u32 t = i < ntok ? sh.tok[i] : 0u;
                        const u32 l = i < ntok ? ((t & TOK_MATCH) ? tok_len(t) : 1u) : 0u;
                        u32 incl = l;
                        for (int o = 1; o < 64; o <<= 1) { const u32 x = __shfl_up(incl, o, 64); if (lane >= (u32)o) incl += x; }
                        tk[r] = i < ntok ? t : 0u;
                        off[r] = base + incl - l;
                        if (i < ntok && !(t & TOK_MATCH)) sh.ring[off[r] & RMASK] = (uint8_t)t;
                        base += __shfl(incl, 63, 64);
                    }
                    __syncthreads();
                    // matches in stream order, each copied by all lanes from the ring; every source byte lies in front of
                    // the match (dist < len: the match repeats its first dist bytes)
#pragma unroll
                    for (u32 r = 0; r < 4; r++) {
                        u64 mm = ballot64((tk[r] & TOK_MATCH) != 0);
                        while (mm) {
                            const int m = __builtin_ctzll(mm);
                            mm &= mm - 1;
                            const u32 t = __shfl(tk[r], m, 64), o = __shfl(off[r], m, 64);
                            const u32 len = tok_len(t), d = tok_dist(t);
                            for (u32 j0 = 0; j0 < len; j0 += 64) {
                                const u32 j = j0 + lane;
                                uint8_t v = 0;
                                if (j < len) v = sh.ring[(o - d + (d < len ? j % d : j)) & RMASK];
                                if (j < len) sh.ring[(o + j) & RMASK] = v;
                            }
                            __syncthreads();
                        }
                    }
                    produced += bout;
                    flush_ring(sh.ring, out, flushed, produced, a16, false, lane);
                    __syncthreads();
                    if (eob) break;
                }
                if (err) break;
            }
            if (fin) done = true;
        }
        flush_ring(sh.ring, out, flushed, produced, a16, true, lane);
        if (lane == 0) {
            u32 e = err;
            if (!e) { br.align(); if (br.err || br.byte_pos() != cend) e = ST_STREAM; }
            if (!e && produced != isize) e = ST_LENGTH;
            status[b] = e;
        }
        __syncthreads();
    }
}

static __global__ void __launch_bounds__(64) k_bgzf_crc(const uint8_t* __restrict__ comp, const BgzfBlock* __restrict__ tab, u64 nblocks,
                                                        const uint8_t* __restrict__ text, u32* __restrict__ status)
{
    __shared__ u32 T[256];
    __shared__ u32 x2n[32];
    const u32 lane = threadIdx.x;
    for (u32 i = lane; i < 256; i += 64) T[i] = crc_table_entry(i);
    if (lane == 0) crc_x2n_table(x2n);
    __syncthreads();
    constexpr u32 CHUNK = 1024;                                  // 64 lanes x 1 KiB = the largest BGZF block
    for (u64 b = blockIdx.x; b < nblocks; b += gridDim.x) {
        if (status[b] != ST_OK) continue;
        const BgzfBlock blk = tab[b];
        const uint8_t* t = text + blk.out_off;
        const u32 isize = blk.isize;
        const u32 lo = lane * CHUNK < isize ? lane * CHUNK : isize, hi = lo + CHUNK < isize ? lo + CHUNK : isize;
        u32 c = 0xffffffffu, i = lo;
        for (; i + 16 <= hi; i += 16) {
            const uint4 v = load16u(t + i);
#pragma unroll
            for (int k = 0; k < 16; k++) c = T[(c ^ byte_of(v, k)) & 0xffu] ^ (c >> 8);
        }
        for (; i < hi; i++) c = T[(c ^ t[i]) & 0xffu] ^ (c >> 8);
        c = hi > lo ? ~c : 0u;
        u32 v = c ? crc_mulmod(crc_xpow_bytes(x2n, isize - hi), c) : 0u;
        for (int o = 32; o > 0; o >>= 1) v ^= __shfl_xor(v, o, 64);
        const uint8_t* q = comp + blk.comp_off + blk.comp_len - 8;
        const u32 want = q[0] | ((u32)q[1] << 8) | ((u32)q[2] << 16) | ((u32)q[3] << 24);
        if (lane == 0 && v != want) status[b] = ST_CRC;
    }
}

// ---- host --------------------------------------------------------------------------------------------------
namespace {

double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

void inflate_on_device(const uint8_t* data, size_t size, const std::vector<BgzfBlock>& blocks, u64 text_size, const char* what, GzText& out,
                       GzInfo& info, hipStream_t st)
{
    const u64 nb = blocks.size();
    DevBuf d_comp, d_tab, d_status;
    d_comp.ensure(size + 16);
    d_tab.ensure(sizeof(BgzfBlock) * (nb + 1));
    d_status.ensure(4 * (nb + 1));
    out.dev.ensure(text_size + 16);
    EDSX_HIP(hipMemcpyAsync(d_comp.ptr, data, size, hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemcpyAsync(d_tab.ptr, blocks.data(), sizeof(BgzfBlock) * nb, hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemsetAsync(d_status.ptr, 0xff, 4 * (nb + 1), st));
    info.h2d_bytes = size + sizeof(BgzfBlock) * nb;
    struct Events {                                              // destroyed on every way out
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
        ~Events() { for (auto e : ev) if (e) (void)hipEventDestroy(e); }
    } evs;
    hipEvent_t* ev = evs.ev;
    for (int i = 0; i < 3; i++) EDSX_HIP(hipEventCreate(&ev[i]));
    const unsigned grid = (unsigned)std::min<u64>(nb, 1u << 16);
    EDSX_HIP(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(k_bgzf_inflate, dim3(grid), dim3(64), 0, st, d_comp.as<uint8_t>(), d_tab.as<BgzfBlock>(), nb, out.dev.as<uint8_t>(),
                       d_status.as<u32>());
    EDSX_HIP(hipEventRecord(ev[1], st));
    hipLaunchKernelGGL(k_bgzf_crc, dim3(grid), dim3(64), 0, st, d_comp.as<uint8_t>(), d_tab.as<BgzfBlock>(), nb, out.dev.as<uint8_t>(),
                       d_status.as<u32>());
    EDSX_HIP(hipEventRecord(ev[2], st));
    std::vector<u32> status(nb);
    EDSX_HIP(hipMemcpyAsync(status.data(), d_status.ptr, 4 * nb, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    float a = 0, b = 0;
    EDSX_HIP(hipEventElapsedTime(&a, ev[0], ev[1]));
    EDSX_HIP(hipEventElapsedTime(&b, ev[1], ev[2]));
    info.inflate_ms = a; info.crc_ms = b;
    for (u64 k = 0; k < nb; k++) {                               // the lowest failing block
        if (status[k] == ST_OK) continue;
        const char* why = status[k] == ST_CRC ? "CRC mismatch" : status[k] == ST_LENGTH ? "length mismatch"
                        : status[k] == ST_STREAM ? "invalid DEFLATE stream" : nullptr;
        if (!why) throw DeviceError("BGZF inflate: block " + std::to_string(k) + " has no status");
        throw FormatError(gz_error_text(what, k, blocks[k].comp_off, why));
    }
    out.on_device = true;
    out.n = text_size;
    info.inflated_on_device = 1;
}

} // namespace

void gz_open(const uint8_t* data, size_t size, const char* what, GzText& out, GzInfo& info, hipStream_t st)
{
    info = GzInfo();
    info.comp_bytes = size;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<BgzfBlock> blocks;
    u64 text_size = 0;
    const GzKind kind = gz_walk(data, size, text_size, [&](const BgzfBlock& b) { blocks.push_back(b); });
    info.index_ms = ms_since(t0);
    info.kind = (int)kind;
    if (kind == GZ_PLAIN) {
        out.plain = data; out.n = size;
        info.text_bytes = size;
        return;
    }
    if (kind == GZ_BGZF && !blocks.empty()) {
        info.blocks = blocks.size();
        info.text_bytes = text_size;
        inflate_on_device(data, size, blocks, text_size, what, out, info, st);
        return;
    }
    const auto t1 = std::chrono::steady_clock::now();
    std::string err;
    u64 members = 0;
    if (!gz_inflate_host(data, size, out.host, what, err, &members)) throw FormatError(err);
    info.inflate_ms = ms_since(t1);
    info.blocks = members;
    out.on_host = true;
    out.n = out.host.size();
    info.text_bytes = out.n;
}

} // namespace edsx
