// msa_group_harness.hip — plain C launchers around the wave64 grouping code of the MSA transform: the helpers of
// csrc/msa_wave.hpp, fast_group<true, HEAVY> of csrc/msa_fast_kernels.hpp and fused_group_run<ROWS64> of
// csrc/msa_scan_kernels.hpp, for tests/test_msa_group_gpu.py only (edsparser_amd/libedsx_msagroup.so).
// Never loaded by the product.  Every launcher takes device pointers and a stream, enqueues and returns the
// hipGetLastError() code; it allocates nothing and keeps no state: the test owns memory, poison, margins and synchronisation.
#include "msa_scan_kernels.hpp"
#include "msa_fast_kernels.hpp"

using namespace edsx;

namespace {

// ---- fast_group: one 64-thread workgroup per segment.  out: MG_GROUP_WORDS u32 per segment - lane l at 8 l: the raw
// G.gid (4), pack_gid2 (1), pack_gid4 (2), G.rep (1); then G.k, G.sumlen, the return code, saw_nl
constexpr u32 MG_GROUP_WORDS = 64 * 8 + 4;

template <bool HEAVY>
__global__ void __launch_bounds__(64) k_mg_group(const MsaView* __restrict__ mvp, const u64* __restrict__ cmeta_l, const u64* __restrict__ seg_a_l,
                                                 u32* __restrict__ out, u64 n)
{
    __shared__ uint8_t strs[HEAVY ? 8192 : 4];
    const u64 seg = blockIdx.x;
    if (seg >= n) return;
    const MsaView mv = *mvp;
    const u32 lane = threadIdx.x & 63;
    // as k_seg_group prepares them
    const uint4 vmask = fast_valid_mask(lane, mv.S);
    const u32 loff = lane * 16u < mv.Spad - 16u ? lane * 16u : mv.Spad - 16u;
    const u64 cmeta = uniform64(cmeta_l[seg]);
    const uint4 col0 = load16u(mv.vc + (cmeta & CNT_SLOT) * (u64)mv.Spad + loff);
    const u32 rb = lane < mv.S ? (u32)mv.vc[(cmeta & CNT_SLOT) * (u64)mv.Spad + lane] : 0u;
    u32 saw_nl = 0;
    FastGroups G;
    const int rc = fast_group<true, HEAVY>(mv, (cmeta & (CNT_SCATTER | CNT_MIXED)) ? uniform64(seg_a_l[seg]) : 0, cmeta, col0, rb, lane, vmask, G,
                                           saw_nl, strs);
    const u32 any_nl = ballot64(saw_nl != 0) ? 1u : 0u;        // (set per lane by some paths: the product ORs it into the status)
    u32* o = out + seg * (u64)MG_GROUP_WORDS;
    const uint2 p4 = pack_gid4(G.gid, vmask);
    u32* l = o + lane * 8u;
    l[0] = G.gid.x; l[1] = G.gid.y; l[2] = G.gid.z; l[3] = G.gid.w;
    l[4] = pack_gid2(G.gid, vmask); l[5] = p4.x; l[6] = p4.y; l[7] = G.rep;
    if (lane == 0) { o[512] = G.k; o[513] = G.sumlen; o[514] = (u32)rc; o[515] = any_nl; }
}

// ---- fused_group_run: one 64-thread workgroup per run; the column image is copied to LDS first (colbuf is LDS in the scan)
template <bool ROWS64>
__global__ void __launch_bounds__(64) k_mg_fused(const K1Params* __restrict__ pp, const uint8_t* __restrict__ cols, const u32* __restrict__ desc,
                                                 const u64* __restrict__ slot_base, u32 ncols, u64 n)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t colbuf[];
    const u64 run = blockIdx.x;
    if (run >= n) return;
    const K1Params p = *pp;
    const u32 lane = threadIdx.x & 63;
    for (u32 o = lane * 16u; o < ncols * p.Spad; o += 1024u)
        *reinterpret_cast<uint4*>(colbuf + o) = *reinterpret_cast<const uint4*>(cols + o);
    __syncthreads();
    // as k_scan_extract prepares them
    const u32 nl = (p.S + 15u) >> 4;
    const uint4 vmask = fast_valid_mask(lane, p.S);
    const u32 loff = lane * 16u < p.Spad - 16u ? lane * 16u : p.Spad - 16u;
    fused_group_run<ROWS64>(p, colbuf, uniform32(desc[run]), uniform64(slot_base[run]), lane, vmask, nl, loff);
}

// ---- wave helpers: one 64-thread workgroup per vector of (a, b, c, d) per lane; MG_WAVE_WORDS u32 per lane
constexpr u32 MG_WAVE_WORDS = 12;

__global__ void __launch_bounds__(64) k_mg_wave(const u32* __restrict__ in, u32* __restrict__ out, u64 n)
{
    const u64 v = blockIdx.x;
    if (v >= n) return;
    const u32 lane = threadIdx.x & 63;
    const u32* i = in + (v * 64 + lane) * 4;
    const u32 a = i[0], b = i[1], c = i[2], d = i[3];
    u32* o = out + (v * 64 + lane) * (u64)MG_WAVE_WORDS;
    o[0] = wave_scan_incl(a);
    u32 sa = a, sb = b, sc = c, sd = d;
    wave_scan_incl4(sa, sb, sc, sd);
    o[1] = sa; o[2] = sb; o[3] = sc; o[4] = sd;
    o[5] = wave_xor_all(a);
    o[6] = wave_or_all(a);
    o[7] = min_lanes8(a);
    const u64 ab = ((u64)b << 32) | a;
    const int src = (int)(uniform32(c) & 63u);                  // the source lane: lane 0's c
    const u64 r = readlane64(ab, src), u = uniform64(ab);
    o[8] = (u32)r; o[9] = (u32)(r >> 32); o[10] = (u32)u; o[11] = (u32)(u >> 32);
}

// leader_byte at every (leader, index) of one vector of uint4 per lane: out[(leader * 16 + index) * 64 + lane]
__global__ void __launch_bounds__(64) k_mg_leader(const uint4* __restrict__ in, u32* __restrict__ out)
{
    const u32 lane = threadIdx.x & 63;
    const uint4 v = in[lane];
    for (int leader = 0; leader < 64; leader++)
        for (u32 idx = 0; idx < 16; idx++) out[((u32)leader * 16u + idx) * 64u + lane] = leader_byte(v, leader, idx);
}

// ---- byte helpers: one thread per item.  Item: uint4 a, b, c; u32 x, lane, S, pad.  MG_BYTES_WORDS u32 out per item.
constexpr u32 MG_BYTES_WORDS = 56;
struct MgBytesIn { uint4 a, b, c; u32 x, lane, S, pad; };

__global__ void __launch_bounds__(256) k_mg_bytes(const MgBytesIn* __restrict__ in, const u32* __restrict__ table, u32* __restrict__ out, u64 n)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const MgBytesIn it = in[i];
    const uint4 a = it.a, b = it.b, c = it.c;
    u32* o = out + i * (u64)MG_BYTES_WORDS;
    auto put4 = [&](u32 at, const uint4& v) { o[at] = v.x; o[at + 1] = v.y; o[at + 2] = v.z; o[at + 3] = v.w; };
    o[0] = bytes_ne_mask(a.x, b.x);
    put4(1, bytes_eq_mask(a, it.x));
    o[5] = first_byte_index(a);
    o[6] = chunk_ne16(a, b);
    o[7] = chunk_eq16(a, it.x);
    uint4 acc = c;
    acc_or_xor(acc, a, b);
    put4(8, acc);
    u32 saw = 0, saw2 = 0;
    put4(12, normalise_col<true>(a, c, saw));
    o[16] = saw;
    put4(17, normalise_col<false>(a, c, saw2));
    o[21] = any_nul(a, c) ? 1u : 0u;
    o[22] = byte_at<0>(a); o[23] = byte_at<1>(a); o[24] = byte_at<2>(a); o[25] = byte_at<3>(a);
    o[26] = byte_at<4>(a); o[27] = byte_at<5>(a); o[28] = byte_at<6>(a); o[29] = byte_at<7>(a);
    o[30] = byte_at<8>(a); o[31] = byte_at<9>(a); o[32] = byte_at<10>(a); o[33] = byte_at<11>(a);
    o[34] = byte_at<12>(a); o[35] = byte_at<13>(a); o[36] = byte_at<14>(a); o[37] = byte_at<15>(a);
    put4(38, fast_valid_mask(it.lane, it.S));
    const uint4 cls = dna_classes(a);
    put4(42, cls);
    o[46] = dna_bad(a, cls, c);
    o[47] = pack_gid2(a, c);
    const uint2 p4 = pack_gid4(a, c);
    o[48] = p4.x; o[49] = p4.y;
    u32 t[16];
#pragma unroll
    for (int k = 0; k < 16; k++) t[k] = table[k];
    o[50] = lutN<8>(t, a.x); o[51] = lutN<16>(t, a.x); o[52] = lutN<32>(t, a.x); o[53] = lutN<64>(t, a.x);
    o[54] = saw2; o[55] = 0;
}

} // namespace

extern "C" {

// sizes the test's mirror of the structs and of the output records is checked against
// 0: MsaView, 1: K1Params, 2: u32 per segment of mg_group, 3: u32 per lane of mg_wave, 4: u32 per item of mg_bytes, 5: the item
u64 mg_sizeof(int what)
{
    switch (what) {
    case 0: return sizeof(MsaView);
    case 1: return sizeof(K1Params);
    case 2: return MG_GROUP_WORDS;
    case 3: return MG_WAVE_WORDS;
    case 4: return MG_BYTES_WORDS;
    case 5: return sizeof(MgBytesIn);
    }
    return 0;
}

// fast_group<true, heavy> of n segments: descriptor cmeta[i], first column seg_a[i] (read for CNT_SCATTER / CNT_MIXED only)
int mg_group(int heavy, const MsaView* mv, const u64* cmeta, const u64* seg_a, u32* out, u64 n, hipStream_t st)
{
    if (n) {
        if (heavy) hipLaunchKernelGGL(k_mg_group<true>, dim3((unsigned)n), dim3(64), 0, st, mv, cmeta, seg_a, out, n);
        else hipLaunchKernelGGL(k_mg_group<false>, dim3((unsigned)n), dim3(64), 0, st, mv, cmeta, seg_a, out, n);
    }
    return (int)hipGetLastError();
}

// fused_group_run<rows64> of n runs over an image of ncols columns of spad bytes (spad = p->Spad; at most 64 KiB in all)
int mg_fused(int rows64, const K1Params* p, const uint8_t* cols, const u32* desc, const u64* slot_base, u32 ncols, u32 spad, u64 n, hipStream_t st)
{
    const size_t lds = (size_t)ncols * spad;
    if (lds == 0 || lds > 65536 || spad % 16) return (int)hipErrorInvalidValue;
    if (n) {
        if (rows64) hipLaunchKernelGGL(k_mg_fused<true>, dim3((unsigned)n), dim3(64), lds, st, p, cols, desc, slot_base, ncols, n);
        else hipLaunchKernelGGL(k_mg_fused<false>, dim3((unsigned)n), dim3(64), lds, st, p, cols, desc, slot_base, ncols, n);
    }
    return (int)hipGetLastError();
}

// n vectors of 64 x (a, b, c, d); out_leader (may be null): leader_byte over leader_in[64] at every (leader, index)
int mg_wave(const u32* in, u32* out, u64 n, const uint4* leader_in, u32* out_leader, hipStream_t st)
{
    if (n) hipLaunchKernelGGL(k_mg_wave, dim3((unsigned)n), dim3(64), 0, st, in, out, n);
    if (out_leader) hipLaunchKernelGGL(k_mg_leader, dim3(1), dim3(64), 0, st, leader_in, out_leader);
    return (int)hipGetLastError();
}

// n items; table: 16 u32 (64 entries of one byte) for lutN
int mg_bytes(const void* in, const u32* table, u32* out, u64 n, hipStream_t st)
{
    if (n) hipLaunchKernelGGL(k_mg_bytes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, static_cast<const MgBytesIn*>(in), table, out, n);
    return (int)hipGetLastError();
}

} // extern "C"
