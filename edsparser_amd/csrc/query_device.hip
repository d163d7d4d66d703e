// query_device.hip — the query side of an EDS on gfx950: pattern sampling and position checks.
//
// Replaces the reference's one-pattern-at-a-time loops (src/cpp/lib/formats/eds.cpp):
//   generate_patterns :673-769                      -> k_pat_sample, one lane per pattern
//   check_position :953-1047 + helpers :1051-1418   -> k_pat_check, one lane per query
// Both read a loaded DeviceEds through its view (eds_device.hpp: per symbol size, first string, single-string length;
// per string str_off into the character pool; with sources the path bitsets, W words, bit 0 = universal)
// plus two exclusive scans built here:
//   cum_common[i]  common characters in front of symbol i (n+1 entries; the reference's cum_common_positions)
//   cum_deg[i]     degenerate strings in front of symbol i (n+1 entries; cum_degenerate_counts)
// The draws are edsx::pattern_draw (draw.hpp), shared with EDS::generate_patterns(os, count, length, seed): for the same
// seed both write the same bytes.
#include "query_device.hpp"
#include "kernel_times.hpp"

#include <chrono>
#include <cstring>

namespace edsx {

namespace {

// per-symbol common length and degenerate size, scanned in place into cum_common / cum_deg
__global__ void k_q_flags(const u64* __restrict__ size, const u64* __restrict__ len1, u64 n, u64* __restrict__ cc,
                          u64* __restrict__ cd)
{
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 sz = size[i];
        cc[i] = sz == 1 ? len1[i] : 0;
        cd[i] = sz > 1 ? sz : 0;
    }
}

// ---- sampling ------------------------------------------------------------------------------------------------
// The start symbol is upper_bound(cum_common, p) - 1.  A sampled top level of cum_common sits in LDS (every stride-th
// entry), so the dependent chain of HBM loads is log2(stride) instead of log2(n).
constexpr int NTOP = 1024;
constexpr u64 NONE = ~0ull;

struct SampleArgs {
    const u64* size; const u64* ent_off; const u64* str_off; const uint8_t* chars; const u64* cc; const u64* cd;
    u64 n, C, seed, i0, cnt; u32 L;
    uint8_t* out;                          // cnt * (L + 1) bytes (pass 1)
    u64* wpos; u64* wcnt;                  // per pattern (pass 1, nullable)
    const u64* woff; int32_t* wdeg;        // chunk CSR of the chosen degenerate strings (pass 2)
    u64* err;                              // min over (pattern << 40 | symbol) of wraps without a non-empty string
};

__device__ __forceinline__ void load_top(const u64* __restrict__ cc, u64 n, u64 stride, u64* top)
{
    for (u32 j = threadIdx.x; j < (u32)NTOP; j += blockDim.x) top[j] = (u64)j * stride <= n ? cc[(u64)j * stride] : NONE;
    __syncthreads();
}

// last x with cc[x] <= p, for p < cc[n]: a common symbol of positive length
__device__ __forceinline__ u64 find_start(const u64* __restrict__ cc, u64 n, u64 stride, const u64* top, u64 p)
{
    u32 lo_t = 0, hi_t = NTOP;                                 // top[lo_t] <= p (top[0] = 0)
    while (hi_t - lo_t > 1) { const u32 mid = (lo_t + hi_t) >> 1; if (top[mid] <= p) lo_t = mid; else hi_t = mid; }
    u64 lo = (u64)lo_t * stride, hi = lo + stride;             // cc[lo] <= p < cc[hi]
    if (hi > n) hi = n;
    while (hi - lo > 1) { const u64 mid = lo + ((hi - lo) >> 1); if (cc[mid] <= p) lo = mid; else hi = mid; }
    return lo;
}

// pass 1 (FILL = false): pattern bytes, witness start and choice count; pass 2 (FILL = true, witnesses only): the
// chosen degenerate string numbers, by the same walk.
template <bool FILL>
__global__ void __launch_bounds__(256) k_pat_sample(SampleArgs a)
{
    __shared__ u64 top[NTOP];
    const u64 stride = (a.n + 1 + NTOP - 1) / NTOP;
    if (a.C > 0) load_top(a.cc, a.n, stride, top);
    const u64 rec = (u64)a.L + 1;
    for (u64 t = blockIdx.x * (u64)blockDim.x + threadIdx.x; t < a.cnt; t += (u64)gridDim.x * blockDim.x) {
        const u64 i = a.i0 + t;
        u64 cur = 0, offset = 0, p = NONE;
        if (a.C > 0) {
            p = pattern_draw(a.seed, i, 0, a.C);
            cur = find_start(a.cc, a.n, stride, top, p);
            offset = p - a.cc[cur];
        }
        u64 k = 1, got = 0, nch = 0;
        u64 cap = 0, w0 = 0;
        if (FILL) { w0 = a.woff[t]; cap = a.woff[t + 1] - w0; }
        uint8_t* o = a.out + t * rec;
        bool first = true;
        while (got < a.L && cur < a.n) {
            const u64 sz = a.size[cur];
            if (sz == 0) { cur++; first = false; continue; }      // (:713; the tokenisers never make one)
            const u64 j = pattern_draw(a.seed, i, k++, sz);
            const u64 sid = a.ent_off[cur] + j;
            const u64 s0 = a.str_off[sid], len = a.str_off[sid + 1] - s0;
            const u64 from = first ? offset : 0;
            if (from < len) {
                const u64 take = min(a.L - got, len - from);
                if (!FILL) for (u64 q = 0; q < take; q++) o[got + q] = a.chars[s0 + from + q];
                got += take;
            }
            if (sz > 1) {
                if (FILL && nch < cap) a.wdeg[w0 + nch] = (int32_t)(a.cd[cur] + j);
                nch++;
            }
            first = false;
            if (got < a.L) cur++;
        }
        if (FILL) continue;
        const bool wrapped = got < a.L;
        while (got < a.L) {                                        // wrap (:747): a uniform non-empty string of symbol got % n
            const u64 w = got % a.n, e0 = a.ent_off[w], sz = a.size[w];
            u64 ne = 0;
            for (u64 q = 0; q < sz; q++) ne += a.str_off[e0 + q + 1] > a.str_off[e0 + q];
            if (ne == 0) { atomicMin((unsigned long long*)a.err, (unsigned long long)((t << 40) | w)); break; }
            u64 j = pattern_draw(a.seed, i, k++, ne), sid = e0;
            for (u64 q = 0; q < sz; q++) {
                if (a.str_off[e0 + q + 1] == a.str_off[e0 + q]) continue;
                if (j-- == 0) { sid = e0 + q; break; }
            }
            const u64 s0 = a.str_off[sid], take = min(a.L - got, a.str_off[sid + 1] - s0);
            for (u64 q = 0; q < take; q++) o[got + q] = a.chars[s0 + q];
            got += take;
        }
        o[a.L] = '\n';
        const bool witness = !wrapped && a.C > 0;
        if (a.wpos) { a.wpos[t] = witness ? p : NONE; a.wcnt[t] = witness ? nch : 0; }
    }
}

// ---- position checks -----------------------------------------------------------------------------------------
struct CheckArgs {
    const u64* size; const u64* ent_off; const u64* str_off; const uint8_t* chars; const u64* bits; u32 W;
    const u64* cc; const u64* cd; u64 n, C, D;
    u64 nq; const u64* pos; const u64* coff; const int32_t* ch; u64 nch; const u64* poff; const uint8_t* pat; u64 npat;
    int8_t* status;
};

// One lane per query.  Pass 1 walks the symbols as reconstruct_from_memory does (:1141-1209): it validates every choice
// (decode_degenerate_string_number :1051-1095, with the pins of EDS::check_position) and compares characters, but keeps
// walking after a mismatch, since an error met later wins (:1047 compares at the end).  With sources, the walk of
// calculate_path_intersection (:1300-1418) visits the same symbols: its first empty step E is found word by word (the
// lane re-walks the T valid steps once per 64-bit word: no W-word accumulator; first_empty_step, query_device.hpp), and an
// error at step T counts only when E >= T.
__global__ void __launch_bounds__(256) k_pat_check(CheckArgs a)
{
    for (u64 q = blockIdx.x * (u64)blockDim.x + threadIdx.x; q < a.nq; q += (u64)gridDim.x * blockDim.x) {
        const u64 c0 = a.coff[q], c1 = a.coff[q + 1], p0 = a.poff[q], p1 = a.poff[q + 1];
        if (c1 < c0 || c1 > a.nch || p1 < p0 || p1 > a.npat) { a.status[q] = -2; continue; }   // malformed CSR
        const u64 L = p1 - p0, nc = c1 - c0, pos = a.pos[q];
        if (L == 0) { a.status[q] = 1; continue; }
        if (pos >= a.C) { a.status[q] = 0; continue; }
        u64 lo = 0, hi = a.n;                                  // last symbol with cc <= pos (cc[0] = 0 <= pos < cc[n])
        while (hi - lo > 1) { const u64 mid = lo + ((hi - lo) >> 1); if (a.cc[mid] <= pos) lo = mid; else hi = mid; }
        const u64 s = lo, offset = pos - a.cc[s];
        const int32_t* ch = a.ch + c0;
        const uint8_t* P = a.pat + p0;
        int err = 0;
        bool mismatch = false;
        u64 got = 0, di = 0, T = 0;
        for (u64 sym = s; sym < a.n && got < L; sym++, T++) {
            u64 sid = a.ent_off[sym], from = 0;
            if (a.size[sym] > 1) {
                if (di >= nc) { err = -2; break; }                 // too few choices
                const int64_t x = ch[di];
                if (x < 0) { err = -2; break; }
                if ((u64)x >= a.D) { err = -1; break; }
                const u64 d0 = a.cd[sym];
                if ((u64)x < d0 || (u64)x >= a.cd[sym + 1]) { err = -2; break; }   // a string of another symbol
                sid += (u64)x - d0;
                di++;
            } else if (sym == s) {
                from = offset;
            }
            const u64 s0 = a.str_off[sid] + from, len = a.str_off[sid + 1] - s0;
            const u64 take = min(len, L - got);
            for (u64 j = 0; j < take && !mismatch; j++) mismatch = a.chars[s0 + j] != P[got + j];
            got += take;
        }
        if (a.bits) {
            // first step after which the intersection is empty
            const u64 E = first_empty_step(a.bits, a.W, T, [&](u64 t, u64& d) {
                const u64 sym = s + t;
                u64 sid = a.ent_off[sym];
                if (a.size[sym] > 1) sid += (u64)ch[d++] - a.cd[sym];
                return sid;
            });
            if (E != NONE && E < T) { a.status[q] = 0; continue; }
        }
        if (err) { a.status[q] = (int8_t)err; continue; }
        a.status[q] = (got == L && !mismatch) ? 1 : 0;
    }
}

} // namespace

// Tokenise (DeviceEds::load) and scan the two position tables; returns n.
u64 QueryPipeline::tables(DeviceEds& de, const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, hipStream_t st)
{
    const auto t0 = std::chrono::steady_clock::now();
    de.load(eds, eds_n, seds, seds_n, seds != nullptr, st);
    info_.tokenise_ms = since_ms(t0);
    n_ = de.n(); C_ = D_ = 0;
    info_.n_symbols = n_; info_.n_strings = de.m();
    if (n_ == 0) return 0;
    const EdsView v = de.view();
    info_.n_chars = v.n_chars;
    cum_common_.ensure(8 * (n_ + 1));
    cum_deg_.ensure(8 * (n_ + 1));
    ctl_.ensure(8 * 8);
    scan_tmp_.ensure(8 * 2 * (n_ / SCAN_TILE + 4));
    u64 hn = n_;
    EDSX_HIP(hipMemcpyAsync(ctl_.ptr, &hn, 8, hipMemcpyHostToDevice, st));
    u64 *cc = cum_common_.as<u64>(), *cd = cum_deg_.as<u64>();
    TimedRuns timed(st, nullptr);
    timed.run("tables", [&] {
        hipLaunchKernelGGL(k_q_flags, dim3(grid_for(n_, 4096)), dim3(256), 0, st, v.sym.size, v.sym.len1, n_, cc, cd);
        ScanSet<2> ss{{cc, cd}, {cc, cd}, {cc + n_, cd + n_}};
        exclusive_scan_multi<2>(ss, ctl_.as<u64>(), scan_tmp_.as<u64>(), st);
    }, &info_.tables_ms);
    u64 h[2] = {0, 0};
    EDSX_HIP(hipMemcpyAsync(&h[0], cc + n_, 8, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipMemcpyAsync(&h[1], cd + n_, 8, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    timed.harvest();
    C_ = h[0]; D_ = h[1];
    info_.num_common_chars = C_; info_.num_degenerate_strings = D_;
    return n_;
}

void QueryPipeline::genpatterns(DeviceEds& de, const uint8_t* eds, size_t eds_n, u64 count, u32 pattern_length, u64 seed,
                                HostBytes& out, std::vector<u64>* wpos, std::vector<u64>* woff, std::vector<int32_t>* wdeg,
                                hipStream_t st)
{
    info_ = QueryInfo{};
    const u64 n = tables(de, eds, eds_n, nullptr, 0, st);
    if (n == 0) throw ParamError("Cannot generate patterns from empty EDS");          // eds.cpp:674-680
    if (pattern_length == 0) throw ParamError("Pattern length must be greater than 0");
    const u64 rec = (u64)pattern_length + 1;
    if (count > (~0ull >> 1) / rec) throw ParamError("Pattern count too large: " + std::to_string(count));
    const bool witness = wpos != nullptr;
    if (witness) { wpos->assign(count, NONE); woff->assign(1, 0); wdeg->clear(); }
    out.take(count * rec);
    if (count == 0) return;
    const u64 chunk = std::min<u64>(CHUNK_PATTERNS, std::max<u64>(1, CHUNK_BYTES / rec));
    out_.ensure(chunk * rec);
    if (witness) { wpos_.ensure(8 * chunk); wcnt_.ensure(8 * chunk); woff_.ensure(8 * (chunk + 1)); }
    scan_tmp_.ensure(8 * (chunk / SCAN_TILE + 4));
    ctl_.ensure(8 * 8);
    u64* ctl = ctl_.as<u64>();                                  // [0] err  [1] chunk size (scan length)
    const EdsView v = de.view();
    SampleArgs a{v.sym.size, v.sym.ent_off, v.str_off, v.chars, cum_common_.as<u64>(), cum_deg_.as<u64>(), n, C_, seed, 0, 0, pattern_length, out_.as<uint8_t>(),
                 witness ? wpos_.as<u64>() : nullptr, witness ? wcnt_.as<u64>() : nullptr, woff_.as<u64>(), nullptr, ctl};
    TimedRuns timed(st, nullptr);
    std::vector<u64> hoff;
    for (u64 i0 = 0; i0 < count; i0 += chunk) {
        const u64 cnt = std::min(chunk, count - i0);
        a.i0 = i0; a.cnt = cnt;
        u64 hctl[2] = {NONE, cnt};
        EDSX_HIP(hipMemcpyAsync(ctl, hctl, sizeof(hctl), hipMemcpyHostToDevice, st));
        timed.run("sample", [&] { hipLaunchKernelGGL(k_pat_sample<false>, dim3(grid_for(cnt, 4096)), dim3(256), 0, st, a); }, &info_.kernel_ms);
        u64 err = NONE, total = 0;
        EDSX_HIP(hipMemcpyAsync(&err, ctl, 8, hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        EDSX_HIP(hipGetLastError());
        timed.harvest();
        if (err != NONE) {
            const u64 t = err >> 40, w = err & ((1ull << 40) - 1);
            throw ParamError("Cannot generate pattern " + std::to_string(i0 + t) + ": the wrap-around reaches symbol " +
                             std::to_string(w) + ", which has no non-empty string");
        }
        if (witness) {                                           // CSR of the choices: count, scan, fill
            exclusive_scan_u64(wcnt_.as<u64>(), woff_.as<u64>(), ctl + 1, woff_.as<u64>() + cnt, scan_tmp_.as<u64>(), st);
            EDSX_HIP(hipMemcpyAsync(&total, woff_.as<u64>() + cnt, 8, hipMemcpyDeviceToHost, st));
            EDSX_HIP(hipStreamSynchronize(st));
            wdeg_.ensure(4 * std::max<u64>(total, 1));
            a.wdeg = wdeg_.as<int32_t>();
            timed.run("witness", [&] { hipLaunchKernelGGL(k_pat_sample<true>, dim3(grid_for(cnt, 4096)), dim3(256), 0, st, a); }, &info_.kernel_ms);
            EDSX_HIP(hipStreamSynchronize(st));
            EDSX_HIP(hipGetLastError());
            timed.harvest();
        }
        const auto t0 = std::chrono::steady_clock::now();
        PinnedDownload::copy(out.data + i0 * rec, out_.ptr, cnt * rec, st);
        if (witness) {
            EDSX_HIP(hipMemcpyAsync(wpos->data() + i0, wpos_.ptr, 8 * cnt, hipMemcpyDeviceToHost, st));
            hoff.resize(cnt + 1);
            EDSX_HIP(hipMemcpyAsync(hoff.data(), woff_.ptr, 8 * (cnt + 1), hipMemcpyDeviceToHost, st));
            const size_t d0 = wdeg->size();
            wdeg->resize(d0 + total);
            if (total) EDSX_HIP(hipMemcpyAsync(wdeg->data() + d0, wdeg_.ptr, 4 * total, hipMemcpyDeviceToHost, st));
            EDSX_HIP(hipStreamSynchronize(st));
            for (u64 t = 1; t <= cnt; t++) woff->push_back(d0 + hoff[t]);
        }
        info_.download_ms += since_ms(t0);
    }
}

void QueryPipeline::check(DeviceEds& de, const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, size_t nq,
                          const u64* pos, const u64* choice_off, const int32_t* choices, const u64* pattern_off,
                          const uint8_t* patterns, int8_t* status, hipStream_t st)
{
    info_ = QueryInfo{};
    const u64 n = tables(de, eds, eds_n, seds, seds_n, st);
    if (nq == 0) return;
    if (n == 0) { std::memset(status, 0, nq); return; }         // an empty EDS answers false first (:957)
    const u64 nch = choice_off[nq], npat = pattern_off[nq];
    q_pos_.ensure(8 * nq); q_coff_.ensure(8 * (nq + 1)); q_poff_.ensure(8 * (nq + 1)); q_status_.ensure(nq);
    q_ch_.ensure(4 * std::max<u64>(nch, 1)); q_pat_.ensure(std::max<u64>(npat, 1));
    EDSX_HIP(hipMemcpyAsync(q_pos_.ptr, pos, 8 * nq, hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemcpyAsync(q_coff_.ptr, choice_off, 8 * (nq + 1), hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemcpyAsync(q_poff_.ptr, pattern_off, 8 * (nq + 1), hipMemcpyHostToDevice, st));
    if (nch) EDSX_HIP(hipMemcpyAsync(q_ch_.ptr, choices, 4 * nch, hipMemcpyHostToDevice, st));
    if (npat) EDSX_HIP(hipMemcpyAsync(q_pat_.ptr, patterns, npat, hipMemcpyHostToDevice, st));
    const EdsView v = de.view();
    CheckArgs a{v.sym.size, v.sym.ent_off, v.str_off, v.chars, v.bits, v.W, cum_common_.as<u64>(), cum_deg_.as<u64>(), n, C_, D_,
                nq, q_pos_.as<u64>(), q_coff_.as<u64>(), q_ch_.as<int32_t>(), nch, q_poff_.as<u64>(), q_pat_.as<uint8_t>(), npat,
                q_status_.as<int8_t>()};
    TimedRuns timed(st, nullptr);
    timed.run("k_pat_check", [&] { hipLaunchKernelGGL(k_pat_check, dim3(grid_for(nq, 4096)), dim3(256), 0, st, a); }, &info_.kernel_ms);
    EDSX_HIP(hipMemcpyAsync(status, q_status_.ptr, nq, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    timed.harvest();
}

} // namespace edsx
