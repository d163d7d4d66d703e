// eds_device.hip — an .eds (+ .seds) text tokenised into HBM on gfx950: DeviceEds (the arrays every EDS consumer
// reads) and the statistics over them.
//
// Replaces EDS::parse / normalize / parse_sources (src/cpp/lib/formats/eds.cpp:39-155, :831-881, :268-355) and
// calculate_statistics / calculate_source_statistics / is_leds (eds.cpp:361-505, eds_transforms.cpp:439-468).
//
// Data layout in HBM
//   chars/str_off     all strings back to back (device tokeniser k_tok_*, host tokenisers for odd text)
//   symbols           size[i], ent_off[i] (first string), len1[i] (length of the only string when size == 1)
//   strings           elen[s] (length) and, with sources, bits[s * W ..] (its path set, bit 0 = the universal path "0")
// The l-EDS merge (merge_device.hip) takes these over through DeviceEds::consume and appends to elen / bits; every other
// consumer reads them through DeviceEds::view.
#include "eds_device.hpp"

#include <thread>

#include <algorithm>
#include <cctype>
#include <cstring>

namespace edsx {

// ---- device tokenisers ------------------------------------------------------------------------------
// The .eds / .seds text goes to HBM as it is and is tokenised there (eds.cpp:39-155 / :268-355 rules) straight into
// the layout above: no host arrays, no per-array upload.  The kernels only accept text every byte of which they can
// place (no whitespace before the end, braces alternate, no comma outside braces, ids are digits that fit an int,
// no empty source set); anything else raises `bad`, and the host tokenisers - which own the reference's error texts
// and its treatment of odd but legal text - take the input instead.
// Two passes over 4 KB blocks of the text (256 threads x 16 bytes), nothing kept per byte:
//   count   per block: '{', '}', ',' (ids for .seds), starts of bare runs, characters - what a byte IS needs only
//           the byte in front of it
//   scan    of the block counts (three packed u64 arrays, one multi-array pass)
//   fill    the same classification again; block prefix + a scan inside the workgroup give every byte its place in
//           chars / str_off / sym_first (its source set), and the brace depth in front of it - which is where the
//           text is validated: a byte that does not fit its depth raises `bad` (the arrays are sized by the counts
//           either way, so a text that is rejected writes inside them)
struct TokCtl { u64 n, bad, nblk, totA, totB, totC, maxid, pad; };
constexpr u32 TOK_BLOCK = 4096;

__device__ __forceinline__ bool tok_ws(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }
__device__ __forceinline__ bool tok_digit(uint8_t c) { return c >= '0' && c <= '9'; }

struct TokSums { u64 a, b, c; };
// exclusive prefix of `mine` over the 256 threads of the workgroup; `total` = sum over all of them
__device__ __forceinline__ TokSums tok_block_scan(const TokSums& mine, TokSums* wsum, TokSums& total)
{
    TokSums inc = mine;
    const u32 lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const u64 ta = __shfl_up(inc.a, o, 64), tb = __shfl_up(inc.b, o, 64), tc = __shfl_up(inc.c, o, 64);
        if (lane >= (u32)o) { inc.a += ta; inc.b += tb; inc.c += tc; }
    }
    __syncthreads();                                          // (wsum of the previous block has been read)
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    TokSums ex{inc.a - mine.a, inc.b - mine.b, inc.c - mine.c};
    total = TokSums{0, 0, 0};
    for (u32 w = 0; w < 4; w++) {
        const TokSums t = wsum[w];
        if (w < wv) { ex.a += t.a; ex.b += t.b; ex.c += t.c; }
        total.a += t.a; total.b += t.b; total.c += t.c;
    }
    return ex;
}
// the 16 bytes of this thread (nb of them exist) and the byte in front of them (0: start of the text)
__device__ __forceinline__ void tok_load(const uint8_t* raw, u64 n, u64 i0, uint8_t (&c)[16], int& nb, uint8_t& prev)
{
    nb = i0 < n ? (n - i0 < 16 ? (int)(n - i0) : 16) : 0;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (nb > 0) v = *reinterpret_cast<const uint4*>(raw + i0);       // (the buffer has 16 bytes of slack behind the text)
    __builtin_memcpy(c, &v, 16);
    prev = (nb > 0 && i0 > 0) ? raw[i0 - 1] : 0;
}

// .eds.  A = '{' | '}' << 32, B = ',' | bare-run starts << 32, C = characters.  Strings open at '{', ',' and at the
// first character of a bare run (eds.cpp:848-878: text outside braces is a symbol of one string), symbols at '{' and there.
template <bool FILL>
__global__ void __launch_bounds__(256) k_tok_eds(const uint8_t* __restrict__ raw, u64 n, u64* __restrict__ A, u64* __restrict__ B,
                                                 u64* __restrict__ C, uint8_t* __restrict__ chars, u64* __restrict__ str_off,
                                                 u64* __restrict__ sym_first, TokCtl* ctl)
{
    __shared__ TokSums wsum[4];
    const u64 nblk = (n + TOK_BLOCK - 1) / TOK_BLOCK;
    bool bad = false;
    for (u64 blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const u64 i0 = blk * TOK_BLOCK + (u64)threadIdx.x * 16;
        uint8_t c[16], prev;
        int nb;
        tok_load(raw, n, i0, c, nb, prev);
        TokSums mine{0, 0, 0};
        uint8_t pv = prev;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            if (k < nb) {
                const uint8_t ch = c[k];
                if (ch == '{') mine.a += 1;
                else if (ch == '}') mine.a += 1ull << 32;
                else if (ch == ',') mine.b += 1;
                else {
                    mine.c += 1;
                    if (i0 + k == 0 || pv == '}') mine.b += 1ull << 32;
                    if (!FILL && tok_ws(ch)) bad = true;
                }
                pv = ch;
            }
        }
        TokSums total;
        TokSums ex = tok_block_scan(mine, wsum, total);
        if constexpr (!FILL) {
            if (threadIdx.x == 0) { A[blk] = total.a; B[blk] = total.b; C[blk] = total.c; }
        } else {
            ex.a += A[blk]; ex.b += B[blk]; ex.c += C[blk];
            u64 o = ex.a & 0xffffffffull, cl = ex.a >> 32, cm = ex.b & 0xffffffffull, br = ex.b >> 32, h = ex.c;
            pv = prev;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                if (k < nb) {
                    const uint8_t ch = c[k];
                    const u64 depth = o - cl;                            // braces open in front of this byte
                    const u64 sidx = o + cm + br;
                    if (ch == '{') { if (depth != 0) bad = true; str_off[sidx] = h; sym_first[o + br] = sidx; o++; }
                    else if (ch == '}') { if (depth != 1) bad = true; cl++; }
                    else if (ch == ',') { if (depth != 1) bad = true; str_off[sidx] = h; cm++; }
                    else {
                        if (depth > 1) bad = true;
                        if (i0 + k == 0 || pv == '}') { str_off[sidx] = h; sym_first[o + br] = sidx; br++; }
                        chars[h] = ch; h++;
                    }
                    pv = ch;
                }
            }
        }
    }
    if (bad) ctl->bad = 1;
    if (FILL && blockIdx.x == 0 && threadIdx.x == 0) {
        const u64 o = ctl->totA & 0xffffffffull, cl = ctl->totA >> 32, cm = ctl->totB & 0xffffffffull, br = ctl->totB >> 32;
        if (o != cl) ctl->bad = 1;                                       // unterminated group
        str_off[o + cm + br] = ctl->totC;
        sym_first[o + br] = o + cm + br;
    }
}

// per-string lengths; the leaf links of the merge's entry pool are k_leaf_links (merge_device.hip)
__global__ void k_tok_lengths(const u64* __restrict__ str_off, u64 m, u32* __restrict__ elen)
{
    for (u64 s = blockIdx.x * (u64)blockDim.x + threadIdx.x; s < m; s += (u64)gridDim.x * blockDim.x)
        elen[s] = (u32)(str_off[s + 1] - str_off[s]);
}

__global__ void k_tok_syms(const u64* __restrict__ sym_first, const u64* __restrict__ str_off, u64 n0, SymArrays s)
{
    for (u64 k = blockIdx.x * (u64)blockDim.x + threadIdx.x; k < n0; k += (u64)gridDim.x * blockDim.x) {
        const u64 f = sym_first[k], sz = sym_first[k + 1] - f;
        s.size[k] = sz; s.ent_off[k] = f; s.len1[k] = sz == 1 ? str_off[f + 1] - str_off[f] : 0;
    }
}

// .seds: an id is a maximal run of digits; value -> ok?  (std::stoi range, eds.cpp:336-349)
__device__ __forceinline__ bool tok_number(const uint8_t* raw, u64 i, u64 n, u64& val)
{
    val = 0;
    u64 j = i;
    for (; j < n && raw[j] >= '0' && raw[j] <= '9'; j++) {
        val = val * 10 + (raw[j] - '0');
        if (val > 2147483647ull) return false;
    }
    return true;
}

// .seds.  A = '{' | '}' << 32, B = ids (an id starts at a digit that does not follow a digit).  COUNT also finds the
// largest id (the width of the path bitsets); FILL validates and sets bit `id` of the byte's source set.
template <bool FILL>
__global__ void __launch_bounds__(256) k_tok_seds(const uint8_t* __restrict__ raw, u64 n, u64* __restrict__ A, u64* __restrict__ B,
                                                  u64* __restrict__ C, u64* __restrict__ bits, u32 W, TokCtl* ctl)
{
    __shared__ TokSums wsum[4];
    const u64 nblk = (n + TOK_BLOCK - 1) / TOK_BLOCK;
    bool bad = false;
    u64 mx = 0;
    for (u64 blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const u64 i0 = blk * TOK_BLOCK + (u64)threadIdx.x * 16;
        uint8_t c[16], prev;
        int nb;
        tok_load(raw, n, i0, c, nb, prev);
        TokSums mine{0, 0, 0};
        uint8_t pv = prev;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            if (k < nb) {
                const uint8_t ch = c[k];
                if (ch == '{') mine.a += 1;
                else if (ch == '}') mine.a += 1ull << 32;
                else if (tok_digit(ch)) {
                    if (!tok_digit(pv)) {
                        mine.b += 1;
                        if (!FILL) { u64 v; if (!tok_number(raw, i0 + k, n, v)) bad = true; mx = v > mx ? v : mx; }
                    }
                } else if (ch != ',') bad = true;
                pv = ch;
            }
        }
        TokSums total;
        TokSums ex = tok_block_scan(mine, wsum, total);
        if constexpr (!FILL) {
            if (threadIdx.x == 0) { A[blk] = total.a; B[blk] = total.b; C[blk] = 0; }
        } else {
            ex.a += A[blk];
            u64 o = ex.a & 0xffffffffull, cl = ex.a >> 32;
            pv = prev;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                if (k < nb) {
                    const uint8_t ch = c[k];
                    const u64 depth = o - cl;
                    if (ch == '{') { if (depth != 0) bad = true; o++; }
                    else {
                        if (depth != 1) bad = true;
                        if (ch == '}') {
                            u64 q = i0 + k;                              // a set of commas only is empty (eds.cpp:330)
                            while (q > 0 && raw[q - 1] == ',') q--;
                            if (q == 0 || raw[q - 1] == '{') bad = true;
                            cl++;
                        } else if (tok_digit(ch) && !tok_digit(pv) && depth == 1) {
                            u64 v;
                            tok_number(raw, i0 + k, n, v);
                            atomicOr((unsigned long long*)&bits[(o - 1) * W + (v >> 6)], 1ull << (v & 63));
                        }
                    }
                    pv = ch;
                }
            }
        }
    }
    if (bad) ctl->bad = 1;
    if (!FILL && mx) atomicMax((unsigned long long*)&ctl->maxid, (unsigned long long)mx);
    if (FILL && blockIdx.x == 0 && threadIdx.x == 0 && (ctl->totA & 0xffffffffull) != (ctl->totA >> 32)) ctl->bad = 1;
}

// ---- host ---------------------------------------------------------------------------------------
namespace {

std::string strip_ws(const uint8_t* p, size_t n)
{
    std::string s;
    s.reserve(n);
    for (size_t i = 0; i < n; i++) if (!std::isspace(p[i])) s.push_back((char)p[i]);
    return s;
}

std::string normalize(const std::string& in)                 // eds.cpp:831-881
{
    std::string out, run;
    out.reserve(in.size() + 16);
    int depth = 0;
    for (char ch : in) {
        if (ch == '{') {
            if (!run.empty() && depth == 0) { out += '{'; out += run; out += '}'; run.clear(); }
            out += ch; depth++;
        } else if (ch == '}') { out += ch; depth--; }
        else if (depth > 0) out += ch;
        else run += ch;
    }
    if (!run.empty() && depth == 0) { out += '{'; out += run; out += '}'; }
    return out;
}

// ---- chunk-parallel host tokenisers ---------------------------------------------------------------
// .eds / .seds text is a sequence of brace groups that do not nest, so a cut right behind any '}' is a
// point where the sequential tokenisers below are in their initial state.  Large inputs are cut there and
// tokenised by several host threads into flat arrays.  The fast path only accepts well-formed text;
// anything else (nesting, a stray brace, a character that does not belong, an empty source set, a number
// beyond int) makes it give up, and the sequential code then produces the reference's error text.
unsigned tokenizer_threads(size_t n)
{
    static long par_min = -1;
    if (par_min < 0) { const char* e = getenv("EDSX_TOKENIZE_PAR_MIN"); par_min = e ? atol(e) : (1l << 20); }
    if ((long)n < par_min) return 1;
    const unsigned hc = std::thread::hardware_concurrency();
    return std::max(1u, std::min(16u, hc ? hc : 4u));
}
std::vector<size_t> brace_cuts(const uint8_t* p, size_t n, unsigned nt)
{
    std::vector<size_t> cut(nt + 1, n);
    cut[0] = 0;
    for (unsigned t = 1; t < nt; t++) {
        size_t g = (size_t)((unsigned __int128)n * t / nt);
        if (g < cut[t - 1]) g = cut[t - 1];
        const uint8_t* b = g < n ? static_cast<const uint8_t*>(memchr(p + g, '}', n - g)) : nullptr;
        cut[t] = b ? static_cast<size_t>(b - p) + 1 : n;
    }
    return cut;
}
struct EdsPart { std::vector<uint8_t> chars; std::vector<u64> str_end; std::vector<u64> sym_nstr; bool ok = true; };
void tokenize_eds_range(const uint8_t* p, size_t lo, size_t hi, EdsPart& out)
{
    out.chars.reserve(hi - lo);
    int depth = 0;
    bool run_open = false;                                   // a bare run (text outside braces) is being collected
    u64 nstr = 0;
    auto close_symbol = [&] { out.str_end.push_back(out.chars.size()); out.sym_nstr.push_back(nstr + 1); nstr = 0; };
    for (size_t i = lo; i < hi; i++) {
        const uint8_t ch = p[i];
        if (std::isspace(ch)) continue;
        if (ch == '{') {
            if (depth) { out.ok = false; return; }           // nesting
            if (run_open) { close_symbol(); run_open = false; }
            depth = 1;
        } else if (ch == '}') {
            if (!depth) { out.ok = false; return; }          // stray brace
            close_symbol();
            depth = 0;
        } else if (ch == ',') { out.str_end.push_back(out.chars.size()); nstr++; if (!depth) run_open = true; }
        else { out.chars.push_back(ch); if (!depth) run_open = true; }
    }
    if (depth) { out.ok = false; return; }                   // unterminated group
    if (run_open) close_symbol();
}
// fills chars / str_off / sym_first like the sequential tokeniser; false: not well-formed, use that one
bool tokenize_eds_parallel(const uint8_t* p, size_t n, std::vector<uint8_t>& chars, std::vector<u64>& str_off,
                           std::vector<u64>& sym_first)
{
    const unsigned nt = tokenizer_threads(n);
    if (nt < 2) return false;
    const std::vector<size_t> cut = brace_cuts(p, n, nt);
    std::vector<EdsPart> parts(nt);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++) th.emplace_back([&, t] { tokenize_eds_range(p, cut[t], cut[t + 1], parts[t]); });
    for (auto& x : th) x.join();
    size_t nc = 0, ns = 0, ny = 0;
    for (const auto& pt : parts) { if (!pt.ok) return false; nc += pt.chars.size(); ns += pt.str_end.size(); ny += pt.sym_nstr.size(); }
    chars.resize(nc); str_off.assign(ns + 1, 0); sym_first.assign(ny + 1, 0);
    std::vector<size_t> c0(nt + 1, 0), s0(nt + 1, 0), y0(nt + 1, 0);
    for (unsigned t = 0; t < nt; t++) {
        c0[t + 1] = c0[t] + parts[t].chars.size(); s0[t + 1] = s0[t] + parts[t].str_end.size(); y0[t + 1] = y0[t] + parts[t].sym_nstr.size();
    }
    th.clear();
    for (unsigned t = 0; t < nt; t++)
        th.emplace_back([&, t] {
            const EdsPart& pt = parts[t];
            if (!pt.chars.empty()) memcpy(chars.data() + c0[t], pt.chars.data(), pt.chars.size());
            for (size_t i = 0; i < pt.str_end.size(); i++) str_off[s0[t] + i + 1] = c0[t] + pt.str_end[i];
            u64 first = s0[t];
            for (size_t i = 0; i < pt.sym_nstr.size(); i++) { first += pt.sym_nstr[i]; sym_first[y0[t] + i + 1] = first; }
        });
    for (auto& x : th) x.join();
    return true;
}
struct SedsPart { std::vector<int> ids; std::vector<u64> set_end; int maxid = 0; bool ok = true; };
void tokenize_seds_range(const uint8_t* p, size_t lo, size_t hi, SedsPart& out)
{
    int depth = 0;
    bool have = false;
    long long val = 0;
    size_t set_begin = 0;
    auto flush = [&] { if (have) { out.ids.push_back((int)val); out.maxid = std::max(out.maxid, (int)val); } have = false; val = 0; };
    for (size_t i = lo; i < hi; i++) {
        const uint8_t ch = p[i];
        if (std::isspace(ch)) continue;
        if (!depth) {
            if (ch != '{') { out.ok = false; return; }
            depth = 1; set_begin = out.ids.size();
        } else if (ch == '}') {
            flush();
            if (out.ids.size() == set_begin) { out.ok = false; return; }      // empty path set
            out.set_end.push_back(out.ids.size());
            depth = 0;
        } else if (ch == ',') flush();
        else if (ch >= '0' && ch <= '9') {
            val = val * 10 + (ch - '0'); have = true;
            if (val > 2147483647ll) { out.ok = false; return; }               // std::stoi would throw
        } else { out.ok = false; return; }
    }
    if (depth) out.ok = false;
}
bool tokenize_seds_parallel(const uint8_t* p, size_t n, std::vector<SedsPart>& parts, u64& nsets, int& maxid)
{
    const unsigned nt = tokenizer_threads(n);
    if (nt < 2) return false;
    const std::vector<size_t> cut = brace_cuts(p, n, nt);
    parts.assign(nt, SedsPart());
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++) th.emplace_back([&, t] { tokenize_seds_range(p, cut[t], cut[t + 1], parts[t]); });
    for (auto& x : th) x.join();
    nsets = 0; maxid = 0;
    for (const auto& pt : parts) { if (!pt.ok) return false; nsets += pt.set_end.size(); maxid = std::max(maxid, pt.maxid); }
    return nsets > 0;
}

} // namespace

void StageTrace::mark(const char* what)
{
    static const bool trace = [] { const char* e = getenv("EDSX_TRACE"); return e && atoi(e); }();
    if (!trace) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[edsx merge] %-26s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - last_).count());
    last_ = now;
}

// elen (and bits) for the m strings, or for the merge's entry pool
void DeviceEds::ensure_strings(bool merge_headroom, bool linear)
{
    const size_t cap = merge_headroom ? std::max<size_t>(2 * m_ + 1024, 4096) : m_;
    elen_.ensure(4 * cap);
    if (linear) bits_.ensure(8 * cap * W_);
}

// Tokenise on the device (kernels above).  false: the text is not plain, or there is none; load() then runs the host
// tokenisers.  On success chars / str_off / the string lengths / the symbol arrays / the source bitsets are in place.
bool DeviceEds::load_device(const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, bool linear, bool merge_headroom,
                            hipStream_t st)
{
    { const char* e = getenv("EDSX_HOST_TOKENIZER"); if (e && atoi(e)) return false; }      // A/B switch for the parity tests
    size_t end = eds_n, send = linear ? seds_n : 0;
    while (end && std::isspace(eds[end - 1])) end--;
    while (send && std::isspace(seds[send - 1])) send--;
    if (end == 0 || end >= 0xfffffff0ull || (linear && (send == 0 || send >= 0xfffffff0ull))) return false;
    const size_t nmax = std::max(end, send);
    if (!device_scratch_fits(nmax + nmax / 64)) return false;   // the raw text + three counters per 4 KB block
    const u64 nblk_max = (nmax + TOK_BLOCK - 1) / TOK_BLOCK;
    raw_.ensure(nmax + 16);
    for (DevBuf* b : {&tk_a_, &tk_b_, &tk_c_}) b->ensure(8 * (nblk_max + 2));
    scan_tmp_.ensure(8 * 3 * (nblk_max / SCAN_TILE + 4));
    TokCtl* ctl = ctl_.as<TokCtl>();
    TokCtl h{};
    h.n = end; h.nblk = (end + TOK_BLOCK - 1) / TOK_BLOCK;
    EDSX_HIP(hipMemcpyAsync(ctl, &h, sizeof(h), hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemcpyAsync(raw_.ptr, eds, end, hipMemcpyHostToDevice, st));
    const uint8_t* raw = raw_.as<uint8_t>();
    u64 *a = tk_a_.as<u64>(), *b = tk_b_.as<u64>(), *c = tk_c_.as<u64>();
    const unsigned grid = (unsigned)std::min<u64>(h.nblk, 8192);
    hipLaunchKernelGGL(k_tok_eds<false>, dim3(grid), dim3(256), 0, st, raw, (u64)end, a, b, c, (uint8_t*)nullptr, (u64*)nullptr,
                       (u64*)nullptr, ctl);
    {
        ScanSet<3> ss{{a, b, c}, {a, b, c}, {&ctl->totA, &ctl->totB, &ctl->totC}};
        exclusive_scan_multi<3>(ss, &ctl->nblk, scan_tmp_.as<u64>(), st);
    }
    EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    if (h.bad) return false;
    const u64 opens = h.totA & 0xffffffffull, commas = h.totB & 0xffffffffull, bare = h.totB >> 32;
    const u64 nchars = h.totC;
    const u64 m = opens + commas + bare, n0 = opens + bare;
    if (n0 == 0 || m == 0 || m >= 0xfffffff0ull) return false;
    n_ = n0; m_ = m;
    chars_.ensure(nchars + 16);
    str_off_.ensure(8 * (m + 1));
    sym_first_.ensure(8 * (n0 + 1));
    hipLaunchKernelGGL(k_tok_eds<true>, dim3(grid), dim3(256), 0, st, raw, (u64)end, a, b, c, chars_.as<uint8_t>(),
                       str_off_.as<u64>(), sym_first_.as<u64>(), ctl);
    ensure_strings(merge_headroom, false);
    hipLaunchKernelGGL(k_tok_lengths, dim3(2048), dim3(256), 0, st, str_off_.as<u64>(), m, elen_.as<u32>());
    for (DevBuf* buf : {&size_, &ent_off_, &len1_}) buf->ensure(8 * (n0 + 1));
    hipLaunchKernelGGL(k_tok_syms, dim3(2048), dim3(256), 0, st, sym_first_.as<u64>(), str_off_.as<u64>(), n0, sym());
    u64 sf_head[2] = {0, 0}, sf_tail[2] = {0, 0}, so_head[2] = {0, 0};
    EDSX_HIP(hipMemcpyAsync(sf_head, sym_first_.as<u64>(), 16, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipMemcpyAsync(sf_tail, sym_first_.as<u64>() + (n0 - 1), 16, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipMemcpyAsync(so_head, str_off_.as<u64>(), 16, hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));     // `bad` of the fill pass (brace depth)
    EDSX_HIP(hipStreamSynchronize(st));
    if (h.bad) return false;
    if (linear) {
        h = TokCtl{};
        h.n = send; h.nblk = (send + TOK_BLOCK - 1) / TOK_BLOCK;
        EDSX_HIP(hipMemcpyAsync(ctl, &h, sizeof(h), hipMemcpyHostToDevice, st));
        EDSX_HIP(hipMemcpyAsync(raw_.ptr, seds, send, hipMemcpyHostToDevice, st));
        const unsigned sgrid = (unsigned)std::min<u64>(h.nblk, 8192);
        hipLaunchKernelGGL(k_tok_seds<false>, dim3(sgrid), dim3(256), 0, st, raw, (u64)send, a, b, c, (u64*)nullptr, 0u, ctl);
        {
            ScanSet<3> ss{{a, b, c}, {a, b, c}, {&ctl->totA, &ctl->totB, &ctl->totC}};
            exclusive_scan_multi<3>(ss, &ctl->nblk, scan_tmp_.as<u64>(), st);
        }
        EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        if (h.bad || (h.totA & 0xffffffffull) != m) return false;   // the host path words the error
        const u32 W = W_ = (u32)(h.maxid / 64 + 1);
        ensure_strings(merge_headroom, true);
        EDSX_HIP(hipMemsetAsync(bits_.ptr, 0, 8 * (size_t)m * W, st));
        hipLaunchKernelGGL(k_tok_seds<true>, dim3(sgrid), dim3(256), 0, st, raw, (u64)send, a, b, c, bits_.as<u64>(), W, ctl);
        EDSX_HIP(hipMemcpyAsync(&h, ctl, sizeof(h), hipMemcpyDeviceToHost, st));
        EDSX_HIP(hipStreamSynchronize(st));
        if (h.bad) return false;
    }
    EDSX_HIP(hipGetLastError());
    head_single_ = sf_head[1] - sf_head[0] == 1;
    tail_single_ = sf_tail[1] - sf_tail[0] == 1;
    head_len_ = so_head[1] - so_head[0];
    n_chars_ = nchars;
    return true;
}

// The host tokenisers (eds.cpp:39-155, same error texts) and the upload.
void DeviceEds::load_host(const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, bool linear, bool merge_headroom,
                      hipStream_t st)
{
    std::vector<uint8_t> chars;
    std::vector<u64> str_off{0}, sym_first{0};
    if (!tokenize_eds_parallel(eds, eds_n, chars, str_off, sym_first)) {
        chars.clear(); str_off.assign(1, 0); sym_first.assign(1, 0);
        std::string in = strip_ws(eds, eds_n);
        if (!in.empty()) {
            in = normalize(in);
            chars.reserve(in.size());
            size_t pos = 0;
            while (pos < in.size()) {
                if (in[pos] != '{') throw FormatError("Expected '{' at position " + std::to_string(pos));
                pos++;
                while (pos < in.size() && in[pos] != '}') {
                    if (in[pos] == ',') str_off.push_back(chars.size());
                    else chars.push_back((uint8_t)in[pos]);
                    pos++;
                }
                str_off.push_back(chars.size());
                if (pos >= in.size() || in[pos] != '}') throw FormatError("Expected '}' at position " + std::to_string(pos));
                pos++;
                sym_first.push_back(str_off.size() - 1);
            }
        }
    }
    const u64 n0 = sym_first.size() - 1, m = str_off.size() - 1;
    u32 W = 1;

    // ---- sources: eds.cpp:268-355 -> bitsets
    std::vector<u64> bits;
    std::vector<SedsPart> sparts;
    u64 par_sets = 0;
    int par_maxid = 0;
    if (linear && tokenize_seds_parallel(seds, seds_n, sparts, par_sets, par_maxid) && par_sets == m) {
        W = (u32)(par_maxid / 64 + 1);
        bits.assign((size_t)m * W, 0);
        std::vector<size_t> base(sparts.size() + 1, 0);
        for (size_t t = 0; t < sparts.size(); t++) base[t + 1] = base[t] + sparts[t].set_end.size();
        std::vector<std::thread> th;
        for (size_t t = 0; t < sparts.size(); t++)
            th.emplace_back([&, t] {
                const SedsPart& pt = sparts[t];
                size_t b = 0;
                for (size_t sidx = 0; sidx < pt.set_end.size(); sidx++) {
                    for (; b < pt.set_end[sidx]; b++) { const int id = pt.ids[b]; bits[(base[t] + sidx) * W + id / 64] |= 1ull << (id % 64); }
                }
            });
        for (auto& x : th) x.join();
    } else if (linear) {
        std::string in = strip_ws(seds, seds_n);
        if (in.empty()) throw FormatError("sEDS input is empty");
        std::vector<std::vector<int>> sets;
        int maxid = 0;
        size_t pos = 0;
        while (pos < in.size()) {
            if (in[pos] != '{') throw FormatError("sEDS: Expected '{' at position " + std::to_string(pos));
            pos++;
            std::vector<int> ids;
            std::string num;
            auto flush = [&] {
                if (num.empty()) return;
                int id;
                try { id = std::stoi(num); } catch (...) { throw FormatError("stoi"); }
                ids.push_back(id);
                maxid = std::max(maxid, id);
                num.clear();
            };
            while (pos < in.size() && in[pos] != '}') {
                if (in[pos] == ',') flush();
                else if (std::isdigit((unsigned char)in[pos])) num += in[pos];
                else
                    throw FormatError("sEDS: Invalid character '" + std::string(1, in[pos]) + "' at position " +
                                      std::to_string(pos));
                pos++;
            }
            flush();
            if (pos >= in.size() || in[pos] != '}') throw FormatError("sEDS: Expected '}' at position " + std::to_string(pos));
            pos++;
            if (ids.empty()) throw FormatError("sEDS: Empty path set at string " + std::to_string(sets.size()));
            sets.push_back(std::move(ids));
        }
        if (sets.size() != m)
            throw FormatError("sEDS: Source count (" + std::to_string(sets.size()) + ") does not match EDS cardinality (" +
                              std::to_string(m) + ")");
        W = (u32)(maxid / 64 + 1);
        bits.assign((size_t)m * W, 0);
        for (size_t sidx = 0; sidx < m; sidx++)
            for (int id : sets[sidx]) bits[sidx * W + id / 64] |= 1ull << (id % 64);
    }

    if (n0 == 0) return;                                     // empty EDS
    if (m >= 0xfffffff0ull) throw FormatError("EDS has too many strings for this build");
    n_ = n0; m_ = m; W_ = linear ? W : 0; n_chars_ = chars.size();
    head_single_ = sym_first[1] - sym_first[0] == 1; tail_single_ = sym_first[n0] - sym_first[n0 - 1] == 1;
    head_len_ = str_off[1] - str_off[0];

    // ---- upload
    chars_.ensure(chars.size() + 16);
    str_off_.ensure(8 * (m + 1));
    EDSX_HIP(hipMemcpyAsync(chars_.ptr, chars.data(), chars.size(), hipMemcpyHostToDevice, st));
    EDSX_HIP(hipMemcpyAsync(str_off_.ptr, str_off.data(), 8 * (m + 1), hipMemcpyHostToDevice, st));
    ensure_strings(merge_headroom, linear);
    hipLaunchKernelGGL(k_tok_lengths, dim3(2048), dim3(256), 0, st, str_off_.as<u64>(), m, elen_.as<u32>());
    if (linear) EDSX_HIP(hipMemcpyAsync(bits_.ptr, bits.data(), 8 * (size_t)m * W, hipMemcpyHostToDevice, st));
    sym_first_.ensure(8 * (n0 + 1));
    EDSX_HIP(hipMemcpyAsync(sym_first_.ptr, sym_first.data(), 8 * (n0 + 1), hipMemcpyHostToDevice, st));
    for (DevBuf* b : {&size_, &ent_off_, &len1_}) b->ensure(8 * (n0 + 1));
    hipLaunchKernelGGL(k_tok_syms, dim3(2048), dim3(256), 0, st, sym_first_.as<u64>(), str_off_.as<u64>(), n0, sym());
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
}

void DeviceEds::load(const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, bool linear, hipStream_t st,
                     bool merge_headroom)
{
    StageTrace trace;
    ctl_.ensure(sizeof(TokCtl));
    n_ = m_ = n_chars_ = head_len_ = 0; W_ = 0; head_single_ = tail_single_ = false; consumed_ = false;
    with_sources_ = linear;
    tokenised_on_device_ = load_device(eds, eds_n, seds, seds_n, linear, merge_headroom, st);
    trace.mark(tokenised_on_device_ ? "upload + device tokenise" : "device tokenise attempt");
    if (tokenised_on_device_) return;
    n_ = m_ = n_chars_ = head_len_ = 0; W_ = 0; head_single_ = tail_single_ = false;   // (a rejected attempt got this far)
    load_host(eds, eds_n, seds, seds_n, linear, merge_headroom, st);
    trace.mark("host tokenise + upload");
}

EdsView DeviceEds::view() const
{
    if (consumed_) throw DeviceError("DeviceEds::view: the merge has consumed this text; load it again");
    return EdsView{SymView{size_.as<u64>(), ent_off_.as<u64>(), len1_.as<u64>()}, str_off_.as<u64>(), chars_.as<uint8_t>(),
                   elen_.as<u32>(), W_ ? bits_.as<u64>() : nullptr, n_, m_, n_chars_, W_};
}

void DeviceEds::drop_scratch()
{
    for (DevBuf* b : {&raw_, &tk_a_, &tk_b_, &tk_c_, &sym_first_, &scan_tmp_}) b->release();
}

DeviceEds::Pool DeviceEds::consume()
{
    consumed_ = true;
    return Pool{elen_, bits_, sym(), str_off_.as<u64>(), chars_.as<uint8_t>()};
}

// ---- statistics and l-EDS validity as device reductions (eds.cpp:361-505, eds_transforms.cpp:439-468) -------------
// acc: [0] degenerate symbols [1] sum(size - 1) over them [2] characters of the non-degenerate symbols [3] their number
//      [4] min / [5] max of their lengths [6] "not an l-EDS" [7] empty strings [8] all characters [9] sum of the set
//      sizes [10] largest set; orbits[W]: OR of all path sets
__global__ void __launch_bounds__(256) k_eds_stats(SymView s, u64 n, const u32* __restrict__ elen, u64 m, const u64* __restrict__ bits,
                                                   u32 W, u64 l, u64* __restrict__ acc, u64* __restrict__ orbits)
{
    const u64 t0 = blockIdx.x * (u64)blockDim.x + threadIdx.x, step = (u64)gridDim.x * blockDim.x;
    u64 ndeg = 0, change = 0, common = 0, nctx = 0, mn = ~0ull, mx = 0, bad = 0;
    for (u64 i = t0; i < n; i += step) {
        const u64 sz = s.size[i];
        if (sz > 1) {
            ndeg++; change += sz - 1;
            if (i + 1 < n && s.size[i + 1] > 1) bad = 1;        // adjacent degenerate symbols (:462-464)
        } else {
            const u64 len = s.len1[i];
            common += len; nctx++;
            mn = len < mn ? len : mn; mx = len > mx ? len : mx;
            if (l && i > 0 && i + 1 < n && len < l) bad = 1;     // a short internal common block (:455-457)
        }
    }
    u64 empty = 0, chars = 0, tot = 0, big = 0;
    for (u64 k = t0; k < m; k += step) {
        const u64 e = elen[k];
        empty += e == 0; chars += e;
        if (bits) {
            u64 c = 0;
            for (u32 w = 0; w < W; w++) c += (u64)__builtin_popcountll(bits[k * W + w]);
            tot += c; big = c > big ? c : big;
        }
    }
    if (bits) {                                                   // OR of all sets, word by word
        for (u32 w = 0; w < W; w++) {
            u64 o = 0;
            for (u64 k = t0; k < m; k += step) o |= bits[k * W + w];
            for (int sh = 32; sh > 0; sh >>= 1) o |= __shfl_xor(o, sh, 64);
            if ((threadIdx.x & 63) == 0 && o) atomicOr(&orbits[w], o);
        }
    }
    ndeg = wave_sum(ndeg); change = wave_sum(change); common = wave_sum(common); nctx = wave_sum(nctx);
    empty = wave_sum(empty); chars = wave_sum(chars); tot = wave_sum(tot);
    for (int sh = 32; sh > 0; sh >>= 1) {
        const u64 a = __shfl_xor(mn, sh, 64), b = __shfl_xor(mx, sh, 64), c = __shfl_xor(big, sh, 64), d = __shfl_xor(bad, sh, 64);
        mn = a < mn ? a : mn; mx = b > mx ? b : mx; big = c > big ? c : big; bad |= d;
    }
    if ((threadIdx.x & 63) == 0) {
        if (ndeg) atomicAdd(&acc[0], ndeg);
        if (change) atomicAdd(&acc[1], change);
        if (common) atomicAdd(&acc[2], common);
        if (nctx) atomicAdd(&acc[3], nctx);
        atomicMin(&acc[4], mn); atomicMax(&acc[5], mx);
        if (bad) atomicOr(&acc[6], 1ull);
        if (empty) atomicAdd(&acc[7], empty);
        if (chars) atomicAdd(&acc[8], chars);
        if (tot) atomicAdd(&acc[9], tot);
        atomicMax(&acc[10], big);
    }
}

void eds_stats(const DeviceEds& de, uint32_t l, DevBuf& acc_buf, EdsStats& out, hipStream_t st)
{
    out = EdsStats{};
    out.has_sources = de.with_sources() ? 1 : 0;
    out.is_leds = 1;
    if (de.n() == 0) return;                                    // empty EDS: all zero (eds.cpp:362-376), trivially an l-EDS
    const EdsView v = de.view();
    acc_buf.ensure(8 * (16 + (size_t)v.W + 1));
    u64* acc = acc_buf.as<u64>();
    std::vector<u64> h(16 + v.W, 0);
    h[4] = ~0ull;
    EDSX_HIP(hipMemcpyAsync(acc, h.data(), 8 * h.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_eds_stats, dim3(1024), dim3(256), 0, st, v.sym, v.n, v.elen, v.m, v.bits, v.W, (u64)l, acc, acc + 16);
    EDSX_HIP(hipMemcpyAsync(h.data(), acc, 8 * h.size(), hipMemcpyDeviceToHost, st));
    EDSX_HIP(hipStreamSynchronize(st));
    EDSX_HIP(hipGetLastError());
    out.n_symbols = v.n; out.n_strings = v.m; out.n_chars = h[8];
    out.num_degenerate = h[0]; out.total_change_size = h[1]; out.num_common_chars = h[2]; out.num_context_blocks = h[3];
    out.min_context = h[3] ? h[4] : 0; out.max_context = h[5]; out.num_empty_strings = h[7];
    out.is_leds = (l == 0 || !h[6]) ? 1 : 0;
    if (v.bits) {
        out.total_paths = h[9]; out.max_paths_per_string = h[10];
        for (u32 w = 0; w < v.W; w++) out.num_paths += (u64)__builtin_popcountll(h[16 + w]);
    }
}

} // namespace edsx
