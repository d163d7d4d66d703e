// msa_slabs.hpp — the host code of the column-slab partition of msa2eds, without a HIP include (as vcf_host.hpp,
// path_records.hpp, lift_core.hpp and slice_core.hpp): the geometry of a FASTA alignment image, the slab cuts, what a
// slab tells the others about its ends (edge descriptors for l = 0, anchors for a context length l > 0), and the stitch
// that follows from the descriptors of all slabs - which bytes of every slab's own text survive and which boundaries are
// recomputed, by whom, from which raw columns.  The ranks of MultiMsa::run_rank and the column batches of
// msa_transform_batched (multi_gpu.hip) both run on it; edsparser_amd/multigpu.py restates the same logic for the Python
// front end.  hipcc compiles it into the library, g++ into tests/cpp/test_msa_slabs.cpp, which runs it under the address
// and undefined-behaviour sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

namespace edsx {

typedef unsigned long long u64;

// ---------------------------------------------------------------------------------------------------------------
// FASTA geometry (the row index of msa_transforms.cpp:46-68 for a plain uniform alignment)
// ---------------------------------------------------------------------------------------------------------------
// ok == false: not partitioned (the unpartitioned transform words the error).  start: where every row's data begins,
// draw: its bytes in the file, lw: the line width of wrapped rows (0: one line per row), L: its columns
struct MsaLayout { bool ok = false; std::vector<u64> start; u64 draw = 0, lw = 0, L = 0; };

inline MsaLayout msa_layout(const uint8_t* f, size_t n)
{
    MsaLayout lay;
    if (n == 0 || f[0] != '>') return lay;
    const uint8_t* he = static_cast<const uint8_t*>(memchr(f, '\n', n));
    if (!he) return lay;
    const u64 start0 = (u64)(he - f) + 1;
    if (start0 >= n) return lay;
    const uint8_t* nl = static_cast<const uint8_t*>(memchr(f + start0, '\n', n - start0));
    if (!nl) return lay;
    // first "\n>" behind the first header
    u64 h2 = n;
    for (const uint8_t* p = nl; p;) {
        const u64 i = (u64)(p - f);
        if (i + 1 < n && f[i + 1] == '>') { h2 = i; break; }
        if (i + 1 >= n) break;
        p = static_cast<const uint8_t*>(memchr(f + i + 1, '\n', n - i - 1));
    }
    if (h2 >= n) return lay;
    const u64 lw = (u64)(nl - f) - start0, draw = h2 - start0;
    if (lw == 0) return lay;
    u64 L, wrapped = 0;
    if (draw == lw) L = lw;
    else {
        const u64 nlines = (draw + 1 + lw) / (lw + 1);
        L = draw + 1 - nlines;
        wrapped = 1;
        if (L == 0 || (L - 1) / lw != nlines - 1) return lay;
    }
    u64 st = start0;
    while (true) {
        if (st + draw > n) return lay;
        lay.start.push_back(st);
        const u64 q = st + draw;
        if (q == n) break;
        if (f[q] != '\n') return lay;
        if (q + 1 == n) break;
        if (f[q + 1] != '>') {                           // blank lines at the very end only
            for (u64 i = q + 1; i < n; i++) if (f[i] != '\n') return lay;
            break;
        }
        const uint8_t* e = static_cast<const uint8_t*>(memchr(f + q + 1, '\n', n - q - 1));
        if (!e) return lay;
        st = (u64)(e - f) + 1;
    }
    if (lay.start.size() < 2) return lay;
    if (wrapped)                                          // every data line but a row's last has lw columns and then '\n'
        for (u64 s : lay.start)
            for (u64 o = lw; o < draw; o += lw + 1) if (f[s + o] != '\n') return lay;
    lay.draw = draw; lay.lw = wrapped ? lw : 0; lay.L = L; lay.ok = true;
    return lay;
}

// slab r of N is the columns [slab_cut(L, r, N), slab_cut(L, r + 1, N))
inline u64 slab_cut(u64 L, int r, int N) { return L * (u64)r / (u64)N; }

// whether an alignment is cut into N slabs at all: two columns per slab, and for an l-EDS room for a standalone common
// run at either end of every slab (at least 4 l columns)
inline bool slabs_fit(const MsaLayout& lay, int N, uint32_t l)
{
    return lay.ok && N >= 2 && lay.L >= 2ull * (u64)N && lay.L / (u64)N >= 4ull * l;
}

// columns [c0, c1) of row s -> dst: column c of a wrapped row is its byte c + c / lw (msa_transforms.cpp:268-269)
inline void row_columns(const uint8_t* fasta, const MsaLayout& lay, u64 s, u64 c0, u64 c1, uint8_t* dst)
{
    const uint8_t* row = fasta + lay.start[s];
    if (lay.lw == 0) { std::memcpy(dst, row + c0, c1 - c0); return; }
    for (u64 c = c0; c < c1;) {
        const u64 take = std::min<u64>(lay.lw - c % lay.lw, c1 - c);
        std::memcpy(dst, row + c + c / lay.lw, take);
        dst += take; c += take;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// l = 0: edge descriptors and the stitch plan (edsparser_amd/multigpu.py::plan_stitch)
// ---------------------------------------------------------------------------------------------------------------
struct SlabEdges {              // twelve u64, exchanged as they are
    u64 n_segments, cols, eds_bytes, seds_bytes;
    u64 first_is_variant, first_cols, first_eds_bytes, first_seds_bytes;
    u64 last_is_variant, last_cols, last_eds_bytes, last_seds_bytes;
};
// e: MsaPipeline::Edges of a slab of ncols columns whose text has E and Q bytes
template <class EdgeInfo> SlabEdges slab_edges(const EdgeInfo& e, u64 ncols, u64 E, u64 Q)
{
    return SlabEdges{e.nseg, ncols, E, Q, e.fvar, e.fcols, e.feds, e.fseds, e.lvar, e.lcols, e.leds, e.lseds};
}

struct SlabChain { int first, last; bool variant; };      // a run of one type over slabs first .. last
struct SlabAction {             // what a rank does to its slab text: bytes dropped at both ends, chains it recomputes
    u64 front_eds = 0, front_seds = 0, back_eds = 0, back_seds = 0;
    std::vector<int> owns;
};
struct StitchPlan { std::vector<SlabChain> chains; std::vector<SlabAction> actions; };

inline StitchPlan plan_stitch(const std::vector<SlabEdges>& e)
{
    const int n = (int)e.size();
    StitchPlan p;
    p.actions.resize(n);
    std::vector<char> join(n > 0 ? n - 1 : 0);
    for (int s = 0; s + 1 < n; s++) join[s] = e[s].last_is_variant == e[s + 1].first_is_variant;
    for (int s = 0; s + 1 < n;) {
        if (!join[s]) { s++; continue; }
        int b = s + 1;
        while (b < n - 1 && join[b] && e[b].n_segments == 1) b++;         // a slab that is ONE run passes the chain on
        p.chains.push_back(SlabChain{s, b, e[s].last_is_variant != 0});
        s = b;
    }
    for (int ci = 0; ci < (int)p.chains.size(); ci++) {
        const SlabChain& ch = p.chains[ci];
        if (!ch.variant) {              // common run: joined textually - "{" and "{0}" go on the right, "}" on the left
            for (int i = ch.first + 1; i <= ch.last; i++) { p.actions[i].front_eds += 1; p.actions[i].front_seds += 3; }
            for (int i = ch.first; i < ch.last; i++) p.actions[i].back_eds += 1;
        } else {                        // variant run: the left-most slab recomputes it from the raw columns
            p.actions[ch.first].back_eds += e[ch.first].last_eds_bytes;
            p.actions[ch.first].back_seds += e[ch.first].last_seds_bytes;
            p.actions[ch.first].owns.push_back(ci);
            for (int i = ch.first + 1; i <= ch.last; i++) {
                p.actions[i].front_eds += e[i].first_eds_bytes;
                p.actions[i].front_seds += e[i].first_seds_bytes;
            }
        }
    }
    return p;
}

// column range (col0, ncols) of slab `rank` inside a variant chain
inline bool chain_columns(const SlabChain& ch, int rank, const std::vector<SlabEdges>& e, u64& col0, u64& ncols)
{
    if (rank < ch.first || rank > ch.last) return false;
    if (rank == ch.first) { col0 = e[rank].cols - e[rank].last_cols; ncols = e[rank].last_cols; }
    else { col0 = 0; ncols = e[rank].first_cols; }                        // (the whole slab when it is a single run)
    return true;
}

// ---------------------------------------------------------------------------------------------------------------
// l > 0 (parse_msa_to_leds_streaming).  An l-EDS joins variant runs with the common runs of fewer than l columns between
// them; only a common run of at least l columns (or one at either end of the alignment) stands alone
// (msa_transforms.cpp:133-190).  A slab transformed on its own applies the "at either end" clause at ITS ends, so its
// text is the alignment's text only between its first and its last standalone run of >= l columns - its anchors: what
// lies between two anchors depends on nothing outside them.  Every boundary is therefore recomputed from the last
// anchor of the left slab to the first anchor of the right one (both included: a mini alignment that begins and ends
// with a standalone run, transformed with the same l), by the left slab's owner.
//   slab r keeps   text[ behind its first anchor .. in front of its last anchor )      (slab 0 from its start, the
//   last slab to its end), followed by the text of the boundary r | r+1.
// A slab without two distinct anchors (or one whose anchors lie more than ANCHOR_MAX_COLS from its ends) is not ok: the
// alignment is then transformed in one piece.
// ---------------------------------------------------------------------------------------------------------------
struct SlabAnchors {            // twelve u64, exchanged as they are
    u64 cols, eds_bytes, seds_bytes, ok;
    u64 tail_col, tail_eds, tail_seds;          // last anchor: its first column, text offsets in front of it
    u64 head_end, head_eds, head_seds;          // first anchor: the column behind it, text offsets behind it
    u64 pad0, pad1;
};
constexpr u64 ANCHOR_MAX_COLS = 1u << 16;

// a: MsaPipeline::Anchors of slab r of N (ncols columns, E and Q bytes of text) - found, first_seg, last_seg, last_col,
// last_eds, last_seds, first_end, first_eds_end, first_seds_end.  A middle slab needs two distinct anchors, the first
// slab only a last one, the last slab only a first one
template <class AnchorInfo> SlabAnchors slab_anchors(const AnchorInfo& a, int r, int N, u64 ncols, u64 E, u64 Q)
{
    SlabAnchors m{};
    m.cols = ncols; m.eds_bytes = E; m.seds_bytes = Q;
    const bool need_head = r > 0, need_tail = r + 1 < N;
    bool ok = a.found != 0;
    if (ok && need_head && need_tail) ok = a.first_seg < a.last_seg;
    if (ok && need_head) ok = a.first_end <= ANCHOR_MAX_COLS;
    if (ok && need_tail) ok = ncols - a.last_col <= ANCHOR_MAX_COLS;
    if (!ok) return m;
    m.ok = 1;
    m.tail_col = need_tail ? a.last_col : ncols; m.tail_eds = need_tail ? a.last_eds : E; m.tail_seds = need_tail ? a.last_seds : Q;
    m.head_end = need_head ? a.first_end : 0; m.head_eds = need_head ? a.first_eds_end : 0; m.head_seds = need_head ? a.first_seds_end : 0;
    return m;
}

// ---------------------------------------------------------------------------------------------------------------
// The stitch, for both context lengths: slab r contributes the bytes [elo, ehi) of its .eds text and [slo, shi) of its
// .seds text, followed by the texts of the jobs it owns, in job order.  A job is one boundary segment that is
// recomputed from raw columns: its parts, left to right, are the columns [col0, col0 + ncols) of slab `slab`, and they
// are neighbours in the alignment.  Between ranks every slab sends the columns of all its parts as ONE payload, the
// parts in job order, each a row-major block: `before` is the number of columns in front of a part in its slab's
// payload, max_cols the columns of the widest payload.
// ---------------------------------------------------------------------------------------------------------------
struct SlabKeep { u64 elo, ehi, slo, shi; };
struct SlabPart { int slab; u64 col0, ncols, before; };
struct SlabJob { int owner; std::vector<SlabPart> parts; };
struct SlabStitch {
    std::vector<SlabKeep> keep;
    std::vector<SlabJob> jobs;
    int chains = 0;             // runs joined over a cut, textually or by a job (MultiMsa::chains)
    u64 max_cols = 0;
};

inline void lay_out_payloads(SlabStitch& st)
{
    std::vector<u64> cols(st.keep.size(), 0);
    for (SlabJob& j : st.jobs)
        for (SlabPart& p : j.parts) { p.before = cols[p.slab]; cols[p.slab] += p.ncols; }
    for (u64 c : cols) st.max_cols = std::max(st.max_cols, c);
}

// l = 0: the plan of plan_stitch; one job per variant chain, owned by its left-most slab
inline SlabStitch stitch_from_edges(const std::vector<SlabEdges>& edges)
{
    const StitchPlan plan = plan_stitch(edges);
    SlabStitch st;
    st.chains = (int)plan.chains.size();
    for (size_t r = 0; r < edges.size(); r++) {
        const SlabEdges& e = edges[r];
        const SlabAction& a = plan.actions[r];
        SlabKeep k{a.front_eds, e.eds_bytes - std::min(e.eds_bytes, a.back_eds), a.front_seds, e.seds_bytes - std::min(e.seds_bytes, a.back_seds)};
        if (k.ehi < k.elo) k.ehi = k.elo;
        if (k.shi < k.slo) k.shi = k.slo;
        st.keep.push_back(k);
    }
    for (const SlabChain& ch : plan.chains) {
        if (!ch.variant) continue;
        SlabJob j{ch.first, {}};
        for (int r = ch.first; r <= ch.last; r++) {
            SlabPart p{r, 0, 0, 0};
            chain_columns(ch, r, edges, p.col0, p.ncols);
            j.parts.push_back(p);
        }
        st.jobs.push_back(j);
    }
    lay_out_payloads(st);
    return st;
}

// l > 0: one job per boundary r | r+1, owned by r - the tail of slab r from its last anchor and the head of slab r+1 to
// behind its first one.  ok = false (and nothing else): some slab has no usable anchors
inline SlabStitch stitch_from_anchors(const std::vector<SlabAnchors>& a, bool& ok)
{
    SlabStitch st;
    const int N = (int)a.size();
    ok = true;
    for (const SlabAnchors& m : a) if (!m.ok) ok = false;
    if (!ok) return st;
    st.chains = N - 1;
    for (int r = 0; r < N; r++) {
        st.keep.push_back(SlabKeep{a[r].head_eds, a[r].tail_eds, a[r].head_seds, a[r].tail_seds});
        if (r + 1 < N) st.jobs.push_back(SlabJob{r, {SlabPart{r, a[r].tail_col, a[r].cols - a[r].tail_col, 0}, SlabPart{r + 1, 0, a[r + 1].head_end, 0}}});
    }
    lay_out_payloads(st);
    return st;
}

// row-major blocks (data, ncols) of the same S rows, left to right -> a one-line-per-row alignment image: per row
// ">r\n" + its columns + "\n"
inline void mini_image(u64 S, const std::vector<std::pair<const uint8_t*, u64>>& parts, std::vector<uint8_t>& out)
{
    u64 width = 0;
    for (const auto& p : parts) width += p.second;
    out.resize(S * (width + 4));
    uint8_t* d = out.data();
    for (u64 s = 0; s < S; s++) {
        d[0] = '>'; d[1] = 'r'; d[2] = '\n'; d += 3;
        for (const auto& p : parts) { std::memcpy(d, p.first + s * p.second, p.second); d += p.second; }
        *d++ = '\n';
    }
}

// sizes: `stride` numbers per rank as all-gathered, the first two the bytes of its .eds and .seds piece -> where rank r
// writes, and the totals
inline void piece_offsets(const std::vector<u64>& sizes, size_t stride, int r, u64& eoff, u64& soff, u64& etot, u64& stot)
{
    eoff = soff = etot = stot = 0;
    for (size_t k = 0; k * stride < sizes.size(); k++) {
        if ((int)k < r) { eoff += sizes[stride * k]; soff += sizes[stride * k + 1]; }
        etot += sizes[stride * k]; stot += sizes[stride * k + 1];
    }
}

} // namespace edsx
