// merge_multi.hip — eds2leds over several GPUs of one node from C++: symbol ranges (the C++ port of
// edsparser_amd/multigpu.py, MergeSharder), host code on the rank threads and exchanges of multi_gpu.hip.
//
// A sentinel - a single-string symbol of at least l characters between two degenerate symbols - is in no mergeable pair,
// so the text on either side of it merges exactly as inside the whole text (merge_device.hpp, MergeShard).  Neighbouring
// ranges share one sentinel; the left one prints it.  Every phase ends in the rank barrier (rank_barrier.hpp):
//   1. rank r scans its slice [end r / N, end (r+1) / N) of the .eds on its device (merge_scan.hip: string starts,
//      validity, the first sentinel whose '}' lies in the slice) and, LINEAR, its slice of the .seds ('{' per block);
//   2. all-gather of a fixed record per rank; every rank derives the same string bases and cut ranks;
//   3. LINEAR: the ranks whose '{' ordinals hold a sentinel's string locate its source set (the k-th '{' ... '}') with
//      the block prefixes still in HBM, and the spans are all-gathered;
//   4. every owner of a range (rank 0 and the cut ranks) runs MergePipeline::run on eds[e0, e1) / seds[s0, s1) with its
//      head / tail sentinel flags; all-gather of the piece sizes and an ok flag (the sentinels came through unmerged);
//   5. rank 0 allocates the outputs, every rank copies its piece to its offset.
// Rank 0 merges the whole text instead - which also gives edsx_leds_merge's output, status and error text - when there
// is one rank or l = 0, a slice is not plain text, no slice but the first holds a sentinel, the source sets do not match
// the strings, or a sentinel was merged / a range failed.
#include "multi_gpu.hpp"

#include <algorithm>
#include <cstring>

namespace edsx {

namespace {

struct MergeRec { u64 ok, strings, has_cut, sym_start, sym_end, strings_before, braces; };     // exchanged as it is
constexpr u64 NONE = ~0ull;

} // namespace

struct MultiMsa::MergeShared {
    const uint8_t* eds; u64 eds_n; const uint8_t* seds; u64 seds_n;     // seds == nullptr: CARTESIAN
    uint32_t l; bool compact;
    HostBytes* leds; HostBytes* sout;
    std::vector<std::exception_ptr> error;                              // per rank
    std::vector<u64> eds_h2d, seds_h2d, range_bytes;                    // per rank (range_bytes NONE: owns no range)
    int fallback = 0, ranges = 1;                                       // written by rank 0
};

void MultiMsa::run_rank_merge(int r, MergeShared& sh)
{
    const int N = world();
    Rank& me = *ranks_[r];
    std::string fail;
    auto phase = [&](auto&& body) -> bool { return rank_phase(*bar_, r, fail, body, &sh.error[r]); };
    hipStream_t st = nullptr;
    const bool linear = sh.seds != nullptr;
    auto cut = [&](u64 n, int k) { return (u64)((unsigned __int128)n * (unsigned)k / (unsigned)N); };
    int why = (N == 1 || sh.l == 0) ? 1 : 0;

    HostBytes out, so;
    if (!why) {
        // ---- 1. my slices of the .eds and the .seds
        MergeRec mine{};
        if (!phase([&] {
                EDSX_HIP(hipSetDevice(me.device));
                if (!me.scan) me.scan.reset(new RangeScanner());
                me.scan->reset_h2d();
                const u64 end = text_end(sh.eds, sh.eds_n);
                const EdsRangeScan s = me.scan->eds(sh.eds, sh.eds_n, end, cut(end, r), cut(end, r + 1), sh.l, st);
                bool sok = true;
                u64 braces = 0;
                if (linear) {
                    const u64 send = text_end(sh.seds, sh.seds_n);
                    sok = me.scan->seds_count(sh.seds, sh.seds_n, cut(send, r), cut(send, r + 1), braces, st);
                }
                mine = MergeRec{s.ok && sok ? 1ull : 0ull, s.strings, s.has_cut ? 1ull : 0ull, s.sym_start, s.sym_end,
                                s.strings_before, braces};
                sh.eds_h2d[r] = me.scan->eds_h2d();
                sh.seds_h2d[r] = me.scan->seds_h2d();
            })) return;

        // ---- 2. every rank's record -> string bases, cut ranks, sentinels (start, end, string index)
        std::vector<MergeRec> g1(N);
        if (!phase([&] { xch_->all_gather(r, &mine, sizeof(MergeRec), g1.data()); })) return;
        std::vector<u64> str_base(N + 1, 0), br_base(N + 1, 0), sent_s(N, 0), sent_e(N, 0), sent_i(N, 0);
        std::vector<int> cut_ranks;
        for (int k = 0; k < N; k++) {
            if (!g1[k].ok) why = 2;
            str_base[k + 1] = str_base[k] + g1[k].strings;
            br_base[k + 1] = br_base[k] + g1[k].braces;
        }
        if (!why) {
            for (int k = 1; k < N; k++) {
                if (!g1[k].has_cut) continue;
                cut_ranks.push_back(k);
                sent_s[k] = g1[k].sym_start; sent_e[k] = g1[k].sym_end; sent_i[k] = str_base[k] + g1[k].strings_before;
            }
            if (cut_ranks.empty()) why = 3;
            else if (linear && br_base[N] != str_base[N]) why = 4;          // the source count differs from the cardinality
        }

        // ---- 3. the source set of string M starts at the M-th '{' of the .seds
        std::vector<u64> loc0(N, NONE), loc1(N, 0);
        if (!why && linear) {
            std::vector<u64> flat(2 * (size_t)N, NONE), all(2 * (size_t)N * N);
            if (!phase([&] {
                    std::vector<int> which;
                    std::vector<u64> ord;
                    for (int k : cut_ranks)
                        if (br_base[r] <= sent_i[k] && sent_i[k] < br_base[r + 1]) { which.push_back(k); ord.push_back(sent_i[k] - br_base[r]); }
                    std::vector<u64> p0(ord.size()), p1(ord.size());
                    me.scan->seds_locate(ord.data(), ord.size(), p0.data(), p1.data(), st);
                    for (size_t i = 0; i < which.size(); i++) { flat[2 * which[i]] = p0[i]; flat[2 * which[i] + 1] = p1[i]; }
                })) return;
            if (!phase([&] { xch_->all_gather(r, flat.data(), 16 * (size_t)N, all.data()); })) return;
            for (int q = 0; q < N; q++)
                for (int k = 0; k < N; k++)
                    if (all[2 * ((size_t)q * N + k)] != NONE) { loc0[k] = all[2 * ((size_t)q * N + k)]; loc1[k] = all[2 * ((size_t)q * N + k) + 1]; }
            for (int k : cut_ranks)
                if (loc0[k] == NONE || loc1[k] == 0) why = 4;                // the source set of a sentinel was not found
        }

        if (!why) {
            // ---- 4. my range
            std::vector<int> owners{0};
            owners.insert(owners.end(), cut_ranks.begin(), cut_ranks.end());
            const auto at = std::find(owners.begin(), owners.end(), r);
            u64 ok = 1;
            if (!phase([&] {
                    if (at == owners.end()) return;
                    const size_t i = (size_t)(at - owners.begin());
                    const int nxt = i + 1 < owners.size() ? owners[i + 1] : -1;
                    const u64 e0 = r == 0 ? 0 : sent_s[r], e1 = nxt < 0 ? sh.eds_n : sent_e[nxt];
                    u64 s0 = 0, s1 = 0;
                    if (linear) { s0 = r == 0 ? 0 : loc0[r]; s1 = nxt < 0 ? sh.seds_n : loc1[nxt]; }
                    sh.range_bytes[r] = e1 - e0;
                    sh.eds_h2d[r] += e1 - e0;
                    sh.seds_h2d[r] += s1 - s0;
                    try {           // any failure sends the whole text to rank 0 (which words the exact error)
                        if (!me.merge) me.merge.reset(new MergePipeline());
                        MergeShard shard;
                        shard.head_sentinel = r != 0;
                        shard.tail_sentinel = nxt >= 0;
                        me.merge->run(me.merge_eds, sh.eds + e0, e1 - e0, linear ? sh.seds + s0 : nullptr, s1 - s0, sh.l, sh.compact, out, so, st, &shard);
                        ok = shard.head_intact && shard.tail_intact ? 1 : 0;
                    } catch (const std::exception&) { ok = 0; }
                })) return;
            const u64 my[3] = {out.size, so.size, ok};
            std::vector<u64> g3(3 * (size_t)N);
            if (!phase([&] { xch_->all_gather(r, my, sizeof(my), g3.data()); })) return;
            for (int k = 0; k < N; k++)
                if (!g3[3 * k + 2]) why = 5;
            if (!why) {
                // ---- 5. rank 0 allocates, every rank copies its piece to its offset
                u64 eoff, soff, etot, stot;
                piece_offsets(g3, 3, r, eoff, soff, etot, stot);
                if (!phase([&] {
                        if (r != 0) return;
                        sh.leds->take(etot); sh.sout->take(stot);
                        sh.ranges = (int)owners.size();
                    })) return;
                phase([&] {
                    if (out.size) std::memcpy(sh.leds->data + eoff, out.data, out.size);
                    if (so.size) std::memcpy(sh.sout->data + soff, so.data, so.size);
                });
                return;
            }
        }
    }

    // ---- the whole text on rank 0: the unpartitioned merge, with its output or its error
    sh.range_bytes[r] = NONE;
    phase([&] {
        if (r != 0) return;
        sh.fallback = why;
        sh.ranges = 1;
        sh.range_bytes[0] = sh.eds_n;
        sh.eds_h2d[0] += sh.eds_n;
        sh.seds_h2d[0] += linear ? sh.seds_n : 0;
        EDSX_HIP(hipSetDevice(me.device));
        if (!me.merge) me.merge.reset(new MergePipeline());
        me.merge->run(me.merge_eds, sh.eds, sh.eds_n, sh.seds, sh.seds_n, sh.l, sh.compact, *sh.leds, *sh.sout, st);
    });
}

void MultiMsa::leds_merge_multi(const uint8_t* eds, size_t eds_n, const uint8_t* seds, size_t seds_n, uint32_t context_len,
                                bool compact, HostBytes& leds, HostBytes& seds_out)
{
    static const uint8_t none = 0;
    const int N = world();
    merge_info_ = MergeMultiInfo();
    MergeShared sh;
    sh.eds = eds ? eds : &none; sh.eds_n = eds_n; sh.seds = seds; sh.seds_n = seds ? seds_n : 0;
    sh.l = context_len; sh.compact = compact;
    sh.leds = &leds; sh.sout = &seds_out;
    sh.error.assign(N, nullptr);
    sh.eds_h2d.assign(N, 0); sh.seds_h2d.assign(N, 0); sh.range_bytes.assign(N, NONE);
    run_ranks([&](int r) { run_rank_merge(r, sh); }, &sh.error);
    MergeMultiInfo& info = merge_info_;
    info.fallback = sh.fallback;
    info.partitioned = sh.fallback == 0;
    info.ranges = sh.ranges;
    bool first = true;
    for (int r = 0; r < N; r++) {
        info.eds_h2d_bytes_max = std::max(info.eds_h2d_bytes_max, sh.eds_h2d[r]);
        info.seds_h2d_bytes_max = std::max(info.seds_h2d_bytes_max, sh.seds_h2d[r]);
        if (sh.range_bytes[r] == NONE) continue;
        info.range_bytes_min = first ? sh.range_bytes[r] : std::min(info.range_bytes_min, sh.range_bytes[r]);
        info.range_bytes_max = std::max(info.range_bytes_max, sh.range_bytes[r]);
        first = false;
    }
}

} // namespace edsx
