// path_records.hpp — the arithmetic of the record driver of a path session (PathPipeline::emit_records, path_device.hip):
// header texts, the layout of the records of spell / align / walks in the caller's buffer, and the output batches a table
// batch is cut into.  Host code without a HIP include, in the style of lift_core.hpp / slice_core.hpp: g++ compiles it for
// tests/cpp/test_path_records.cpp, which runs it under the address and undefined-behaviour sanitizers.
//
// A record is a header text followed by a body.  Its body follows from its length L (characters, columns or token bytes):
//   FASTA (spell, align)   the L characters in lines of lw, a line feed behind each: L + ceil(L / lw) bytes, none for L = 0;
//                          lw is the line width asked for, or L (at least 1) when that is 0 or larger.  An empty sequence
//                          keeps its header.  (align: every record has the same L, so the same lw and body.)
//   WALK                   the L token bytes, the last comma a tab, then "*\n": L + 2 bytes; lw = 0.  A path without a
//                          step (L = 0) has no record at all: no header, no bytes, and it is in no batch.
#pragma once

#include <stddef.h>
#include <algorithm>
#include <string>
#include <vector>

namespace edsx {

// one requested path of an output batch: where its record and its body start in the batch's buffer, where its header
// text lies in the header blob, its length, the line width in force (>= 1; walks: 0), the body bytes and its row of the
// choice tables
struct PathRec { unsigned long long rec_off, body_off, hdr_src, L, lw, body, row; };

namespace records {

typedef unsigned long long u64;

enum Rule { FASTA, WALK };

// the header texts of n records laid end to end; off (n + 1 entries): where each begins
struct Headers { std::string blob; std::vector<u64> off; };

inline std::string default_name(const char* prefix, u64 id) { return std::string(prefix ? prefix : "path") + std::to_string(id); }

// ">name\n" per record (names[k], else prefix - null: "path" - + id)
inline Headers fasta_headers(const u64* ids, size_t n, const char* const* names, const char* prefix)
{
    Headers h;
    h.off.assign(n + 1, 0);
    for (size_t k = 0; k < n; k++) {
        h.blob += '>';
        h.blob += names ? std::string(names[k]) : default_name(prefix, ids[k]);
        h.blob += '\n';
        h.off[k + 1] = h.blob.size();
    }
    return h;
}

// "P\t<name>\t" per record; bad_name (-> the index of the first name that is empty or holds a tab, line feed or blank, else n)
inline Headers walk_headers(const u64* ids, size_t n, const char* const* names, const char* prefix, size_t& bad_name)
{
    Headers h;
    h.off.assign(n + 1, 0);
    bad_name = n;
    for (size_t k = 0; k < n; k++) {
        const std::string name = names ? std::string(names[k]) : default_name(prefix, ids[k]);
        if (name.empty() || name.find_first_of("\t\n ") != std::string::npos) { bad_name = k; return h; }
        h.blob += "P\t" + name + "\t";
        h.off[k + 1] = h.blob.size();
    }
    return h;
}

// the line width in force and the body bytes of a record of length L
inline void body_of(Rule rule, u64 L, u64 line_width, u64& lw, u64& body)
{
    if (rule == WALK) { lw = 0; body = L ? L + 2 : 0; return; }
    lw = (line_width == 0 || line_width > L) ? std::max<u64>(L, 1) : line_width;
    body = L ? L + (L + lw - 1) / lw : 0;
}

// rec[k] without its two batch offsets; start (n + 1 entries): where record k begins in the caller's buffer, start[n] the total
struct Layout { std::vector<PathRec> rec; std::vector<u64> start; };

// len[k]: the length of record k; hoff: Headers::off; KT: records per table batch (record k reads table row k % KT)
inline Layout layout(Rule rule, const u64* len, size_t n, const u64* hoff, u64 line_width, u64 KT)
{
    Layout y;
    y.rec.resize(n);
    y.start.assign(n + 1, 0);
    for (size_t k = 0; k < n; k++) {
        PathRec& r = y.rec[k];
        r.rec_off = r.body_off = 0;
        r.L = len[k];
        body_of(rule, r.L, line_width, r.lw, r.body);
        r.hdr_src = hoff[k];
        r.row = k % KT;
        const bool dropped = rule == WALK && r.L == 0;
        y.start[k + 1] = y.start[k] + (dropped ? 0 : (hoff[k + 1] - hoff[k]) + r.body);
    }
    return y;
}

// the output batch that begins with record r0 of the table batch [i0, i1) ends in front of record batch_end: one record,
// then as many more as keep the batch within the budget
inline size_t batch_end(const std::vector<u64>& start, size_t r0, size_t i1, u64 budget)
{
    size_t r1 = r0 + 1;
    while (r1 < i1 && start[r1 + 1] - start[r0] <= budget) r1++;
    return r1;
}

// the records of the batch [r0, r1) that have bytes, with their offsets in the batch's buffer -> the largest body among them
inline u64 batch_records(const Layout& y, const u64* hoff, size_t r0, size_t r1, std::vector<PathRec>& batch)
{
    u64 max_body = 0;
    batch.clear();
    for (size_t k = r0; k < r1; k++) {
        if (y.start[k + 1] == y.start[k]) continue;
        PathRec r = y.rec[k];
        r.rec_off = y.start[k] - y.start[r0];
        r.body_off = r.rec_off + (hoff[k + 1] - hoff[k]);
        max_body = std::max(max_body, r.body);
        batch.push_back(r);
    }
    return max_body;
}

} // namespace records
} // namespace edsx
