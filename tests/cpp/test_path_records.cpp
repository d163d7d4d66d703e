// test_path_records.cpp — the arithmetic of the record driver of a path session on the CPU:
// edsparser_amd/csrc/path_records.hpp (header texts, record layout, output batches, as PathPipeline::emit_records walks
// them), over a case file written by tests/test_path_records_cpu.py; meant to be built with -fsanitize=address,undefined.
// Nothing here allocates by the lengths it is given: a case with records of several GB is numbers only.
//
// Case (u64, little endian): rule (0 spell, 1 align, 2 walks), n, line_width, KT, budget, ids[n], len[n].  The names are
// the default ones, "path" + id.
// Result: the header blob (its size, then one word per byte) and off[n + 1]; the total; per record L lw body hdr_src row
// start; then per table batch [i0, i1) and output batch inside it: i0 r0 r1 bytes nrec max_body, and per record of the
// batch rec_off body_off hdr_src L lw body row; a word of ~0 ends the case.
#include "path_records.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

using namespace edsx;
using records::u64;

namespace {

struct Reader {
    const std::vector<uint8_t>& f;
    size_t at = 0;
    u64 one()
    {
        if (at + 8 > f.size()) { std::fprintf(stderr, "case file cut short\n"); std::exit(2); }
        u64 v; std::memcpy(&v, f.data() + at, 8); at += 8; return v;
    }
    std::vector<u64> block(u64 count)
    {
        std::vector<u64> v(count);
        for (auto& x : v) x = one();
        return v;
    }
};

int fail(const char* what) { std::fprintf(stderr, "%s\n", what); return 1; }

// the header functions on names of the caller's: texts, offsets and the name check of the P lines
int check_names()
{
    const u64 ids[3] = {7, 8, 9};
    const char* good[3] = {"a", "chr1#2", ">x"};
    const records::Headers f = records::fasta_headers(ids, 3, good, "ignored");
    if (f.blob != ">a\n>chr1#2\n>>x\n" || f.off != std::vector<u64>{0, 3, 11, 15}) return fail("fasta_headers with names");
    if (records::fasta_headers(ids, 2, nullptr, "hap").blob != ">hap7\n>hap8\n") return fail("fasta_headers with a prefix");
    if (records::fasta_headers(ids, 0, nullptr, nullptr).off != std::vector<u64>{0}) return fail("fasta_headers of nothing");
    size_t bad = 99;
    const records::Headers w = records::walk_headers(ids, 3, good, nullptr, bad);
    if (bad != 3 || w.blob != "P\ta\tP\tchr1#2\tP\t>x\t" || w.off != std::vector<u64>{0, 4, 13, 18}) return fail("walk_headers with names");
    const char* bads[4][3] = {{"a", "", "c"}, {"a b", "b", "c"}, {"a", "b", "c\td"}, {"a", "b\n", ""}};
    const size_t where[4] = {1, 0, 2, 1};
    for (int k = 0; k < 4; k++) {
        records::walk_headers(ids, 3, bads[k], nullptr, bad);
        if (bad != where[k]) return fail("walk_headers: the first bad name");
    }
    records::walk_headers(ids, 3, nullptr, "my hap", bad);
    if (bad != 0) return fail("walk_headers: a prefix with a blank");
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: test_path_records cases.bin results.bin\n"); return 2; }
    if (check_names()) return 1;
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::ofstream out(argv[2], std::ios::binary);
    auto put = [&](u64 v) { out.write(reinterpret_cast<const char*>(&v), 8); };
    Reader r{file};
    size_t cases = 0;
    while (r.at < file.size()) {
        const u64 kind = r.one(), n = r.one(), line_width = r.one(), KT = r.one(), budget = r.one();
        const std::vector<u64> ids = r.block(n), len = r.block(n);
        if (kind > 2 || n == 0 || KT == 0) return fail("bad case");
        const records::Rule rule = kind == 2 ? records::WALK : records::FASTA;
        size_t bad = n;
        const records::Headers h = rule == records::WALK ? records::walk_headers(ids.data(), n, nullptr, nullptr, bad)
                                                         : records::fasta_headers(ids.data(), n, nullptr, nullptr);
        if (bad != n || h.off.size() != n + 1 || h.off[n] != h.blob.size()) return fail("headers");
        put(h.blob.size());
        for (unsigned char c : h.blob) put(c);
        for (u64 v : h.off) put(v);
        const records::Layout y = records::layout(rule, len.data(), n, h.off.data(), line_width, KT);
        if (y.rec.size() != n || y.start.size() != n + 1) return fail("layout sizes");
        put(y.start[n]);
        for (size_t k = 0; k < n; k++) {
            const PathRec& p = y.rec[k];
            put(p.L); put(p.lw); put(p.body); put(p.hdr_src); put(p.row); put(y.start[k]);
        }
        std::vector<PathRec> batch;
        for (size_t i0 = 0; i0 < n; i0 += KT) {                  // as emit_records
            const size_t i1 = std::min<size_t>(n, i0 + KT);
            for (size_t r0 = i0, r1; r0 < i1; r0 = r1) {
                r1 = records::batch_end(y.start, r0, i1, budget);
                if (r1 <= r0 || r1 > i1) return fail("batch_end outside its table batch");
                const u64 max_body = records::batch_records(y, h.off.data(), r0, r1, batch);
                put(i0); put(r0); put(r1); put(y.start[r1] - y.start[r0]); put(batch.size()); put(max_body);
                for (const PathRec& p : batch) { put(p.rec_off); put(p.body_off); put(p.hdr_src); put(p.L); put(p.lw); put(p.body); put(p.row); }
            }
        }
        put(~0ull);
        cases++;
    }
    out.close();
    std::printf("%zu cases\n", cases);
    return out ? 0 : 1;
}
