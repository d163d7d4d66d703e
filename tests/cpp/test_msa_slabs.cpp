// test_msa_slabs.cpp — the host code of the column-slab partition of msa2eds on the CPU: edsparser_amd/csrc/msa_slabs.hpp
// (image geometry, slab cuts, descriptors, the stitch of both context lengths, mini alignments, piece offsets), over a
// case file written by tests/test_msa_slabs_cpu.py; meant to be built with -fsanitize=address,undefined.  The program
// computes and prints; what the numbers should be is the driver's business.
//
// The case file is a sequence of words (u64, little endian) and blobs (a word with the byte count, the bytes, zeros up to
// the next multiple of eight); so is the result file.  A case begins with its mode:
//   1 layout    blob image, N, l, nq, nq x (c0, c1)
//               -> ok; then only if ok: S, start[S], draw, lw, L, slabs_fit(N, l), slab_cut(L, 0 .. N, N), and per query
//               the blob of row_columns of every row, row after row
//   2 edges     N, N x the twelve words of SlabEdges           -> the stitch (below)
//   3 anchors   N, N x (the ten words of MsaPipeline::Anchors, ncols, E, Q)
//               -> N x the twelve words of slab_anchors, ok, then only if ok: the stitch
//   4 mini      S, np, np x (ncols, blob of S x ncols bytes)   -> the blob of mini_image
//   5 offsets   stride, r, n, n words                          -> eoff soff etot stot
// The stitch: chains, max_cols, N x (elo ehi slo shi), the number of jobs, per job owner, np, np x (slab col0 ncols before).
#include "msa_slabs.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

using namespace edsx;

namespace {

struct Reader {
    const std::vector<uint8_t>& f;
    size_t at = 0;
    u64 one()
    {
        if (at + 8 > f.size()) { std::fprintf(stderr, "case file cut short\n"); std::exit(2); }
        u64 v; std::memcpy(&v, f.data() + at, 8); at += 8; return v;
    }
    std::vector<uint8_t> blob()                                  // a copy of exactly its size: a read past it is seen
    {
        const u64 n = one();
        if (at + n > f.size()) { std::fprintf(stderr, "case file cut short\n"); std::exit(2); }
        std::vector<uint8_t> b(f.begin() + at, f.begin() + at + n);
        at += (n + 7) / 8 * 8;
        return b;
    }
};

struct Writer {
    std::ofstream out;
    void one(u64 v) { out.write(reinterpret_cast<const char*>(&v), 8); }
    void blob(const std::vector<uint8_t>& b)
    {
        one(b.size());
        out.write(reinterpret_cast<const char*>(b.data()), (std::streamsize)b.size());
        for (size_t i = b.size(); i % 8; i++) out.put(0);
    }
};

struct AnchorInfo { u64 nseg, found, first_seg, last_seg, last_col, last_eds, last_seds, first_end, first_eds_end, first_seds_end; };

void put_stitch(Writer& w, const SlabStitch& st)
{
    w.one((u64)st.chains); w.one(st.max_cols);
    for (const SlabKeep& k : st.keep) { w.one(k.elo); w.one(k.ehi); w.one(k.slo); w.one(k.shi); }
    w.one(st.jobs.size());
    for (const SlabJob& j : st.jobs) {
        w.one((u64)j.owner); w.one(j.parts.size());
        for (const SlabPart& p : j.parts) { w.one((u64)p.slab); w.one(p.col0); w.one(p.ncols); w.one(p.before); }
    }
}

} // namespace

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: test_msa_slabs cases.bin results.bin\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    Writer w{std::ofstream(argv[2], std::ios::binary)};
    Reader r{file};
    size_t cases = 0;
    for (; r.at < file.size(); cases++) {
        const u64 mode = r.one();
        if (mode == 1) {
            const std::vector<uint8_t> img = r.blob();
            const int N = (int)r.one();
            const uint32_t l = (uint32_t)r.one();
            const u64 nq = r.one();
            const MsaLayout lay = msa_layout(img.data(), img.size());
            w.one(lay.ok);
            const u64 S = lay.start.size();
            if (lay.ok) {
                w.one(S);
                for (u64 s : lay.start) w.one(s);
                w.one(lay.draw); w.one(lay.lw); w.one(lay.L); w.one(slabs_fit(lay, N, l));
                for (int k = 0; k <= N; k++) w.one(slab_cut(lay.L, k, N));
            }
            for (u64 q = 0; q < nq; q++) {
                const u64 c0 = r.one(), c1 = r.one();
                if (!lay.ok) continue;
                if (c0 > c1 || c1 > lay.L) { std::fprintf(stderr, "bad column query\n"); return 2; }
                std::vector<uint8_t> cols(S * (c1 - c0));
                for (u64 s = 0; s < S; s++) row_columns(img.data(), lay, s, c0, c1, cols.data() + s * (c1 - c0));
                w.blob(cols);
            }
        } else if (mode == 2) {
            std::vector<SlabEdges> edges(r.one());
            for (SlabEdges& e : edges) {
                u64 v[12];
                for (u64& x : v) x = r.one();
                e = SlabEdges{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11]};
            }
            put_stitch(w, stitch_from_edges(edges));
        } else if (mode == 3) {
            const int N = (int)r.one();
            std::vector<SlabAnchors> all;
            for (int k = 0; k < N; k++) {
                u64 v[13];
                for (u64& x : v) x = r.one();
                const AnchorInfo a{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9]};
                const SlabAnchors m = slab_anchors(a, k, N, v[10], v[11], v[12]);
                for (u64 x : {m.cols, m.eds_bytes, m.seds_bytes, m.ok, m.tail_col, m.tail_eds, m.tail_seds, m.head_end, m.head_eds, m.head_seds,
                              m.pad0, m.pad1}) w.one(x);
                all.push_back(m);
            }
            bool ok = false;
            const SlabStitch st = stitch_from_anchors(all, ok);
            w.one(ok);
            if (ok) put_stitch(w, st);
        } else if (mode == 4) {
            const u64 S = r.one(), np = r.one();
            std::vector<std::vector<uint8_t>> data;
            std::vector<std::pair<const uint8_t*, u64>> parts;
            for (u64 k = 0; k < np; k++) {
                const u64 ncols = r.one();
                data.push_back(r.blob());
                if (data.back().size() != S * ncols) { std::fprintf(stderr, "bad block\n"); return 2; }
            }
            for (const auto& d : data) parts.emplace_back(d.data(), d.size() / S);
            std::vector<uint8_t> mini(3, 'x');                   // (not empty: mini_image sizes it)
            mini_image(S, parts, mini);
            w.blob(mini);
        } else if (mode == 5) {
            const u64 stride = r.one();
            const int rank = (int)r.one();
            std::vector<u64> sizes(r.one());
            for (u64& x : sizes) x = r.one();
            u64 eoff = 1, soff = 2, etot = 3, stot = 4;
            piece_offsets(sizes, stride, rank, eoff, soff, etot, stot);
            w.one(eoff); w.one(soff); w.one(etot); w.one(stot);
        } else { std::fprintf(stderr, "bad mode\n"); return 2; }
    }
    w.out.close();
    std::printf("%zu cases\n", cases);
    return w.out ? 0 : 1;
}
