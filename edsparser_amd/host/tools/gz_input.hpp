// gz_input.hpp — compressed input files of the tools.  A file is probed by content (edsx_gz_probe).  BGZF goes to the
// library as it is and is inflated on the device; any other gzip file is inflated here, on this thread, with the
// decoder core the device kernel is compiled from - so a broken file is reported before any device work.
#pragma once
#include "edsx.h"
#include "../../csrc/inflate.hpp"
#include "tool_common.hpp"

#include <vector>

namespace tool {

struct GzInput {
    const uint8_t* data = nullptr;     // what the library gets: the mapped file (plain, BGZF) or `text` (gzip)
    size_t size = 0;
    int kind = 0;                      // of the file: 0 plain, 1 BGZF, 2 gzip
    uint64_t blocks = 0;
    std::vector<uint8_t> text;

    // what: "VCF", "FASTA" or "input" (the error texts); named_gz: the file name promises gzip
    GzInput(const MappedFile& f, const char* what, bool named_gz)
    {
        data = f.data(); size = f.size();
        if (edsx_gz_probe(f.data(), f.size(), &kind) != EDSX_OK) throw std::runtime_error("edsx_gz_probe failed");
        if (kind == 0) {
            if (named_gz) throw std::runtime_error(edsx::gz::gz_error_text(what, 0, 0, "not a gzip member"));
            return;
        }
        if (kind == 1) {
            unsigned long long n = 0;
            edsx::gz::gz_walk(f.data(), f.size(), n, [&](const edsx::gz::BgzfBlock&) { blocks++; });
            return;
        }
        std::string err;
        unsigned long long members = 0;
        if (!edsx::gz::gz_inflate_host(f.data(), f.size(), text, what, err, &members)) throw std::runtime_error(err);
        blocks = members;
        data = text.empty() ? reinterpret_cast<const uint8_t*>("") : text.data();
        size = text.size();
    }
    bool compressed() const { return kind != 0; }
    std::string describe() const
    {
        return kind == 0 ? "plain" : kind == 1 ? "BGZF, " + std::to_string(blocks) + " blocks" : "gzip (inflated on the host, one thread)";
    }
};

inline bool gz_extension(const std::filesystem::path& p) { return p.extension() == ".gz" || p.extension() == ".bgz"; }

} // namespace tool
