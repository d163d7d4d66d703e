// edsparser-locate — find every occurrence of patterns in an EDS (+ .seds), on the GPU (edsx_eds_locate).
// The pattern file is what edsparser-genpatterns writes: one pattern per line.  Output is TSV, one hit per line:
//   pattern  common_pos  symbol  string_in_symbol  offset  choices
// pattern is 0-based, common_pos is "-" for a start inside a degenerate symbol, choices are the degenerate string numbers,
// comma-separated: columns 2 and 6 of a common-start line are a --witness line of edsparser-genpatterns, and what
// EDS::check_position takes.  --count-only writes "pattern  total  flags" instead (flags: 1 hits left out, 2 a walk cut
// at its 65th choice).  Argument and pattern-file errors are reported before a context is created.
#include "tool_front.hpp"

using namespace edsparser;

int main(int argc, char** argv)
{
    return tool::run([&] {
        cli::Parser opts("Locate patterns in EDS");
        opts.add("help", 'h', false, false, "Show help message");
        opts.add("input", 'i', true, true, "Input EDS file");
        opts.add("sources", 's', true, false, "Input sEDS file (the strings of a hit must share a path)");
        opts.add("patterns", 'p', true, true, "Pattern file, one pattern per line");
        opts.add("output", 'o', true, true, "Output TSV file");
        opts.add("max-hits", 0, true, false, "Hits reported per pattern (default: 1024)");
        opts.add("common-only", 0, false, false, "Only starts in common symbols (the domain of check_position)");
        opts.add("count-only", 0, false, false, "Write pattern, total and flags instead of the hits");
        opts.parse(argc, argv);
        if (opts.has("help")) {
            std::cout << opts.usage() << "\n";
            return;
        }
        opts.notify();
        const std::filesystem::path input_file = opts.get("input"), pattern_file = opts.get("patterns"), output_file = opts.get("output");
        uint64_t max_hits = 1024;
        if (opts.has("max-hits")) {
            const std::string v = opts.get("max-hits");
            size_t used = 0;
            try { max_hits = std::stoull(v, &used); } catch (...) { used = 0; }
            if (used != v.size() || v[0] == '-') throw std::runtime_error("the argument ('" + v + "') for option '--max-hits' is invalid");
        }
        if (max_hits == 0) tool::fail("--max-hits must be at least 1");
        if (!std::filesystem::exists(input_file)) tool::fail("Input file does not exist: \"" + input_file.string() + "\"");
        if (opts.has("sources") && !std::filesystem::exists(opts.get("sources")))
            tool::fail("Sources file does not exist: \"" + opts.get("sources") + "\"");
        if (!std::filesystem::exists(pattern_file)) tool::fail("Pattern file does not exist: \"" + pattern_file.string() + "\"");

        // the patterns as CSR: a trailing '\r' is dropped, a missing final newline is fine, an empty line is an error
        std::string text;
        std::vector<uint64_t> off(1, 0);
        {
            std::ifstream in(pattern_file, std::ios::binary);
            if (!in) tool::fail("Cannot open pattern file: \"" + pattern_file.string() + "\"");
            const std::string raw = detail::slurp(in);
            size_t line = 1;
            for (size_t b = 0; b < raw.size(); line++) {
                size_t e = raw.find('\n', b);
                if (e == std::string::npos) e = raw.size();
                size_t len = e - b;
                if (len && raw[b + len - 1] == '\r') len--;
                if (len == 0) tool::fail("Pattern file line " + std::to_string(line) + " is empty");
                text.append(raw, b, len);
                off.push_back(text.size());
                b = e + 1;
            }
        }
        const size_t n = off.size() - 1;

        std::cerr << "Loading EDS file: " << input_file << "\n";
        const tool::MappedFile eds(input_file, "input");
        std::unique_ptr<tool::MappedFile> seds;
        if (opts.has("sources")) seds.reset(new tool::MappedFile(opts.get("sources"), "sources"));
        edsx_ctx* ctx = detail::context();
        detail::Buf hoff, hits, coff, ch, totals, flags;
        std::cerr << "Locating " << n << " patterns...\n";
        const int rc = edsx_eds_locate(ctx, eds.data(), eds.size(), seds ? seds->data() : nullptr, seds ? seds->size() : 0, n, off.data(),
                                       reinterpret_cast<const uint8_t*>(text.data()), max_hits,
                                       opts.has("common-only") ? EDSX_LOCATE_COMMON_ONLY : 0u, &hoff.b, &hits.b, &coff.b, &ch.b,
                                       &totals.b, &flags.b);
        tool::check(ctx, rc);
        edsx_query_info info;
        edsx_query_last_info(ctx, &info);
        std::cerr << "Loaded EDS with " << info.n_symbols << " symbols, " << info.n_strings << " strings\n";
        const uint64_t* ho = reinterpret_cast<const uint64_t*>(hoff.b.data);
        const edsx_locate_hit* hit = reinterpret_cast<const edsx_locate_hit*>(hits.b.data);
        const uint64_t* co = reinterpret_cast<const uint64_t*>(coff.b.data);
        const int32_t* deg = reinterpret_cast<const int32_t*>(ch.b.data);
        const uint64_t* tot = reinterpret_cast<const uint64_t*>(totals.b.data);
        const uint8_t* fl = flags.b.data;
        size_t truncated = 0;
        for (size_t q = 0; q < n; q++) truncated += fl[q] != 0;
        {
            std::ofstream out(output_file, std::ios::binary);
            if (!out) tool::fail("Cannot open output file: \"" + output_file.string() + "\"");
            std::string buf;
            for (size_t q = 0; q < n; q++) {
                if (opts.has("count-only")) {
                    buf += std::to_string(q) + "\t" + std::to_string(tot[q]) + "\t" + std::to_string(fl[q]) + "\n";
                } else {
                    for (uint64_t h = ho[q]; h < ho[q + 1]; h++) {
                        buf += std::to_string(q) + "\t" + (hit[h].common_pos == UINT64_MAX ? std::string("-") : std::to_string(hit[h].common_pos)) +
                               "\t" + std::to_string(hit[h].symbol) + "\t" + std::to_string(hit[h].string) + "\t" +
                               std::to_string(hit[h].offset) + "\t";
                        for (uint64_t k = co[h]; k < co[h + 1]; k++) {
                            if (k > co[h]) buf += ',';
                            buf += std::to_string(deg[k]);
                        }
                        buf += '\n';
                    }
                }
                if (buf.size() >= (1u << 20)) { out.write(buf.data(), static_cast<std::streamsize>(buf.size())); buf.clear(); }
            }
            out.write(buf.data(), static_cast<std::streamsize>(buf.size()));
        }
        std::cerr << "Patterns: " << n << ", hits: " << ho[n] << ", truncated patterns: " << truncated << "\n";
        std::cerr << "Device: tokenise " << info.tokenise_ms << " ms, tables " << info.tables_ms << " ms, kernels " << info.kernel_ms
                  << " ms, download " << info.download_ms << " ms\n";
        std::cerr << "Output written to: " << output_file << "\n";
    });
}
