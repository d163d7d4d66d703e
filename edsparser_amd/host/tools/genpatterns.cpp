// edsparser-genpatterns — sample patterns from an EDS (benchmark queries for an index), on the GPU.
// Flags, messages and exit codes follow the reference tool (src/cpp/tools/genpatterns.cpp:36-41 options, :54-110
// validation and messages); the patterns come from edsx_eds_genpatterns, the bytes of EDS::generate_patterns with the
// same seed.  New: --seed (default from std::random_device, printed so that a run can be repeated) and --witness FILE
// (per pattern: its start common position, a tab and the chosen degenerate string numbers; "-" for a wrapped pattern).
#include "edsx.h"
#include "../cli_util.hpp"
#include "../device.hpp"
#include "tool_common.hpp"

#include <random>

using namespace edsparser;

int main(int argc, char** argv)
{
    Timer timer;
    timer.start();
    try {
        cli::Parser opts("Generate random patterns from EDS");
        opts.add("help", 'h', false, false, "Show help message");
        opts.add("input", 'i', true, true, "Input EDS file");
        opts.add("output", 'o', true, true, "Output pattern file");
        opts.add("count", 'n', true, false, "Number of patterns (default: 100)");
        opts.add("length", 'l', true, false, "Pattern length (default: 10)");
        opts.add("seed", 0, true, false, "Random seed (default: from std::random_device)");
        opts.add("witness", 0, true, false, "Also write each pattern's start position and degenerate string numbers");
        opts.parse(argc, argv);
        if (opts.has("help")) {
            std::cout << opts.usage() << "\n";
            tool::print_performance(timer);
            return 0;
        }
        opts.notify();
        const std::filesystem::path input_file = opts.get("input"), output_file = opts.get("output");
        const long count = opts.get_int("count", 100);
        const unsigned long length = opts.get_unsigned("length", 10);
        if (count < 0) throw std::runtime_error("the argument ('" + opts.get("count") + "') for option '--count' is invalid");
        uint64_t seed = 0;
        if (opts.has("seed")) {
            size_t used = 0;
            try { seed = std::stoull(opts.get("seed"), &used); } catch (...) { used = 0; }
            if (used != opts.get("seed").size() || opts.get("seed")[0] == '-')
                throw std::runtime_error("the argument ('" + opts.get("seed") + "') for option '--seed' is invalid");
        } else {
            std::random_device rd;
            seed = (static_cast<uint64_t>(rd()) << 32) ^ rd();
        }
        auto fail = [&](const std::string& msg) { std::cerr << "Error: " << msg << "\n"; tool::print_performance(timer); return 1; };
        if (!std::filesystem::exists(input_file)) {
            std::cerr << "Error: Input file does not exist: " << input_file << "\n";
            tool::print_performance(timer);
            return 1;
        }
        if (count == 0) return fail("Pattern count must be greater than 0");
        if (length == 0) return fail("Pattern length must be greater than 0");

        std::cerr << "Loading EDS file: " << input_file << "\n";
        std::cerr << "Seed: " << seed << "\n";
        const tool::MappedFile eds(input_file, "input");
        edsx_ctx* ctx = detail::context();
        const bool with_witness = opts.has("witness");
        detail::Buf pats, wpos, woff, wdeg;
        const int rc = edsx_eds_genpatterns(ctx, eds.data(), eds.size(), static_cast<uint64_t>(count), static_cast<uint32_t>(length),
                                            seed, &pats.b, with_witness ? &wpos.b : nullptr, with_witness ? &woff.b : nullptr,
                                            with_witness ? &wdeg.b : nullptr);
        if (rc != EDSX_OK) return fail(edsx_last_error(ctx));
        edsx_query_info info;
        edsx_query_last_info(ctx, &info);                      // the counts of the device tables
        std::cerr << "Loaded EDS with " << info.n_symbols << " symbols, " << info.n_strings << " strings\n";
        if (length > info.n_chars) {
            std::cerr << "Warning: Pattern length (" << length << ") is greater than total EDS size (" << info.n_chars << ")\n";
            std::cerr << "Patterns may be truncated or generation may fail\n";
        }
        {
            std::ofstream out(output_file, std::ios::binary);
            if (!out) return fail("Cannot open output file: \"" + output_file.string() + "\"");
            std::cerr << "Generating " << count << " patterns of length " << length << "...\n";
            out.write(reinterpret_cast<const char*>(pats.b.data), static_cast<std::streamsize>(pats.b.size));
        }
        if (with_witness) {
            const std::filesystem::path wfile = opts.get("witness");
            std::ofstream w(wfile, std::ios::binary);
            if (!w) return fail("Cannot open witness file: \"" + wfile.string() + "\"");
            const uint64_t* pos = reinterpret_cast<const uint64_t*>(wpos.b.data);
            const uint64_t* off = reinterpret_cast<const uint64_t*>(woff.b.data);
            const int32_t* deg = reinterpret_cast<const int32_t*>(wdeg.b.data);
            std::string line;
            for (long i = 0; i < count; i++) {
                if (pos[i] == UINT64_MAX) { w << "-\n"; continue; }
                line = std::to_string(pos[i]) + "\t";
                for (uint64_t k = off[i]; k < off[i + 1]; k++) {
                    if (k > off[i]) line += ',';
                    line += std::to_string(deg[k]);
                }
                line += '\n';
                w << line;
            }
        }
        std::cerr << "Successfully generated " << count << " patterns\n";
        std::cerr << "Output written to: " << output_file << "\n";
        tool::print_performance(timer);
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "Error: " << e.what() << "\n";
        tool::print_performance(timer);
        return 1;
    }
}
