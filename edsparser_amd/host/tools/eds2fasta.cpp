// eds2fasta — spell the sequence of the paths of an EDS with sources as FASTA, on the GPU (edsx_paths_*).
// The inverse of msa2eds / vcf2eds: path s + 1 of msa2eds(A) is row s of A without its gaps.  Banner, "[Performance]"
// line and exit codes in the style of the other tools.  The paths are spelled in batches sized from their lengths
// (--batch-mb) and every batch is appended to the output file, so host memory stays bounded.
#include "edsx.h"
#include "../cli_util.hpp"
#include "../device.hpp"
#include "tool_common.hpp"

#include <memory>
#include <vector>

using namespace edsparser;

namespace {

struct Session {
    edsx_paths_session* s = nullptr;
    ~Session() { edsx_paths_close(s); }
};

} // namespace

int main(int argc, char** argv)
{
    Timer timer;
    timer.start();
    try {
        cli::Parser opts("Spell the paths of an EDS with sources as FASTA");
        opts.add("help", 'h', false, false, "Show help message");
        opts.add("input", 'i', true, true, "Input EDS file (.eds / .leds)");
        opts.add("sources", 's', true, false, "Input source file (default: <input> with the .seds extension)");
        opts.add("output", 'o', true, false, "Output FASTA file (default: <input stem>.fa)");
        opts.add("paths", 'p', true, false, "Path ids and ranges, e.g. 1,5,7-9 (default: all paths)");
        opts.add("line-width", 'w', true, false, "Characters per sequence line, 0 = one line (default: 60)");
        opts.add("names", 0, true, false, "File whose line k names path k (default: <prefix><id>)");
        opts.add("prefix", 0, true, false, "Record name prefix (default: path)");
        opts.add("batch-mb", 0, true, false, "FASTA megabytes spelled per batch (default: 4096)");
        opts.parse(argc, argv);
        if (opts.has("help")) {
            std::cout << "eds2fasta - spell the sequence of every path of an EDS\n\n" << opts.usage() << "\n"
                      << "A path takes, per symbol, the first string whose source set holds its id or 0.\n"
                         "Paths partition trivially: run one eds2fasta per GPU with disjoint -p ranges.\n\n"
                         "EXAMPLES:\n"
                         "  eds2fasta -i in.eds                       # in.seds -> in.fa, all paths\n"
                         "  eds2fasta -i in.eds -p 1,5,7-9 -w 80 -o some.fa\n\n";
            tool::print_performance(timer);
            return 0;
        }
        opts.notify();
        const std::filesystem::path input_file = opts.get("input");
        std::filesystem::path sources_file = opts.get("sources"), output_file = opts.get("output");
        if (sources_file.empty()) { sources_file = input_file; sources_file.replace_extension(".seds"); }
        if (output_file.empty()) output_file = input_file.parent_path() / (input_file.stem().string() + ".fa");
        const unsigned long line_width = opts.get_unsigned("line-width", 60);
        const unsigned long batch_mb = opts.get_unsigned("batch-mb", 4096);
        const std::string prefix = opts.get("prefix", "path");
        auto fail = [&](const std::string& msg) { std::cerr << "Error: " << msg << "\n"; tool::print_performance(timer); return 1; };
        if (batch_mb == 0) return fail("--batch-mb must be > 0");
        if (!std::filesystem::exists(input_file)) return fail("Input file does not exist: " + input_file.string());
        if (!std::filesystem::exists(sources_file)) return fail("Path spelling needs sources (.seds): " + sources_file.string() + " does not exist");
        std::vector<uint64_t> ids;
        if (opts.has("paths")) ids = tool::parse_paths(opts.get("paths"));

        std::cout << "EDS → FASTA path spelling\n";
        std::cout << "  Input: " << input_file << "\n";
        std::cout << "  Sources: " << sources_file << "\n";
        std::cout << "  Output: " << output_file << "\n";
        std::cout << "  Line width: " << line_width << "\n";

        edsx_ctx* ctx = detail::context();
        Session ses;
        {
            const tool::MappedFile eds(input_file, "input"), seds(sources_file, "sources");
            if (edsx_paths_open(ctx, eds.data(), eds.size(), seds.data(), seds.size(), &ses.s) != EDSX_OK)
                return fail(edsx_last_error(ctx));
        }
        edsx_paths_info_t info;
        edsx_paths_info(ses.s, &info);
        std::cout << "  Symbols: " << info.n_symbols << " (" << info.n_choice_symbols << " with a choice), strings: " << info.n_strings
                  << ", paths: " << info.num_paths << "\n";
        if (!opts.has("paths")) for (uint64_t p = 1; p <= info.num_paths; p++) ids.push_back(p);

        std::vector<std::string> all_names;
        if (opts.has("names")) {
            std::ifstream nf(opts.get("names"));
            if (!nf) return fail("Cannot open names file: " + opts.get("names"));
            for (std::string line; std::getline(nf, line);) {
                if (!line.empty() && line.back() == '\r') line.pop_back();
                all_names.push_back(line);
            }
        }
        std::vector<uint64_t> len(ids.size()), miss(ids.size());
        if (edsx_paths_lengths(ses.s, ids.data(), ids.size(), len.data(), miss.data()) != EDSX_OK) return fail(edsx_last_error(ctx));
        std::vector<const char*> names;
        if (opts.has("names")) {
            for (uint64_t p : ids) {
                if (p > all_names.size() || all_names[p - 1].empty())
                    return fail("The names file has no name for path " + std::to_string(p));
                names.push_back(all_names[p - 1].c_str());
            }
        }
        for (size_t k = 0; k < ids.size(); k++)
            if (miss[k]) std::cerr << "Warning: path " << ids[k] << " has no string in " << miss[k] << " symbols\n";

        std::ofstream out(output_file, std::ios::binary);
        if (!out) return fail("Cannot open output file: " + output_file.string());
        const uint64_t budget = static_cast<uint64_t>(batch_mb) << 20;
        uint64_t total = 0, batches = 0;
        for (size_t k0 = 0; k0 < ids.size();) {
            size_t k1 = k0;
            uint64_t bytes = 0;
            while (k1 < ids.size()) {                            // body + line feeds + a generous header
                const uint64_t rec = len[k1] + (line_width ? len[k1] / line_width : 0) + 2 + 64 + (names.empty() ? prefix.size() : std::string(names[k1]).size());
                if (k1 > k0 && bytes + rec > budget) break;
                bytes += rec;
                k1++;
            }
            detail::Buf fasta;
            if (edsx_paths_spell(ses.s, ids.data() + k0, k1 - k0, names.empty() ? nullptr : names.data() + k0, prefix.c_str(), line_width,
                                 &fasta.b, nullptr) != EDSX_OK)
                return fail(edsx_last_error(ctx));
            out.write(reinterpret_cast<const char*>(fasta.b.data), static_cast<std::streamsize>(fasta.b.size));
            if (!out) return fail("Cannot write output file: " + output_file.string());
            total += fasta.b.size;
            batches++;
            k0 = k1;
        }
        std::cout << "  Paths spelled: " << ids.size() << " in " << batches << (batches == 1 ? " batch" : " batches") << ", " << total
                  << " bytes\n";
        std::cout << "Spelling complete!\n";
        tool::print_performance(timer);
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "Error: " << e.what() << "\n";
        tool::print_performance(timer);
        return 1;
    }
}
