// eds2msa — write the paths of an EDS with sources as the rows of one alignment (aligned FASTA), on the GPU
// (edsx_paths_align).  The view msa2eds reads: every symbol owns as many columns as its longest string has characters, a
// row holds the path's strings left-justified there and the gap character elsewhere.  Banner, "[Performance]" line and
// exit codes in the style of the other tools.  The rows are written in batches (--batch-mb) and every batch is appended
// to the output file, so host memory stays bounded.
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
        cli::Parser opts("Write the paths of an EDS with sources as an aligned FASTA");
        opts.add("help", 'h', false, false, "Show help message");
        opts.add("input", 'i', true, true, "Input EDS file (.eds / .leds)");
        opts.add("sources", 's', true, false, "Input source file (default: <input> with the .seds extension)");
        opts.add("output", 'o', true, false, "Output alignment file (default: <input stem>.msa)");
        opts.add("paths", 'p', true, false, "Path ids and ranges, e.g. 1,5,7-9 (default: all paths)");
        opts.add("line-width", 'w', true, false, "Characters per line, 0 = one line per row (default: 0)");
        opts.add("names", 0, true, false, "File whose line k names path k (default: <prefix><id - 1>)");
        opts.add("prefix", 0, true, false, "Row name prefix (default: s)");
        opts.add("gap", 0, true, false, "Gap character (default: -)");
        opts.add("max-mb", 0, true, false, "Refuse an alignment above this many megabytes, 0 = no limit (default: 0)");
        opts.add("batch-mb", 0, true, false, "Alignment megabytes written per batch (default: 4096)");
        opts.parse(argc, argv);
        if (opts.has("help")) {
            std::cout << "eds2msa - write the paths of an EDS as the rows of one alignment\n\n" << opts.usage() << "\n"
                      << "A symbol owns as many columns as its longest string has characters; a row holds, per symbol, the\n"
                         "first string whose source set holds the path's id or 0, left-justified, and gaps elsewhere.\n"
                         "The columns do not depend on -p: run one eds2msa per GPU with disjoint -p ranges and\n"
                         "concatenate the files.  Rows are named <prefix>0, <prefix>1, ... for paths 1, 2, ...\n\n"
                         "EXAMPLES:\n"
                         "  eds2msa -i in.eds                         # in.seds -> in.msa, all paths\n"
                         "  eds2msa -i in.eds -p 1-32 -w 60 --gap . -o part1.msa\n\n";
            tool::print_performance(timer);
            return 0;
        }
        opts.notify();
        const std::filesystem::path input_file = opts.get("input");
        std::filesystem::path sources_file = opts.get("sources"), output_file = opts.get("output");
        if (sources_file.empty()) { sources_file = input_file; sources_file.replace_extension(".seds"); }
        if (output_file.empty()) output_file = input_file.parent_path() / (input_file.stem().string() + ".msa");
        const unsigned long line_width = opts.get_unsigned("line-width", 0);
        const unsigned long batch_mb = opts.get_unsigned("batch-mb", 4096);
        const unsigned long max_mb = opts.get_unsigned("max-mb", 0);
        const std::string prefix = opts.get("prefix", "s"), gap_text = opts.get("gap", "-");
        auto fail = [&](const std::string& msg) { std::cerr << "Error: " << msg << "\n"; tool::print_performance(timer); return 1; };
        if (batch_mb == 0) return fail("--batch-mb must be > 0");
        if (gap_text.size() != 1) return fail("--gap takes one character");
        const int gap = static_cast<unsigned char>(gap_text[0]);
        if (gap == 0 || std::string(">\n\r {},").find(gap_text[0]) != std::string::npos)
            return fail("Gap character is not usable in an alignment");
        if (!std::filesystem::exists(input_file)) return fail("Input file does not exist: " + input_file.string());
        if (!std::filesystem::exists(sources_file)) return fail("Path spelling needs sources (.seds): " + sources_file.string() + " does not exist");
        std::vector<uint64_t> ids;
        if (opts.has("paths")) ids = tool::parse_paths(opts.get("paths"));

        std::cout << "EDS → MSA alignment export\n";
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
        edsx_align_info info;
        if (edsx_paths_align_info(ses.s, &info) != EDSX_OK) return fail(edsx_last_error(ctx));
        std::cout << "  Symbols: " << info.n_symbols << " (" << info.n_zero_width_symbols << " without a column, the widest "
                  << info.widest_symbol << "), columns: " << info.n_columns << ", paths: " << info.num_paths << "\n";
        if (!opts.has("paths")) for (uint64_t p = 1; p <= info.num_paths; p++) ids.push_back(p);
        for (uint64_t p : ids)                                   // before the output file is created
            if (p == 0 || p > info.num_paths)
                return fail("Path id " + std::to_string(p) + " out of range (1.." + std::to_string(info.num_paths) + ")");

        std::vector<std::string> all_names;
        if (opts.has("names")) {
            std::ifstream nf(opts.get("names"));
            if (!nf) return fail("Cannot open names file: " + opts.get("names"));
            for (std::string line; std::getline(nf, line);) {
                if (!line.empty() && line.back() == '\r') line.pop_back();
                all_names.push_back(line);
            }
        }
        // the row names: the headers msa2eds inputs carry here count from 0, the path ids from 1
        std::vector<std::string> name_text;
        for (uint64_t p : ids) {
            if (!opts.has("names")) { name_text.push_back(prefix + std::to_string(p - 1)); continue; }
            if (p == 0 || p > all_names.size() || all_names[p - 1].empty())
                return fail("The names file has no name for path " + std::to_string(p));
            name_text.push_back(all_names[p - 1]);
        }
        std::vector<const char*> names;
        for (const auto& t : name_text) names.push_back(t.c_str());

        // every row has the same body: the size of the file is known before a byte of it is made
        const uint64_t W = info.n_columns, lw = (line_width == 0 || line_width > W) ? std::max<uint64_t>(W, 1) : line_width;
        const uint64_t body = W ? W + (W + lw - 1) / lw : 0;
        std::vector<uint64_t> rec(ids.size());
        uint64_t whole = 0;
        bool wraps = false;
        for (size_t k = 0; k < ids.size(); k++) {
            rec[k] = name_text[k].size() + 2 + body;
            wraps |= __builtin_add_overflow(whole, rec[k], &whole);
        }
        if (wraps) whole = ~0ull;
        const uint64_t cap = static_cast<uint64_t>(max_mb) << 20;
        if (wraps || (cap && whole > cap))
            return fail("Alignment has " + std::string(wraps ? "more than " : "") + std::to_string(whole >> 20) + " megabytes, above the limit of " +
                        std::to_string(max_mb) + " (--max-mb)");

        std::ofstream out(output_file, std::ios::binary);
        if (!out) return fail("Cannot open output file: " + output_file.string());
        const uint64_t budget = static_cast<uint64_t>(batch_mb) << 20;
        uint64_t total = 0, batches = 0;
        std::vector<uint64_t> miss;
        for (size_t k0 = 0; k0 < ids.size();) {
            size_t k1 = k0;
            uint64_t bytes = 0;
            while (k1 < ids.size() && (k1 == k0 || bytes + rec[k1] <= budget)) bytes += rec[k1++];
            detail::Buf fasta;
            miss.assign(k1 - k0, 0);
            if (edsx_paths_align(ses.s, ids.data() + k0, k1 - k0, names.data() + k0, nullptr, line_width, gap, 0, &fasta.b,
                                 miss.data()) != EDSX_OK)
                return fail(edsx_last_error(ctx));
            out.write(reinterpret_cast<const char*>(fasta.b.data), static_cast<std::streamsize>(fasta.b.size));
            if (!out) return fail("Cannot write output file: " + output_file.string());
            for (size_t k = k0; k < k1; k++)
                if (miss[k - k0]) std::cerr << "Warning: path " << ids[k] << " has no string in " << miss[k - k0] << " symbols\n";
            total += fasta.b.size;
            batches++;
            k0 = k1;
        }
        std::cout << "  Rows written: " << ids.size() << " in " << batches << (batches == 1 ? " batch" : " batches") << ", " << total
                  << " bytes\n";
        std::cout << "Alignment complete!\n";
        tool::print_performance(timer);
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "Error: " << e.what() << "\n";
        tool::print_performance(timer);
        return 1;
    }
}
