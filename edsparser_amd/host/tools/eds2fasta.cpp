// eds2fasta — spell the sequence of the paths of an EDS with sources as FASTA, on the GPU (edsx_paths_*).
// The inverse of msa2eds / vcf2eds: path s + 1 of msa2eds(A) is row s of A without its gaps.  Banner, "[Performance]"
// line and exit codes in the style of the other tools.  The paths are spelled in batches sized from their lengths
// (--batch-mb) and every batch is appended to the output file, so host memory stays bounded.
#include "tool_front.hpp"

using namespace edsparser;

int main(int argc, char** argv)
{
    return tool::run([&] {
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
            return;
        }
        opts.notify();
        const tool::Files f = tool::files(opts, ".fa");
        const unsigned long line_width = opts.get_unsigned("line-width", 60);
        const unsigned long batch_mb = opts.get_unsigned("batch-mb", 4096);
        if (batch_mb == 0) tool::fail("--batch-mb must be > 0");
        tool::need_files(f);
        std::vector<uint64_t> ids = tool::path_list(opts, "paths");

        std::cout << "EDS → FASTA path spelling\n";
        std::cout << "  Input: " << f.input << "\n";
        std::cout << "  Sources: " << f.sources << "\n";
        std::cout << "  Output: " << f.output << "\n";
        std::cout << "  Line width: " << line_width << "\n";

        tool::Session ses(f);
        const edsx_paths_info_t& info = ses.info;
        std::cout << "  Symbols: " << info.n_symbols << " (" << info.n_choice_symbols << " with a choice), strings: " << info.n_strings
                  << ", paths: " << info.num_paths << "\n";
        if (ids.empty()) ids = tool::all_paths(info.num_paths);

        const tool::Names table(opts, "path");
        std::vector<uint64_t> len(ids.size()), miss(ids.size());
        ses.check(edsx_paths_lengths(ses.s, ids.data(), ids.size(), len.data(), miss.data()));   // the library checks the ids
        std::vector<std::string> name_text;
        if (table.given) name_text = table.names_of(ids);
        const std::vector<const char*> names = tool::c_strs(name_text);
        for (size_t k = 0; k < ids.size(); k++)
            if (miss[k]) std::cerr << "Warning: path " << ids[k] << " has no string in " << miss[k] << " symbols\n";

        std::ofstream out(f.output, std::ios::binary);
        if (!out) tool::fail("Cannot open output file: " + f.output.string());
        const uint64_t budget = static_cast<uint64_t>(batch_mb) << 20;
        uint64_t total = 0, batches = 0;
        for (size_t k0 = 0; k0 < ids.size();) {
            size_t k1 = k0;
            uint64_t bytes = 0;
            while (k1 < ids.size()) {                            // body + line feeds + a generous header
                const uint64_t rec = len[k1] + (line_width ? len[k1] / line_width : 0) + 2 + 64 + (names.empty() ? table.prefix.size() : name_text[k1].size());
                if (k1 > k0 && bytes + rec > budget) break;
                bytes += rec;
                k1++;
            }
            detail::Buf fasta;
            ses.check(edsx_paths_spell(ses.s, ids.data() + k0, k1 - k0, names.empty() ? nullptr : names.data() + k0, table.prefix.c_str(), line_width,
                                       &fasta.b, nullptr));
            out.write(reinterpret_cast<const char*>(fasta.b.data), static_cast<std::streamsize>(fasta.b.size));
            if (!out) tool::fail("Cannot write output file: " + f.output.string());
            total += fasta.b.size;
            batches++;
            k0 = k1;
        }
        std::cout << "  Paths spelled: " << ids.size() << " in " << batches << (batches == 1 ? " batch" : " batches") << ", " << total
                  << " bytes\n";
        std::cout << "Spelling complete!\n";
    });
}
