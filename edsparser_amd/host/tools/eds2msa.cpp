// eds2msa — write the paths of an EDS with sources as the rows of one alignment (aligned FASTA), on the GPU
// (edsx_paths_align).  The view msa2eds reads: every symbol owns as many columns as its longest string has characters, a
// row holds the path's strings left-justified there and the gap character elsewhere.  Banner, "[Performance]" line and
// exit codes in the style of the other tools.  The rows are written in batches (--batch-mb) and every batch is appended
// to the output file, so host memory stays bounded.
#include "tool_front.hpp"

using namespace edsparser;

int main(int argc, char** argv)
{
    return tool::run([&] {
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
            return;
        }
        opts.notify();
        const tool::Files f = tool::files(opts, ".msa");
        const unsigned long line_width = opts.get_unsigned("line-width", 0);
        const unsigned long batch_mb = opts.get_unsigned("batch-mb", 4096);
        const unsigned long max_mb = opts.get_unsigned("max-mb", 0);
        const std::string gap_text = opts.get("gap", "-");
        if (batch_mb == 0) tool::fail("--batch-mb must be > 0");
        if (gap_text.size() != 1) tool::fail("--gap takes one character");
        const int gap = static_cast<unsigned char>(gap_text[0]);
        if (gap == 0 || std::string(">\n\r {},").find(gap_text[0]) != std::string::npos) tool::fail("Gap character is not usable in an alignment");
        tool::need_files(f);
        std::vector<uint64_t> ids = tool::path_list(opts, "paths");

        std::cout << "EDS → MSA alignment export\n";
        std::cout << "  Input: " << f.input << "\n";
        std::cout << "  Sources: " << f.sources << "\n";
        std::cout << "  Output: " << f.output << "\n";
        std::cout << "  Line width: " << line_width << "\n";

        tool::Session ses(f);
        edsx_align_info info;
        ses.check(edsx_paths_align_info(ses.s, &info));
        std::cout << "  Symbols: " << info.n_symbols << " (" << info.n_zero_width_symbols << " without a column, the widest "
                  << info.widest_symbol << "), columns: " << info.n_columns << ", paths: " << info.num_paths << "\n";
        tool::resolve_paths(ids, info.num_paths);                // before the output file is created

        // the row names: the headers msa2eds inputs carry here count from 0, the path ids from 1
        const std::vector<std::string> name_text = tool::Names(opts, "s").names_of(ids);
        const std::vector<const char*> names = tool::c_strs(name_text);

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
            tool::fail("Alignment has " + std::string(wraps ? "more than " : "") + std::to_string(whole >> 20) + " megabytes, above the limit of " +
                       std::to_string(max_mb) + " (--max-mb)");

        std::ofstream out(f.output, std::ios::binary);
        if (!out) tool::fail("Cannot open output file: " + f.output.string());
        const uint64_t budget = static_cast<uint64_t>(batch_mb) << 20;
        uint64_t total = 0, batches = 0;
        std::vector<uint64_t> miss;
        for (size_t k0 = 0; k0 < ids.size();) {
            size_t k1 = k0;
            uint64_t bytes = 0;
            while (k1 < ids.size() && (k1 == k0 || bytes + rec[k1] <= budget)) bytes += rec[k1++];
            detail::Buf fasta;
            miss.assign(k1 - k0, 0);
            ses.check(edsx_paths_align(ses.s, ids.data() + k0, k1 - k0, names.data() + k0, nullptr, line_width, gap, 0, &fasta.b, miss.data()));
            out.write(reinterpret_cast<const char*>(fasta.b.data), static_cast<std::streamsize>(fasta.b.size));
            if (!out) tool::fail("Cannot write output file: " + f.output.string());
            for (size_t k = k0; k < k1; k++)
                if (miss[k - k0]) std::cerr << "Warning: path " << ids[k] << " has no string in " << miss[k - k0] << " symbols\n";
            total += fasta.b.size;
            batches++;
            k0 = k1;
        }
        std::cout << "  Rows written: " << ids.size() << " in " << batches << (batches == 1 ? " batch" : " batches") << ", " << total
                  << " bytes\n";
        std::cout << "Alignment complete!\n";
    });
}
