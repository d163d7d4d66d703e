// edsparser-dist — pairwise distances between the paths of an EDS with sources, on the GPU (edsx_paths_distances): the
// matrix a tree builder, a duplicate check or a nearest-neighbour search would otherwise compute from the rows eds2msa
// writes.  --metric columns: the alignment columns at which two rows differ ("no character" is a value of its own, there
// is no gap parameter); --metric strings: the symbols at which two paths take different strings.  --normalize divides by
// the number of columns (or symbols).  The text is written on the host:
//   tsv      "path\t<name_1>...\t<name_K>", then per row "<name>\t<d_1>...\t<d_K>"
//   phylip   "K", then per row the name and the K values separated by single blanks
// Rows are named <prefix><id - 1>, as eds2msa names them, or by line id of --names.  Banner, "[Performance]" line and exit
// codes in the style of the other tools.
#include "tool_front.hpp"

#include <cstdio>
#include <vector>

using namespace edsparser;

int main(int argc, char** argv)
{
    return tool::run([&] {
        cli::Parser opts("Pairwise distances between the paths of an EDS with sources");
        opts.add("help", 'h', false, false, "Show help message");
        opts.add("input", 'i', true, true, "Input EDS file (.eds / .leds)");
        opts.add("sources", 's', true, false, "Input source file (default: <input> with the .seds extension)");
        opts.add("output", 'o', true, false, "Output matrix file (default: <input stem>.dist)");
        opts.add("paths", 'p', true, false, "Path ids and ranges, e.g. 1,5,7-9 (default: all paths)");
        opts.add("metric", 0, true, false, "columns or strings (default: columns)");
        opts.add("normalize", 0, false, false, "Divide by the number of alignment columns (strings: of symbols)");
        opts.add("format", 0, true, false, "tsv or phylip (default: tsv)");
        opts.add("names", 0, true, false, "File whose line k names path k (default: <prefix><id - 1>)");
        opts.add("prefix", 0, true, false, "Row name prefix (default: s)");
        opts.add("max-mb", 0, true, false, "Refuse a matrix above this many megabytes, 0 = no limit (default: 0)");
        opts.parse(argc, argv);
        if (opts.has("help")) {
            std::cout << "edsparser-dist - pairwise distances between the paths of an EDS\n\n" << opts.usage() << "\n"
                      << "columns: the columns of the alignment eds2msa writes at which two rows differ; a column where a\n"
                         "path has no character differs from every character and equals itself.  strings: the symbols at\n"
                         "which two paths take different strings.  Rows are named <prefix>0, <prefix>1, ... for paths 1, 2, ...\n\n"
                         "EXAMPLES:\n"
                         "  edsparser-dist -i in.eds                                  # in.seds -> in.dist, all paths, tsv\n"
                         "  edsparser-dist -i in.eds -p 1-32 --normalize --format phylip -o tree.phy\n\n";
            return;
        }
        opts.notify();
        const tool::Files f = tool::files(opts, ".dist");
        const unsigned long max_mb = opts.get_unsigned("max-mb", 0);
        const std::string metric_text = opts.get("metric", "columns"), format = opts.get("format", "tsv");
        const bool normalize = opts.has("normalize");
        if (metric_text != "columns" && metric_text != "strings")
            tool::fail("the argument ('" + metric_text + "') for option '--metric' is invalid");
        if (format != "tsv" && format != "phylip") tool::fail("the argument ('" + format + "') for option '--format' is invalid");
        const int metric = metric_text == "columns" ? EDSX_DIST_COLUMNS : EDSX_DIST_STRINGS;
        tool::need_files(f);
        std::vector<uint64_t> ids = tool::path_list(opts, "paths");

        std::cout << "EDS path distances\n";
        std::cout << "  Input: " << f.input << "\n";
        std::cout << "  Sources: " << f.sources << "\n";
        std::cout << "  Output: " << f.output << "\n";
        std::cout << "  Metric: " << metric_text << (normalize ? ", normalized" : "") << ", format: " << format << "\n";

        tool::Session ses(f);
        const edsx_paths_info_t& pi = ses.info;
        tool::resolve_paths(ids, pi.num_paths);                  // before the output file is created
        const size_t K = ids.size();

        const std::vector<std::string> name = tool::Names(opts, "s").names_of(ids, true);

        uint64_t bytes = 0;
        const bool wraps = __builtin_mul_overflow(static_cast<uint64_t>(K), static_cast<uint64_t>(K), &bytes) ||
                           __builtin_mul_overflow(bytes, static_cast<uint64_t>(8), &bytes);
        if (wraps) bytes = ~0ull;
        const uint64_t cap = static_cast<uint64_t>(max_mb) << 20;
        if (wraps || (cap && bytes > cap))
            tool::fail("Distance matrix has " + std::string(wraps ? "more than " : "") + std::to_string(bytes >> 20) +
                        " megabytes, above the limit of " + std::to_string(max_mb) + " (--max-mb)");
        std::vector<uint64_t> matrix(K * K), miss(K);
        edsx_dist_info di;
        if (K) ses.check(edsx_paths_distances(ses.s, ids.data(), K, metric, cap, matrix.data(), miss.data(), &di));
        if (!K) di = edsx_dist_info{0, 0, 0, 0, 0};
        for (size_t k = 0; k < K; k++)
            if (miss[k]) std::cerr << "Warning: path " << ids[k] << " has no string in " << miss[k] << " symbols\n";
        std::cout << "  Paths: " << K << " of " << pi.num_paths << ", units: " << di.units << " (" << di.variable_units << " variable), class columns: "
                  << di.class_columns << " in " << di.chunks << (di.chunks == 1 ? " chunk" : " chunks") << "\n";

        std::string text;
        const bool tsv = format == "tsv";
        const char sep = tsv ? '\t' : ' ';
        if (tsv) { text = "path"; for (const auto& nm : name) { text += '\t'; text += nm; } text += '\n'; }
        else text = std::to_string(K) + "\n";
        char cell[64];
        for (size_t a = 0; a < K; a++) {
            text += name[a];
            for (size_t b = 0; b < K; b++) {
                const uint64_t d = matrix[a * K + b];
                if (normalize) std::snprintf(cell, sizeof(cell), "%.6f", di.units ? static_cast<double>(d) / static_cast<double>(di.units) : 0.0);
                else std::snprintf(cell, sizeof(cell), "%llu", static_cast<unsigned long long>(d));
                text += sep;
                text += cell;
            }
            text += '\n';
        }
        tool::write_bytes(f.output, reinterpret_cast<const uint8_t*>(text.data()), text.size(), "output");
        edsx_paths_timing t;
        edsx_paths_last_timing(ses.s, &t);
        std::cout << "  Device: tables " << t.choose_ms << " ms, class list " << t.scan_ms << " ms, rows and pairs " << t.copy_ms << " ms\n";
        std::cout << "  Matrix written: " << K << " x " << K << ", " << text.size() << " bytes\n";
        std::cout << "Distances complete!\n";
    });
}
