// edsparser-dist — pairwise distances between the paths of an EDS with sources, on the GPU (edsx_paths_distances): the
// matrix a tree builder, a duplicate check or a nearest-neighbour search would otherwise compute from the rows eds2msa
// writes.  --metric columns: the alignment columns at which two rows differ ("no character" is a value of its own, there
// is no gap parameter); --metric strings: the symbols at which two paths take different strings.  --normalize divides by
// the number of columns (or symbols).  The text is written on the host:
//   tsv      "path\t<name_1>...\t<name_K>", then per row "<name>\t<d_1>...\t<d_K>"
//   phylip   "K", then per row the name and the K values separated by single blanks
// Rows are named <prefix><id - 1>, as eds2msa names them, or by line id of --names.  Banner, "[Performance]" line and exit
// codes in the style of the other tools.
#include "edsx.h"
#include "../cli_util.hpp"
#include "../device.hpp"
#include "tool_common.hpp"

#include <cstdio>
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
            tool::print_performance(timer);
            return 0;
        }
        opts.notify();
        const std::filesystem::path input_file = opts.get("input");
        std::filesystem::path sources_file = opts.get("sources"), output_file = opts.get("output");
        if (sources_file.empty()) { sources_file = input_file; sources_file.replace_extension(".seds"); }
        if (output_file.empty()) output_file = input_file.parent_path() / (input_file.stem().string() + ".dist");
        const unsigned long max_mb = opts.get_unsigned("max-mb", 0);
        const std::string prefix = opts.get("prefix", "s"), metric_text = opts.get("metric", "columns"), format = opts.get("format", "tsv");
        const bool normalize = opts.has("normalize");
        auto fail = [&](const std::string& msg) { std::cerr << "Error: " << msg << "\n"; tool::print_performance(timer); return 1; };
        if (metric_text != "columns" && metric_text != "strings")
            return fail("the argument ('" + metric_text + "') for option '--metric' is invalid");
        if (format != "tsv" && format != "phylip") return fail("the argument ('" + format + "') for option '--format' is invalid");
        const int metric = metric_text == "columns" ? EDSX_DIST_COLUMNS : EDSX_DIST_STRINGS;
        if (!std::filesystem::exists(input_file)) return fail("Input file does not exist: " + input_file.string());
        if (!std::filesystem::exists(sources_file)) return fail("Path spelling needs sources (.seds): " + sources_file.string() + " does not exist");
        std::vector<uint64_t> ids;
        if (opts.has("paths")) ids = tool::parse_paths(opts.get("paths"));

        std::cout << "EDS path distances\n";
        std::cout << "  Input: " << input_file << "\n";
        std::cout << "  Sources: " << sources_file << "\n";
        std::cout << "  Output: " << output_file << "\n";
        std::cout << "  Metric: " << metric_text << (normalize ? ", normalized" : "") << ", format: " << format << "\n";

        edsx_ctx* ctx = detail::context();
        Session ses;
        {
            const tool::MappedFile eds(input_file, "input"), seds(sources_file, "sources");
            if (edsx_paths_open(ctx, eds.data(), eds.size(), seds.data(), seds.size(), &ses.s) != EDSX_OK)
                return fail(edsx_last_error(ctx));
        }
        edsx_paths_info_t pi;
        edsx_paths_info(ses.s, &pi);
        if (!opts.has("paths")) for (uint64_t p = 1; p <= pi.num_paths; p++) ids.push_back(p);
        for (uint64_t p : ids)                                   // before the output file is created
            if (p == 0 || p > pi.num_paths)
                return fail("Path id " + std::to_string(p) + " out of range (1.." + std::to_string(pi.num_paths) + ")");
        const size_t K = ids.size();

        std::vector<std::string> all_names;
        if (opts.has("names")) {
            std::ifstream nf(opts.get("names"));
            if (!nf) return fail("Cannot open names file: " + opts.get("names"));
            for (std::string line; std::getline(nf, line);) {
                if (!line.empty() && line.back() == '\r') line.pop_back();
                all_names.push_back(line);
            }
        }
        std::vector<std::string> name;
        for (uint64_t p : ids) {
            if (!opts.has("names")) name.push_back(prefix + std::to_string(p - 1));
            else if (p > all_names.size()) return fail("The names file has no name for path " + std::to_string(p));
            else name.push_back(all_names[p - 1]);
            if (name.back().empty() || name.back().find_first_of("\t \n") != std::string::npos)
                return fail("The name of path " + std::to_string(p) + " is empty or holds a tab, blank or line feed");
        }

        uint64_t bytes = 0;
        const bool wraps = __builtin_mul_overflow(static_cast<uint64_t>(K), static_cast<uint64_t>(K), &bytes) ||
                           __builtin_mul_overflow(bytes, static_cast<uint64_t>(8), &bytes);
        if (wraps) bytes = ~0ull;
        const uint64_t cap = static_cast<uint64_t>(max_mb) << 20;
        if (wraps || (cap && bytes > cap))
            return fail("Distance matrix has " + std::string(wraps ? "more than " : "") + std::to_string(bytes >> 20) +
                        " megabytes, above the limit of " + std::to_string(max_mb) + " (--max-mb)");
        std::vector<uint64_t> matrix(K * K), miss(K);
        edsx_dist_info di;
        if (K && edsx_paths_distances(ses.s, ids.data(), K, metric, cap, matrix.data(), miss.data(), &di) != EDSX_OK)
            return fail(edsx_last_error(ctx));
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
        tool::write_bytes(output_file, reinterpret_cast<const uint8_t*>(text.data()), text.size(), "output");
        edsx_paths_timing t;
        edsx_paths_last_timing(ses.s, &t);
        std::cout << "  Device: tables " << t.choose_ms << " ms, class list " << t.scan_ms << " ms, rows and pairs " << t.copy_ms << " ms\n";
        std::cout << "  Matrix written: " << K << " x " << K << ", " << text.size() << " bytes\n";
        std::cout << "Distances complete!\n";
        tool::print_performance(timer);
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "Error: " << e.what() << "\n";
        tool::print_performance(timer);
        return 1;
    }
}
