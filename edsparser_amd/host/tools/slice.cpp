// edsparser-slice — cut regions out of an EDS with sources, on the GPU (edsx_paths_slice): every region becomes an .eds +
// .seds of its own that holds the symbols of the region, the two edge symbols cut at the alignment column, and the source
// set of every string.  Regions (slice_args.hpp) come from -r PATH:START-END and --columns START-END, both repeatable, and
// from --bed FILE (BED3+; column 1 names the path, column 4, if present, the output); positions count from 0, END is
// exclusive.  A path is named by its id or by --prefix + id.
//   -o OUT.eds        one region: OUT.eds, and the sources next to it with the .seds extension
//   --output-dir DIR  <name>.eds / <name>.seds per region; the default name is <path>_<start>_<end> or cols_<start>_<end>
//   --table           one line per region on standard output:
//                     name symbol_first symbol_last cut_first cut_end column_first column_end strings chars eds_bytes seds_bytes status
// A region that is empty or leaves its path is RANGE: it writes no file and is reported on standard error; the exit status
// is non-zero only when the call fails.  Argument and BED errors are reported before a context is created.
#include "slice_args.hpp"
#include "tool_front.hpp"

using namespace edsparser;

namespace {

std::string num(uint64_t v) { return v == UINT64_MAX ? std::string(".") : std::to_string(v); }

} // namespace

int main(int argc, char** argv)
{
    return tool::run([&] {
        cli::Parser opts("Cut regions out of an EDS by path or column coordinates");
        opts.add("help", 'h', false, false, "Show help message");
        opts.add("input", 'i', true, true, "Input EDS file (.eds / .leds)");
        opts.add("sources", 's', true, false, "Input source file (default: <input> with the .seds extension)");
        opts.add("region", 'r', true, false, "PATH:START-END, characters of a path (repeatable)");
        opts.add("columns", 0, true, false, "START-END, columns of the alignment view (repeatable)");
        opts.add("bed", 0, true, false, "BED3+ file: path, start, end and, in column 4, the output name");
        opts.add("output", 'o', true, false, "Output EDS file of the one region (sources: the same with .seds)");
        opts.add("output-dir", 0, true, false, "Directory for <name>.eds / <name>.seds of every region");
        opts.add("prefix", 0, true, false, "Path name prefix accepted in front of an id (default: path)");
        opts.add("table", 0, false, false, "Print one line per region: symbols, cuts, columns, sizes, status");
        opts.add("max-bytes", 0, true, false, "Fail when all slices together are larger (default: no limit)");
        opts.parse(argc, argv);
        if (opts.has("help")) {
            std::cout << "edsparser-slice - cut regions out of an EDS by path or column coordinates\n\n" << opts.usage() << "\n"
                      << "EXAMPLES:\n"
                         "  edsparser-slice -i in.eds -r 7:10200000-10300000 -o region.eds    # of path 7, with all variation there\n"
                         "  edsparser-slice -i in.eds --columns 0-5000 --columns 5000-10000 --output-dir parts\n"
                         "  edsparser-slice -i in.eds --bed genes.bed --output-dir genes --table > genes.tsv\n\n";
            return;
        }
        opts.notify();
        const tool::Files f = tool::files(opts);
        const std::string prefix = opts.get("prefix", "path");
        uint64_t max_bytes = 0;
        if (opts.has("max-bytes") && !slice_args::parse_u64(opts.get("max-bytes"), max_bytes))
            tool::fail("the argument ('" + opts.get("max-bytes") + "') for option '--max-bytes' is invalid");

        // the regions, in command-line order
        std::vector<slice_args::Region> regions;
        for (const auto& g : opts.given()) {
            slice_args::Region r;
            if (g.first == "region") {
                if (!slice_args::parse_region(g.second, prefix, r)) tool::fail("the argument ('" + g.second + "') for option '--region' is invalid");
                regions.push_back(r);
            } else if (g.first == "columns") {
                if (!slice_args::parse_columns(g.second, r)) tool::fail("the argument ('" + g.second + "') for option '--columns' is invalid");
                regions.push_back(r);
            } else if (g.first == "bed") {
                std::ifstream file(g.second, std::ios::binary);
                if (!file) tool::fail("Cannot open BED file: \"" + g.second + "\"");
                size_t line_no = 0;
                for (std::string line; std::getline(file, line);) {
                    line_no++;
                    const int rc = slice_args::parse_bed_line(line, prefix, r);
                    if (rc < 0) tool::fail("BED file line " + std::to_string(line_no) + " is malformed: \"" + line + "\"");
                    if (rc > 0) regions.push_back(r);
                }
            }
        }
        const size_t n = regions.size();
        if (n == 0) tool::fail("No region given (-r, --columns or --bed)");
        const bool to_file = opts.has("output"), to_dir = opts.has("output-dir");
        if (to_file && to_dir) tool::fail("--output and --output-dir exclude each other");
        if (to_file && n != 1) tool::fail("--output takes one region; use --output-dir for " + std::to_string(n));
        if (!to_file && !to_dir && !opts.has("table")) tool::fail("Nothing to do: give --output, --output-dir or --table");
        tool::need_files(f, true);

        std::cerr << "Loading EDS file: " << f.input << "\n";
        tool::Session ses(f);
        std::cerr << "Loaded EDS with " << ses.info.n_symbols << " symbols, " << ses.info.num_paths << " paths\n";
        std::cerr << "Slicing " << n << " regions...\n";

        std::vector<uint64_t> path(n), start(n), end(n);
        for (size_t r = 0; r < n; r++) { path[r] = regions[r].path; start[r] = regions[r].start; end[r] = regions[r].end; }
        std::vector<edsx_slice_region> reg(n);
        std::vector<uint8_t> st(n);
        detail::Buf eds, seds;
        ses.check(edsx_paths_slice(ses.s, n, path.data(), start.data(), end.data(), max_bytes, &eds.b, &seds.b, reg.data(), st.data()));

        if (to_dir) std::filesystem::create_directories(opts.get("output-dir"));
        std::string table;
        size_t written = 0;
        for (size_t r = 0; r < n; r++) {
            const edsx_slice_region& g = reg[r];
            if (opts.has("table"))
                table += regions[r].name + "\t" + num(g.symbol_first) + "\t" + num(g.symbol_last) + "\t" + num(g.cut_first) + "\t" + num(g.cut_end) +
                         "\t" + num(g.column_first) + "\t" + num(g.column_end) + "\t" + num(g.strings) + "\t" + num(g.chars) + "\t" +
                         num(g.eds_len) + "\t" + num(g.seds_len) + "\t" + (st[r] ? "RANGE" : "OK") + "\n";
            if (st[r]) {
                std::cerr << "Region " << regions[r].name << " (" << (path[r] ? prefix + std::to_string(path[r]) : std::string("columns")) << " "
                          << start[r] << "-" << end[r] << ") is empty or out of range: nothing written\n";
                continue;
            }
            if (!to_file && !to_dir) continue;
            std::filesystem::path e = to_file ? std::filesystem::path(opts.get("output")) : std::filesystem::path(opts.get("output-dir")) / (regions[r].name + ".eds");
            std::filesystem::path q = e;
            if (to_file) q.replace_extension(".seds"); else q = std::filesystem::path(opts.get("output-dir")) / (regions[r].name + ".seds");
            tool::write_bytes(e, static_cast<const uint8_t*>(eds.b.data) + g.eds_off, g.eds_len, "output");
            tool::write_bytes(q, static_cast<const uint8_t*>(seds.b.data) + g.seds_off, g.seds_len, "sources output");
            written++;
        }
        std::cout << table;
        edsx_paths_timing t;
        edsx_paths_last_timing(ses.s, &t);
        std::cerr << "Device: resolve, count and scan " << t.choose_ms + t.scan_ms << " ms, fill " << t.copy_ms << " ms, " << t.bytes_written << " bytes\n";
        if (to_file || to_dir) std::cerr << "Slices written: " << written << " of " << n << "\n";
    });
}
