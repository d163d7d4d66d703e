// edsparser-mosaic — paths of an EDS with sources written as minimal mosaics of other paths, on the GPU (edsx_paths_mosaic):
// every target as the fewest copies from the donors plus the symbols no donor shares - the breakpoints of a recombinant, the
// parental origin along a cross, the painting of a panel by itself, the closest-donor track - which one would otherwise
// compute from the records of edsparser-ibs or the rows eds2msa writes with a greedy interval cover per target.  The text
// is written on the host:
//   "target\tdonor\tsymbol_first\tsymbol_last\tsites\tcolumn_first\tcolumn_end\tcolumns", then one line per record in record
//   order; donor is "." for a private segment; columns = column_end - column_first, ready for edsparser-slice --columns.
//   --breakpoints: "target\tdonor_before\tdonor_after\tsymbol\tcolumn", one line per place where the donor of a target
//   changes: the symbol and the column at which the new segment starts.
// Paths are named <prefix><id - 1>, as eds2msa names them, or by line id of --names.  Banner, "[Performance]" line and exit
// codes in the style of the other tools.
#include "edsx.h"
#include "../cli_util.hpp"
#include "../device.hpp"
#include "tool_common.hpp"

#include <vector>

using namespace edsparser;

namespace {

struct Session {
    edsx_paths_session* s = nullptr;
    ~Session() { edsx_paths_close(s); }
};

struct Buf {
    edsx_buf b{nullptr, 0};
    ~Buf() { edsx_buf_free(&b); }
};

// tool::parse_paths under the name of the option it reads
std::vector<uint64_t> parse_list(const std::string& text, const std::string& option)
{
    try { return tool::parse_paths(text); }
    catch (const std::runtime_error&) { throw std::runtime_error("the argument ('" + text + "') for option '--" + option + "' is invalid"); }
}

} // namespace

int main(int argc, char** argv)
{
    Timer timer;
    timer.start();
    try {
        cli::Parser opts("Paths of an EDS with sources as minimal mosaics of other paths");
        opts.add("help", 'h', false, false, "Show help message");
        opts.add("input", 'i', true, true, "Input EDS file (.eds / .leds)");
        opts.add("sources", 's', true, false, "Input source file (default: <input> with the .seds extension)");
        opts.add("output", 'o', true, false, "Output table file (default: <input stem>.mosaic)");
        opts.add("targets", 't', true, false, "Target path ids and ranges, e.g. 1,5,7-9 (default: all paths)");
        opts.add("donors", 'd', true, false, "Donor path ids and ranges (default: all paths)");
        opts.add("max-segments", 0, true, false, "Refuse more segments than this, 0 = no limit (default: 0)");
        opts.add("breakpoints", 0, false, false, "Write only where the donor of a target changes");
        opts.add("names", 0, true, false, "File whose line k names path k (default: <prefix><id - 1>)");
        opts.add("prefix", 0, true, false, "Path name prefix (default: s)");
        opts.parse(argc, argv);
        if (opts.has("help")) {
            std::cout << "edsparser-mosaic - paths of an EDS as the fewest copies from other paths\n\n" << opts.usage() << "\n"
                      << "A copied segment is a run of symbols at all of which the target and its donor take the same string; it\n"
                         "reaches as far as any donor does, and of donors that reach equally far the first one listed has it.  A\n"
                         "private segment (donor '.') holds symbols that no donor shares.  A donor that is the target's own path is\n"
                         "skipped, so without -t and -d every path is painted by all the others.  sites counts the symbols inside\n"
                         "that offer a choice, the columns are those of the alignment eds2msa writes.  Paths are named <prefix>0,\n"
                         "<prefix>1, ... for paths 1, 2, ...\n\n"
                         "EXAMPLES:\n"
                         "  edsparser-mosaic -i in.eds                               # in.seds -> in.mosaic, every path by the others\n"
                         "  edsparser-mosaic -i in.eds -t 7 -d 1-6 --breakpoints -o breaks.tsv\n\n";
            tool::print_performance(timer);
            return 0;
        }
        opts.notify();
        const std::filesystem::path input_file = opts.get("input");
        std::filesystem::path sources_file = opts.get("sources"), output_file = opts.get("output");
        if (sources_file.empty()) { sources_file = input_file; sources_file.replace_extension(".seds"); }
        if (output_file.empty()) output_file = input_file.parent_path() / (input_file.stem().string() + ".mosaic");
        const unsigned long max_segments = opts.get_unsigned("max-segments", 0);
        const bool breakpoints = opts.has("breakpoints");
        const std::string prefix = opts.get("prefix", "s");
        auto fail = [&](const std::string& msg) { std::cerr << "Error: " << msg << "\n"; tool::print_performance(timer); return 1; };
        if (!std::filesystem::exists(input_file)) return fail("Input file does not exist: " + input_file.string());
        if (!std::filesystem::exists(sources_file)) return fail("Path spelling needs sources (.seds): " + sources_file.string() + " does not exist");
        std::vector<uint64_t> targets, donors;
        if (opts.has("targets")) targets = parse_list(opts.get("targets"), "targets");
        if (opts.has("donors")) donors = parse_list(opts.get("donors"), "donors");

        std::cout << "EDS path mosaics\n";
        std::cout << "  Input: " << input_file << "\n";
        std::cout << "  Sources: " << sources_file << "\n";
        std::cout << "  Output: " << output_file << (breakpoints ? " (breakpoints)\n" : "\n");

        edsx_ctx* ctx = detail::context();
        Session ses;
        {
            const tool::MappedFile eds(input_file, "input"), seds(sources_file, "sources");
            if (edsx_paths_open(ctx, eds.data(), eds.size(), seds.data(), seds.size(), &ses.s) != EDSX_OK)
                return fail(edsx_last_error(ctx));
        }
        edsx_paths_info_t pi;
        edsx_paths_info(ses.s, &pi);
        if (!opts.has("targets")) for (uint64_t p = 1; p <= pi.num_paths; p++) targets.push_back(p);
        if (!opts.has("donors")) for (uint64_t p = 1; p <= pi.num_paths; p++) donors.push_back(p);
        for (const auto* ids : {&targets, &donors})                // before the output file is created
            for (uint64_t p : *ids)
                if (p == 0 || p > pi.num_paths)
                    return fail("Path id " + std::to_string(p) + " out of range (1.." + std::to_string(pi.num_paths) + ")");

        std::vector<std::string> all_names;
        if (opts.has("names")) {
            std::ifstream nf(opts.get("names"));
            if (!nf) return fail("Cannot open names file: " + opts.get("names"));
            for (std::string line; std::getline(nf, line);) {
                if (!line.empty() && line.back() == '\r') line.pop_back();
                all_names.push_back(line);
            }
        }
        std::vector<std::string> tname, dname;
        for (const auto& [ids, name] : {std::make_pair(&targets, &tname), std::make_pair(&donors, &dname)})
            for (uint64_t p : *ids) {
                if (!opts.has("names")) name->push_back(prefix + std::to_string(p - 1));
                else if (p > all_names.size()) return fail("The names file has no name for path " + std::to_string(p));
                else name->push_back(all_names[p - 1]);
                if (name->back().empty() || name->back().find_first_of("\t \n") != std::string::npos)
                    return fail("The name of path " + std::to_string(p) + " is empty or holds a tab, blank or line feed");
            }

        Buf segs, off;
        edsx_mosaic_info mi{0, 0, 0, 0, 0, 0, 0, 0};
        if (!targets.empty() && edsx_paths_mosaic(ses.s, targets.data(), targets.size(), donors.data(), donors.size(), max_segments, &segs.b,
                                                  &off.b, &mi) != EDSX_OK)
            return fail(edsx_last_error(ctx));
        std::cout << "  Targets: " << targets.size() << ", donors: " << donors.size() << " of " << pi.num_paths << " paths, choice symbols: "
                  << mi.choice_symbols << ", class columns: " << mi.class_columns << "\n";

        const edsx_mosaic_segment* rec = reinterpret_cast<const edsx_mosaic_segment*>(segs.b.data);
        auto who = [&](uint64_t y) { return y == UINT64_MAX ? std::string(".") : dname[y]; };
        std::string text;
        uint64_t lines = 0;
        if (breakpoints) {
            text = "target\tdonor_before\tdonor_after\tsymbol\tcolumn\n";
            for (uint64_t k = 1; k < mi.segments; k++) {
                const edsx_mosaic_segment &a = rec[k - 1], &b = rec[k];
                if (a.target != b.target) continue;
                text += tname[b.target] + '\t' + who(a.donor) + '\t' + who(b.donor) + '\t' + std::to_string(b.symbol_first) + '\t' +
                        std::to_string(b.column_first) + '\n';
                lines++;
            }
        } else {
            text = "target\tdonor\tsymbol_first\tsymbol_last\tsites\tcolumn_first\tcolumn_end\tcolumns\n";
            for (uint64_t k = 0; k < mi.segments; k++) {
                const edsx_mosaic_segment& s = rec[k];
                text += tname[s.target]; text += '\t'; text += who(s.donor);
                for (uint64_t v : {s.symbol_first, s.symbol_last, s.sites, s.column_first, s.column_end, s.column_end - s.column_first}) {
                    text += '\t';
                    text += std::to_string(v);
                }
                text += '\n';
            }
            lines = mi.segments;
        }
        tool::write_bytes(output_file, reinterpret_cast<const uint8_t*>(text.data()), text.size(), "output");
        edsx_paths_timing t;
        edsx_paths_last_timing(ses.s, &t);
        std::cout << "  Device: tables " << t.choose_ms << " ms, class list and scan " << t.scan_ms << " ms, rows and march " << t.copy_ms << " ms\n";
        std::cout << "  Segments: " << mi.segments << " (" << mi.private_segments << " private over " << mi.private_symbols << " symbols), switches: "
                  << mi.switches << "; lines written: " << lines << ", " << text.size() << " bytes\n";
        std::cout << "Mosaic complete!\n";
        tool::print_performance(timer);
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "Error: " << e.what() << "\n";
        tool::print_performance(timer);
        return 1;
    }
}
