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
#include "tool_front.hpp"

#include <vector>

using namespace edsparser;

int main(int argc, char** argv)
{
    return tool::run([&] {
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
            return;
        }
        opts.notify();
        const tool::Files f = tool::files(opts, ".mosaic");
        const unsigned long max_segments = opts.get_unsigned("max-segments", 0);
        const bool breakpoints = opts.has("breakpoints");
        tool::need_files(f);
        std::vector<uint64_t> targets = tool::path_list(opts, "targets"), donors = tool::path_list(opts, "donors");

        std::cout << "EDS path mosaics\n";
        std::cout << "  Input: " << f.input << "\n";
        std::cout << "  Sources: " << f.sources << "\n";
        std::cout << "  Output: " << f.output << (breakpoints ? " (breakpoints)\n" : "\n");

        tool::Session ses(f);
        const edsx_paths_info_t& pi = ses.info;
        tool::resolve_paths(targets, pi.num_paths);              // before the output file is created
        tool::resolve_paths(donors, pi.num_paths);

        const tool::Names table(opts, "s");
        const std::vector<std::string> tname = table.names_of(targets, true), dname = table.names_of(donors, true);

        detail::Buf segs, off;
        edsx_mosaic_info mi{0, 0, 0, 0, 0, 0, 0, 0};
        if (!targets.empty())
            ses.check(edsx_paths_mosaic(ses.s, targets.data(), targets.size(), donors.data(), donors.size(), max_segments, &segs.b, &off.b, &mi));
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
        tool::write_bytes(f.output, reinterpret_cast<const uint8_t*>(text.data()), text.size(), "output");
        edsx_paths_timing t;
        edsx_paths_last_timing(ses.s, &t);
        std::cout << "  Device: tables " << t.choose_ms << " ms, class list and scan " << t.scan_ms << " ms, rows and march " << t.copy_ms << " ms\n";
        std::cout << "  Segments: " << mi.segments << " (" << mi.private_segments << " private over " << mi.private_symbols << " symbols), switches: "
                  << mi.switches << "; lines written: " << lines << ", " << text.size() << " bytes\n";
        std::cout << "Mosaic complete!\n";
    });
}
