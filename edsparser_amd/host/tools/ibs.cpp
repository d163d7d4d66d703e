// edsparser-ibs — the segments every two paths of an EDS with sources share, on the GPU (edsx_paths_ibs): the maximal
// stretches of symbols over which two paths take the same strings (identity by state), the table a relatedness estimate, a
// recombination breakpoint search or a duplicate check would otherwise compute from the rows eds2msa writes with an
// O(P^2 W) run-length loop.  --min-sites and --min-columns drop short segments.  The text is written on the host:
//   "path_a\tpath_b\tsymbol_first\tsymbol_last\tsites\tcolumn_first\tcolumn_end\tcolumns", then one line per record in
//   record order; columns = column_end - column_first, ready for edsparser-slice --columns.
// Paths are named <prefix><id - 1>, as eds2msa names them, or by line id of --names.  Banner, "[Performance]" line and exit
// codes in the style of the other tools.
#include "tool_front.hpp"

#include <vector>

using namespace edsparser;

int main(int argc, char** argv)
{
    return tool::run([&] {
        cli::Parser opts("Segments that two paths of an EDS with sources share");
        opts.add("help", 'h', false, false, "Show help message");
        opts.add("input", 'i', true, true, "Input EDS file (.eds / .leds)");
        opts.add("sources", 's', true, false, "Input source file (default: <input> with the .seds extension)");
        opts.add("output", 'o', true, false, "Output table file (default: <input stem>.ibs)");
        opts.add("paths", 'p', true, false, "Path ids and ranges, e.g. 1,5,7-9 (default: all paths)");
        opts.add("min-sites", 0, true, false, "Report segments with at least this many choice symbols (default: 1)");
        opts.add("min-columns", 0, true, false, "Report segments with at least this many alignment columns (default: 0)");
        opts.add("max-segments", 0, true, false, "Refuse more segments than this, 0 = no limit (default: 0)");
        opts.add("names", 0, true, false, "File whose line k names path k (default: <prefix><id - 1>)");
        opts.add("prefix", 0, true, false, "Path name prefix (default: s)");
        opts.parse(argc, argv);
        if (opts.has("help")) {
            std::cout << "edsparser-ibs - the segments every two paths of an EDS share\n\n" << opts.usage() << "\n"
                      << "A segment is a maximal run of symbols at all of which the two paths take the same string; it is\n"
                         "bounded by a symbol where they differ or by an end of the EDS.  sites counts the symbols inside that\n"
                         "offer a choice, the columns are those of the alignment eds2msa writes.  Paths are named <prefix>0,\n"
                         "<prefix>1, ... for paths 1, 2, ...\n\n"
                         "EXAMPLES:\n"
                         "  edsparser-ibs -i in.eds                                   # in.seds -> in.ibs, all pairs of paths\n"
                         "  edsparser-ibs -i in.eds -p 1-32 --min-sites 50 --min-columns 10000 -o tracts.tsv\n\n";
            return;
        }
        opts.notify();
        const tool::Files f = tool::files(opts, ".ibs");
        const unsigned long min_sites = opts.get_unsigned("min-sites", 1), min_columns = opts.get_unsigned("min-columns", 0),
                            max_segments = opts.get_unsigned("max-segments", 0);
        tool::need_files(f);
        std::vector<uint64_t> ids = tool::path_list(opts, "paths");

        std::cout << "EDS shared segments\n";
        std::cout << "  Input: " << f.input << "\n";
        std::cout << "  Sources: " << f.sources << "\n";
        std::cout << "  Output: " << f.output << "\n";
        std::cout << "  Minimum: " << min_sites << " sites, " << min_columns << " columns\n";

        tool::Session ses(f);
        const edsx_paths_info_t& pi = ses.info;
        tool::resolve_paths(ids, pi.num_paths);                  // before the output file is created
        const size_t K = ids.size();

        const std::vector<std::string> name = tool::Names(opts, "s").names_of(ids, true);

        detail::Buf segs, off;
        edsx_ibs_info ii{0, 0, 0, 0, 0, 0, 0, 0};
        if (K) ses.check(edsx_paths_ibs(ses.s, ids.data(), K, min_sites, min_columns, max_segments, &segs.b, &off.b, &ii));
        std::cout << "  Paths: " << K << " of " << pi.num_paths << ", pairs: " << ii.pairs << ", choice symbols: " << ii.choice_symbols
                  << ", class columns: " << ii.class_columns << " in " << ii.chunks << (ii.chunks == 1 ? " chunk" : " chunks") << "\n";

        std::string text = "path_a\tpath_b\tsymbol_first\tsymbol_last\tsites\tcolumn_first\tcolumn_end\tcolumns\n";
        const edsx_ibs_segment* rec = reinterpret_cast<const edsx_ibs_segment*>(segs.b.data);
        for (uint64_t k = 0; k < ii.segments; k++) {
            const edsx_ibs_segment& s = rec[k];
            text += name[s.x]; text += '\t'; text += name[s.y];
            for (uint64_t v : {s.symbol_first, s.symbol_last, s.sites, s.column_first, s.column_end, s.column_end - s.column_first}) {
                text += '\t';
                text += std::to_string(v);
            }
            text += '\n';
        }
        tool::write_bytes(f.output, reinterpret_cast<const uint8_t*>(text.data()), text.size(), "output");
        edsx_paths_timing t;
        edsx_paths_last_timing(ses.s, &t);
        std::cout << "  Device: tables " << t.choose_ms << " ms, class list, stitch and scan " << t.scan_ms << " ms, rows and segment scan "
                  << t.copy_ms << " ms\n";
        std::cout << "  Segments written: " << ii.segments << " of " << ii.candidate_segments << ", " << text.size() << " bytes\n";
        std::cout << "IBS complete!\n";
    });
}
