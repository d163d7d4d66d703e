// edsparser-ld — linkage disequilibrium between the alleles of an EDS with sources, on the GPU (edsx_paths_ld): r² between
// every two alleles whose choice symbols lie at most --window choice symbols apart, the table a pruning step, a
// haplotype-block plot or a tag-SNP choice otherwise computes from the genotypes eds2vcf writes.  An allele is a string of a
// symbol with a choice - string 0, REF in eds2vcf's convention, only with --all-strings - that at least --min-count of the
// paths take and at least --min-count of the paths present there do not.  The texts are written on the host:
//   pairs    "symbol_a string_a symbol_b string_b n_ab n_a n_b n r2", tab separated, r2 as %.6g, the pairs with r2 >= --min-r2
//   --freq   "symbol string count present freq": the listed alleles, the allele frequency table of the panel
// Banner, "[Performance]" line and exit codes in the style of the other tools.
#include "tool_front.hpp"

#include <cmath>
#include <cstdio>
#include <vector>

using namespace edsparser;

int main(int argc, char** argv)
{
    return tool::run([&] {
        cli::Parser opts("Linkage disequilibrium between the alleles of an EDS with sources");
        opts.add("help", 'h', false, false, "Show help message");
        opts.add("input", 'i', true, true, "Input EDS file (.eds / .leds)");
        opts.add("sources", 's', true, false, "Input source file (default: <input> with the .seds extension)");
        opts.add("output", 'o', true, false, "Output pair file (default: <input stem>.ld)");
        opts.add("paths", 'p', true, false, "Path ids and ranges, e.g. 1,5,7-9 (default: all paths)");
        opts.add("window", 0, true, false, "Pairs of alleles at most this many choice symbols apart (default: 100)");
        opts.add("min-r2", 0, true, false, "Report pairs with r2 at or above this value of [0, 1] (default: 0.2)");
        opts.add("min-count", 0, true, false, "List alleles that this many paths take and this many do not (default: 1)");
        opts.add("all-strings", 0, false, false, "List string 0 of a symbol too");
        opts.add("freq", 0, true, false, "Write the listed alleles with their counts to this file");
        opts.add("max-pairs", 0, true, false, "Refuse more pairs than this, 0 = no limit (default: 0)");
        opts.parse(argc, argv);
        if (opts.has("help")) {
            std::cout << "edsparser-ld - linkage disequilibrium between the alleles of an EDS\n\n" << opts.usage() << "\n"
                      << "An allele is a string of a symbol that is not a single string of all paths; a path carries the first\n"
                         "string of a symbol, in file order, that names it.  Counts are taken over the paths that have a string\n"
                         "at both symbols; a pair in which an allele is carried by all or none of them has no r2 and is left out.\n\n"
                         "EXAMPLES:\n"
                         "  edsparser-ld -i in.eds                                    # in.seds -> in.ld, window 100, r2 >= 0.2\n"
                         "  edsparser-ld -i in.eds --window 1000 --min-r2 0.8 --min-count 5 --freq in.frq -o pruned.ld\n\n";
            return;
        }
        opts.notify();
        const tool::Files f = tool::files(opts, ".ld");
        edsx_ld_opts lo;
        lo.window = opts.get_unsigned("window", 100);
        lo.min_count = opts.get_unsigned("min-count", 1);
        lo.max_pairs = opts.get_unsigned("max-pairs", 0);
        lo.all_strings = opts.has("all-strings") ? 1 : 0;
        lo.min_r2 = 0.2;
        if (lo.window == 0) tool::fail("the argument ('0') for option '--window' is invalid");
        if (opts.has("min-r2")) {
            const std::string t = opts.get("min-r2");
            size_t used = 0;
            try { lo.min_r2 = std::stod(t, &used); } catch (...) { used = 0; }
            if (used != t.size() || t.empty() || !(lo.min_r2 >= 0.0 && lo.min_r2 <= 1.0))
                tool::fail("the argument ('" + t + "') for option '--min-r2' is invalid");
        }
        tool::need_files(f);
        const std::vector<uint64_t> ids = tool::path_list(opts, "paths");   // none: all paths, and the library checks the ids

        std::cout << "EDS linkage disequilibrium\n";
        std::cout << "  Input: " << f.input << "\n";
        std::cout << "  Sources: " << f.sources << "\n";
        std::cout << "  Output: " << f.output << "\n";
        std::cout << "  Window: " << lo.window << " choice symbols, r2 >= " << lo.min_r2 << ", min count: " << lo.min_count
                  << (lo.all_strings ? ", all strings" : "") << "\n";

        tool::Session ses(f);
        detail::Buf pairs, alleles;
        edsx_ld_info li;
        ses.check(edsx_paths_ld(ses.s, ids.data(), ids.size(), &lo, &pairs.b, &alleles.b, &li));
        std::cout << "  Paths: " << li.paths << ", choice symbols: " << li.choice_symbols << ", alleles: " << li.alleles << "\n";
        std::cout << "  Candidate pairs: " << li.candidate_pairs << " in " << li.tiles << (li.tiles == 1 ? " tile" : " tiles") << ", undefined: "
                  << li.undefined_pairs << ", reported: " << li.pairs << "\n";

        char line[256];
        std::string text = "symbol_a\tstring_a\tsymbol_b\tstring_b\tn_ab\tn_a\tn_b\tn\tr2\n";
        const edsx_ld_pair* p = reinterpret_cast<const edsx_ld_pair*>(pairs.b.data);
        for (uint64_t k = 0; k < li.pairs; k++) {
            std::snprintf(line, sizeof(line), "%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%.6g\n", (unsigned long long)p[k].symbol_a,
                          (unsigned long long)p[k].string_a, (unsigned long long)p[k].symbol_b, (unsigned long long)p[k].string_b,
                          (unsigned long long)p[k].n_ab, (unsigned long long)p[k].n_a, (unsigned long long)p[k].n_b, (unsigned long long)p[k].n,
                          p[k].r2);
            text += line;
        }
        tool::write_bytes(f.output, reinterpret_cast<const uint8_t*>(text.data()), text.size(), "output");
        if (opts.has("freq")) {
            std::string ft = "symbol\tstring\tcount\tpresent\tfreq\n";
            const edsx_ld_allele* a = reinterpret_cast<const edsx_ld_allele*>(alleles.b.data);
            for (uint64_t k = 0; k < li.alleles; k++) {
                const double f = a[k].present ? static_cast<double>(a[k].count) / static_cast<double>(a[k].present) : 0.0;
                std::snprintf(line, sizeof(line), "%llu\t%llu\t%llu\t%llu\t%.6g\n", (unsigned long long)a[k].symbol, (unsigned long long)a[k].string,
                              (unsigned long long)a[k].count, (unsigned long long)a[k].present, f);
                ft += line;
            }
            tool::write_bytes(opts.get("freq"), reinterpret_cast<const uint8_t*>(ft.data()), ft.size(), "frequency");
        }
        edsx_paths_timing t;
        edsx_paths_last_timing(ses.s, &t);
        std::cout << "  Device: allele and tile lists " << t.scan_ms << " ms, rows and pairs " << t.copy_ms << " ms\n";
        std::cout << "  Pairs written: " << li.pairs << ", " << text.size() << " bytes\n";
        std::cout << "LD complete!\n";
    });
}
