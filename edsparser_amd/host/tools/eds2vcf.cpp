// eds2vcf — write an EDS, and the genotypes of its sources when it has them, as a VCF 4.2 file plus the reference FASTA
// its positions refer to, on the GPU (edsx_eds_vcf).  Every symbol with two strings or more becomes a record, every path a
// sample column: the way from msa2eds / vcf2eds / edsparser-subset back to bcftools, association pipelines and IGV.
// Banner, "[Performance]" line and exit codes in the style of the other tools.
#include "tool_front.hpp"

using namespace edsparser;

int main(int argc, char** argv)
{
    return tool::run([&] {
        cli::Parser opts("Write an EDS and its sources as a VCF plus reference FASTA");
        opts.add("help", 'h', false, false, "Show help message");
        opts.add("input", 'i', true, true, "Input EDS file (.eds / .leds)");
        opts.add("sources", 's', true, false, "Input source file (default: <input> with the .seds extension, if it exists)");
        opts.add("no-samples", 0, false, false, "Write the eight fixed columns alone, even when there are sources");
        opts.add("output", 'o', true, false, "Output VCF file (default: <input stem>.vcf)");
        opts.add("ref-out", 0, true, false, "Output reference FASTA (default: <input stem>.ref.fa)");
        opts.add("chrom", 0, true, false, "Contig name (default: eds)");
        opts.add("ref-path", 0, true, false, "Path whose strings are the reference alleles (default: 0, the first string of every symbol)");
        opts.add("names", 0, true, false, "File whose line k names the sample of path k (default: <prefix><id>)");
        opts.add("prefix", 0, true, false, "Sample name prefix (default: path)");
        opts.add("line-width", 0, true, false, "Line width of the reference FASTA, 0 = one line (default: 60)");
        opts.add("max-bytes", 0, true, false, "Refuse record lines of more bytes than this in all (default: no limit)");
        opts.parse(argc, argv);
        if (opts.has("help")) {
            std::cout << "eds2vcf - an EDS and its sources as a VCF plus reference FASTA\n\n" << opts.usage() << "\n"
                      << "Every symbol with two strings or more is one record; its first string (or the string of --ref-path) is\n"
                         "REF, the other strings follow in file order as ALT.  Equal texts are not merged and nothing is trimmed.\n"
                         "A record with an empty string gets the reference base in front of it on every allele.  With sources,\n"
                         "every path is one sample; its genotype lists the alleles whose source set holds it, joined by '/'.\n"
                         "There is no path selection here: edsparser-subset restricts an EDS to chosen paths and renumbers them.\n\n"
                         "EXAMPLES:\n"
                         "  eds2vcf -i in.eds                       # in.seds, if there, -> in.vcf and in.ref.fa\n"
                         "  eds2vcf -i in.eds --no-samples -o sites.vcf\n"
                         "  eds2vcf -i in.eds --ref-path 1 --chrom chr21 --names samples.txt\n\n";
            return;
        }
        opts.notify();
        const tool::Files f = tool::files(opts, ".vcf");
        std::filesystem::path ref_file = opts.get("ref-out");
        if (ref_file.empty()) ref_file = tool::beside(f.input, ".ref.fa");
        const bool no_samples = opts.has("no-samples");
        const std::string chrom = opts.get("chrom", "eds");
        tool::need_input(f);
        if (no_samples && (f.sources_given || opts.has("names") || opts.has("ref-path")))
            tool::fail("--no-samples does not go with --sources, --names or --ref-path");
        const bool with_samples = !no_samples && std::filesystem::exists(f.sources);
        if (!no_samples && !with_samples && f.sources_given) tool::fail("Sources file does not exist: " + f.sources.string());
        if (!with_samples && opts.has("names")) tool::fail("--names needs sources (.seds): " + f.sources.string() + " does not exist");

        // every line of the names file goes to the library as it is: it names the samples and checks the names itself
        const tool::Names table(opts, "path");
        const std::vector<const char*> names = tool::c_strs(table.lines);

        std::cout << "EDS → VCF export\n";
        std::cout << "  Input: " << f.input << "\n";
        if (with_samples) std::cout << "  Sources: " << f.sources << "\n";
        std::cout << "  Output: " << f.output << "\n";
        std::cout << "  Reference: " << ref_file << "\n";

        edsx_ctx* ctx = detail::context();
        const tool::MappedFile eds(f.input, "input");
        edsx_vcf_export_opts o{};
        o.chrom = chrom.c_str(); o.prefix = table.prefix.c_str();
        o.ref_path = opts.get_unsigned("ref-path", 0);
        o.line_width = opts.get_unsigned("line-width", 60);
        o.max_bytes = opts.get_unsigned("max-bytes", 0);
        static const char* const none[1] = {nullptr};
        if (table.given) { o.names = names.empty() ? none : names.data(); o.n_names = names.size(); }
        edsx_vcf_export_info info;
        detail::Buf vcf, fa;
        int rc;
        if (with_samples) {
            const tool::MappedFile seds(f.sources, "sources");
            rc = edsx_eds_vcf(ctx, eds.data(), eds.size(), seds.data(), seds.size(), &o, &vcf.b, &fa.b, &info);
        } else rc = edsx_eds_vcf(ctx, eds.data(), eds.size(), nullptr, 0, &o, &vcf.b, &fa.b, &info);
        tool::check(ctx, rc);
        tool::write_bytes(f.output, vcf.b.data, vcf.b.size, "output");
        tool::write_bytes(ref_file, fa.b.data, fa.b.size, "reference");

        std::cout << "  Symbols: " << info.symbols << ", strings: " << info.strings << "\n";
        std::cout << "  Records: " << info.records << " (" << info.anchored << " anchored)";
        if (with_samples) std::cout << ", samples: " << info.paths;
        std::cout << "\n  Reference length: " << info.ref_length << "\n";
        if (info.overlapping)
            std::cerr << "Warning: " << info.overlapping << (info.overlapping == 1 ? " record overlaps" : " records overlap")
                      << " the record before: anchored next to another degenerate symbol\n";
        std::cout << "  Bytes written: " << vcf.b.size + fa.b.size << "\n";
        std::cout << "Export complete!\n";
    });
}
