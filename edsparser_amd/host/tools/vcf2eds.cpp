// vcf2eds — VCF + reference FASTA -> EDS / l-EDS + sources, on the GPU.
// Flags, validation, naming, statistics block: src/cpp/tools/vcf2eds.cpp:36-43, :102-114,
// :159-180, :204-216.
#include "edsparser/transforms/vcf_transforms.hpp"
#include "edsx.h"
#include "../cli_util.hpp"
#include "../device.hpp"
#include "gz_input.hpp"
#include "tool_common.hpp"

using namespace edsparser;

namespace {

void print_statistics(const VCFStats& stats)
{
    std::cout << "Variant Processing Statistics:\n";
    std::cout << "  Total variants read:        " << stats.total_variants << "\n";
    std::cout << "  Successfully processed:     " << stats.processed_variants << "\n";
    std::cout << "  Skipped (malformed):        " << stats.skipped_malformed << "\n";
    std::cout << "  Skipped (unsupported SV):   " << stats.skipped_unsupported_sv << "\n";
    std::cout << "  Total skipped:              " << stats.total_skipped() << "\n";
    std::cout << "  Variant groups created:     " << stats.variant_groups << "\n";
    if (stats.total_variants > 0) {
        const double rate = (100.0 * stats.processed_variants) / stats.total_variants;
        std::cout << "  Success rate:               " << std::fixed << std::setprecision(1) << rate << "%\n";
    }
    std::cout << "\n";
}

VCFStats to_stats(const edsx_vcf_stats& c)
{
    VCFStats s;
    s.total_variants = c.total_variants; s.processed_variants = c.processed_variants;
    s.skipped_malformed = c.skipped_malformed; s.skipped_unsupported_sv = c.skipped_unsupported_sv;
    s.variant_groups = c.variant_groups;
    return s;
}

struct VcfSession {                                // edsx_vcf_session, closed on every way out
    edsx_vcf_session* h = nullptr;
    ~VcfSession() { edsx_vcf_session_close(h); }
};

// --all-chroms: one session, one pair of files per FASTA record that the VCF has record lines for.  false: a contig failed.
bool transform_all_contigs(const tool::GzInput& vcf_in, const tool::GzInput& fasta_in, bool compressed, const std::string& stem,
                           const std::filesystem::path& out_dir, Length context_length)
{
    edsx_ctx* ctx = detail::context();
    VcfSession ses;
    int rc = compressed ? edsx_vcf_session_open_z(ctx, vcf_in.data, vcf_in.size, fasta_in.data, fasta_in.size, &ses.h)
                        : edsx_vcf_session_open(ctx, vcf_in.data, vcf_in.size, fasta_in.data, fasta_in.size, &ses.h);
    if (rc != EDSX_OK) detail::throw_status(rc, ctx);
    const edsx_contig* recs = nullptr;
    size_t nrecs = 0;
    edsx_vcf_session_contigs(ses.h, &recs, &nrecs);
    {
        detail::Buf unknown;
        rc = edsx_vcf_session_unknown_contigs(ses.h, &unknown.b);
        if (rc != EDSX_OK) detail::throw_status(rc, ctx);
        std::istringstream lines(unknown.str());
        for (std::string ln; std::getline(lines, ln);) {
            const size_t tab = ln.rfind('\t');
            std::cerr << "Warning: contig '" << ln.substr(0, tab) << "' has " << ln.substr(tab + 1)
                      << " VCF record line(s) and no record in the reference FASTA\n";
        }
    }
    std::filesystem::create_directories(out_dir);
    std::vector<std::pair<std::string, VCFStats>> done;
    bool all_ok = true;
    for (size_t i = 0; i < nrecs; i++) {
        if (recs[i].duplicate || recs[i].vcf_records == 0) continue;
        const char* name_p = nullptr;
        size_t name_n = 0;
        if (edsx_vcf_session_contig_name(ses.h, i, &name_p, &name_n) != EDSX_OK || !name_p)
            throw std::runtime_error("FASTA record " + std::to_string(i) + " has no name in the session");
        const std::string name(name_p, name_n);
        try {
            if (name.empty() || name == "." || name == ".." || name.find('/') != std::string::npos || name.find('\0') != std::string::npos)
                throw std::runtime_error("contig name cannot be used in a file name");
            detail::Buf eds, seds;
            edsx_vcf_stats cst{};
            rc = edsx_vcf_session_transform(ses.h, i, context_length, &eds.b, &seds.b, &cst);
            if (rc != EDSX_OK) detail::throw_status(rc, ctx);
            const std::string base = context_length > 0 ? stem + "." + name + "_l" + std::to_string(context_length) : stem + "." + name;
            const std::filesystem::path eds_path = out_dir / (base + (context_length > 0 ? ".leds" : ".eds"));
            const std::filesystem::path seds_path = out_dir / (base + ".seds");
            tool::write_bytes(eds_path, eds.b.data, eds.b.size, "output");
            tool::write_bytes(seds_path, seds.b.data, seds.b.size, "sources");
            std::cout << "  Contig " << name << ": " << eds_path << ", " << seds_path << "\n";
            done.push_back({name, to_stats(cst)});
        } catch (const std::exception& e) {
            std::cerr << "Error [" << name << "]: " << e.what() << "\n";
            all_ok = false;
        }
    }
    std::cout << "Transformation complete!\n\n";
    for (const auto& d : done) {
        std::cout << "Contig " << d.first << "\n";
        print_statistics(d.second);
    }
    edsx_vcf_session_stats info{};
    edsx_vcf_session_info(ses.h, &info);
    std::cout << "VCF record lines: " << info.records_total << " total, " << info.records_without_token << " without a token, "
              << info.records_unknown_contig << " of contigs the reference lacks\n\n";
    return all_ok;
}

} // namespace

int main(int argc, char** argv)
{
    Timer timer;
    timer.start();
    try {
        cli::Parser opts("Transform VCF (Variant Call Format) to EDS/l-EDS");
        opts.add("help", 'h', false, false, "Show help message");
        opts.add("input", 'i', true, true, "Input VCF file (.vcf, .vcf.gz, .vcf.bgz)");
        opts.add("reference", 'r', true, true, "Reference FASTA file (plain, gzip or BGZF: probed by content)");
        opts.add("output", 'o', true, false, "Output EDS file (default: <input>.eds)");
        opts.add("sources", 's', true, false, "Output source file (default: <output>.seds)");
        opts.add("context-length", 'l', true, false, "Create l-EDS with minimum context length (0 = regular EDS)");
        opts.add("chrom", 'c', true, false, "Transform one contig: the VCF records whose CHROM is NAME over the FASTA record NAME");
        opts.add("all-chroms", 0, false, false, "Transform every contig of the reference that has VCF records: <stem>.<contig>.eds/.seds each");
        opts.add("output-dir", 0, true, false, "Directory of the --all-chroms outputs (default: the input's directory)");
        opts.add("gpus", 'g', true, false, "Spread the records over this many GPUs of the node by reference position (RCCL exchanges; default 1)");
        opts.parse(argc, argv);
        if (opts.has("help")) {
            std::cout << "vcf2eds - Transform VCF (Variant Call Format) to EDS\n\n" << opts.usage() << "\n"
                      << "DESCRIPTION:\n"
                         "  Transforms a VCF file with a reference FASTA to an Elastic-Degenerate\n"
                         "  String (EDS) with sample-level source tracking. Each sample in the VCF\n"
                         "  is tracked as a separate path in the source file.\n\n"
                         "SUPPORTED VARIANTS:\n"
                         "  SNPs, small indels, <DEL>, <INS>, multi-allelic sites\n\n"
                         "EXAMPLES:\n"
                         "  vcf2eds -i variants.vcf -r ref.fa            # variants.eds + variants.seds\n"
                         "  vcf2eds -i variants.vcf -r ref.fa --gpus 8   # position ranges on GPUs 0..7, over RCCL\n"
                         "  vcf2eds -i wgs.vcf -r hg38.fa --chrom chr21  # one contig of a multi-contig VCF and FASTA\n"
                         "  vcf2eds -i wgs.vcf -r hg38.fa --all-chroms --output-dir out   # out/wgs.<contig>.eds + .seds\n\n"
                         "CONTIGS:\n"
                         "  Without --chrom / --all-chroms the first FASTA record is the reference and CHROM is\n"
                         "  ignored, as the reference tool does.\n\n"
                         "COMPRESSED INPUT:\n"
                         "  -i takes .vcf.gz / .vcf.bgz, -r is probed by content.  BGZF (bgzip) files are inflated on\n"
                         "  the GPU, one wave per 64 KiB block, CRC-32 checked, and the text stays in device memory;\n"
                         "  any other gzip file is inflated on the host, on one thread.  x.vcf.gz writes x.eds.\n"
                         "  With --gpus N a compressed input is inflated on GPU 0 first.\n\n";
            tool::print_performance(timer);
            return 0;
        }
        opts.notify();
        const std::filesystem::path input_file = opts.get("input");
        // x.vcf.gz / x.vcf.bgz name their outputs as x.vcf does
        const bool named_gz = tool::gz_extension(input_file);
        const std::filesystem::path named_file = named_gz ? input_file.parent_path() / input_file.stem() : input_file;
        const std::filesystem::path reference_file = opts.get("reference");
        const std::filesystem::path output_file = opts.get("output");
        const std::filesystem::path sources_file = opts.get("sources");
        const Length context_length = static_cast<Length>(opts.get_unsigned("context-length", 0));
        const unsigned long ngpu = opts.has("gpus") ? opts.get_unsigned("gpus", 1) : 0;
        if (opts.has("gpus") && (ngpu == 0 || ngpu > 64)) throw std::runtime_error("--gpus must be between 1 and 64");
        const bool all_chroms = opts.has("all-chroms"), one_chrom = opts.has("chrom");
        const std::string chrom = opts.get("chrom");
        if (all_chroms && one_chrom) throw std::runtime_error("--chrom and --all-chroms exclude each other");
        if (all_chroms && (opts.has("output") || opts.has("sources")))
            throw std::runtime_error("--all-chroms names its outputs itself (<stem>.<contig>.eds): use --output-dir, not -o / -s");
        if (opts.has("output-dir") && !all_chroms) throw std::runtime_error("--output-dir needs --all-chroms");
        if ((all_chroms || one_chrom) && opts.has("gpus"))
            throw std::runtime_error("--chrom / --all-chroms cannot be combined with --gpus: contigs are transformed on one GPU");
        if (one_chrom && chrom.empty()) throw std::runtime_error("--chrom needs a contig name");

        if (named_file.extension() != ".vcf") {
            std::cerr << "Error: Input file must be a VCF file (.vcf)\n";
            std::cerr << "Got: " << input_file << "\n";
            tool::print_performance(timer);
            return 1;
        }
        if (!std::filesystem::exists(reference_file)) {
            std::cerr << "Error: Reference FASTA file not found: " << reference_file << "\n";
            tool::print_performance(timer);
            return 1;
        }
        // both files are mapped and handed to the C ABI as they are (no ifstream -> std::string copies)
        tool::MappedFile vcf_map(input_file, "VCF"), fasta_map(reference_file, "reference FASTA");
        // gzip / BGZF inputs: a broken compressed layer ends the run here, before any device work
        const tool::GzInput vcf_in(vcf_map, "VCF", named_gz), fasta_in(fasta_map, "FASTA", false);
        const bool compressed = vcf_in.compressed() || fasta_in.compressed();

        const bool create_leds = context_length > 0;
        if (create_leds) {
            std::cout << "VCF → l-EDS transformation (l=" << context_length << ")\n";
            std::cout << "  Using two-stage pipeline: VCF→EDS→l-EDS\n";
        } else {
            std::cout << "VCF → EDS transformation\n";
        }
        std::cout << "  Input: " << input_file << "\n";
        std::cout << "  Reference: " << reference_file << "\n";
        if (compressed) std::cout << "  Compression: VCF " << vcf_in.describe() << ", reference " << fasta_in.describe() << "\n";
        if (one_chrom) std::cout << "  Contig: " << chrom << "\n";
        if (all_chroms) {
            std::cout << "  Contigs: every reference record with VCF records\n";
            const std::filesystem::path dir = opts.has("output-dir") ? std::filesystem::path(opts.get("output-dir")) : input_file.parent_path();
            const bool ok = transform_all_contigs(vcf_in, fasta_in, compressed, named_file.stem().string(), dir.empty() ? std::filesystem::path(".") : dir,
                                                  context_length);
            tool::print_performance(timer);
            return ok ? 0 : 1;
        }

        VCFStats stats;
        detail::Buf eds_out, seds_out;
        edsx_vcf_stats cst{};
        auto take_stats = [&] {
            stats.total_variants = cst.total_variants; stats.processed_variants = cst.processed_variants;
            stats.skipped_malformed = cst.skipped_malformed; stats.skipped_unsupported_sv = cst.skipped_unsupported_sv;
            stats.variant_groups = cst.variant_groups;
        };
        if (ngpu) {
            // N rank threads inside the library, one per GPU (devices 0 .. N-1): reference-position ranges, RCCL exchanges
            std::vector<int> devs(ngpu);
            for (unsigned long i = 0; i < ngpu; i++) devs[i] = static_cast<int>(i);
            edsx_multi* mg = nullptr;
            if (edsx_multi_create(devs.data(), static_cast<int>(ngpu), 1, &mg) != EDSX_OK)
                throw std::runtime_error("cannot use " + std::to_string(ngpu) + " GPUs (gfx950 devices 0.." + std::to_string(ngpu - 1) + " with RCCL)");
            // BGZF inputs are inflated on GPU 0 and handed over as text
            detail::Buf vtext, ftext;
            const uint8_t* vp = vcf_in.data; size_t vn = vcf_in.size;
            const uint8_t* fp = fasta_in.data; size_t fn = fasta_in.size;
            auto inflate0 = [&](const tool::GzInput& z, detail::Buf& t, const uint8_t*& p, size_t& n) {
                if (z.kind != 1) return;
                edsx_ctx* ctx = detail::context();
                const int zrc = edsx_gz_inflate(ctx, z.data, z.size, &t.b);
                if (zrc != EDSX_OK) { edsx_multi_destroy(mg); detail::throw_status(zrc, ctx); }
                p = t.b.data ? t.b.data : reinterpret_cast<const uint8_t*>(""); n = t.b.size;
            };
            inflate0(vcf_in, vtext, vp, vn);
            inflate0(fasta_in, ftext, fp, fn);
            const int rc = edsx_vcf_transform_multi(mg, vp, vn, fp, fn, context_length, &eds_out.b, &seds_out.b, &cst);
            const std::string what = rc != EDSX_OK ? edsx_multi_last_error(mg) : "";
            edsx_vcf_multi_info info{};
            edsx_multi_last_vcf(mg, &info);
            edsx_multi_destroy(mg);
            take_stats();
            if (rc != EDSX_OK) throw std::runtime_error(what);
            std::cout << "  GPUs: " << ngpu << (info.partitioned ? " (position ranges" + std::string(info.fasta_windowed ? ", FASTA windows" : "") + ")"
                                                                 : std::string(ngpu > 1 ? " (not partitioned: one GPU transforms the file)" : "")) << "\n";
        } else {
            edsx_ctx* ctx = detail::context();
            const int rc = compressed ? edsx_vcf_transform_z(ctx, vcf_in.data, vcf_in.size, fasta_in.data, fasta_in.size,
                                                             one_chrom ? chrom.c_str() : nullptr, context_length, &eds_out.b, &seds_out.b, &cst)
                         : one_chrom ? edsx_vcf_transform_contig(ctx, vcf_in.data, vcf_in.size, fasta_in.data, fasta_in.size,
                                                                 chrom.c_str(), context_length, &eds_out.b, &seds_out.b, &cst)
                                     : edsx_vcf_transform(ctx, vcf_in.data, vcf_in.size, fasta_in.data, fasta_in.size, context_length,
                                                          &eds_out.b, &seds_out.b, &cst);
            take_stats();
            if (rc != EDSX_OK) detail::throw_status(rc, ctx);
        }

        std::filesystem::path eds_path, seds_path;
        if (create_leds) {
            const std::string base = named_file.stem().string(), suffix = "_l" + std::to_string(context_length);
            eds_path = output_file.empty() ? input_file.parent_path() / (base + suffix + ".leds") : output_file;
            seds_path = sources_file.empty() ? eds_path.parent_path() / (base + suffix + ".seds") : sources_file;
        } else {
            eds_path = output_file.empty() ? input_file.parent_path() / (named_file.stem().string() + ".eds") : output_file;
            seds_path = sources_file.empty() ? eds_path.parent_path() / (eds_path.stem().string() + ".seds") : sources_file;
        }
        tool::write_bytes(eds_path, eds_out.b.data, eds_out.b.size, "output");
        tool::write_bytes(seds_path, seds_out.b.data, seds_out.b.size, "sources");

        std::cout << "Transformation complete!\n";
        std::cout << "  Output: " << eds_path << "\n";
        std::cout << "  Sources: " << seds_path << "\n";
        std::cout << "\n";
        print_statistics(stats);
        tool::print_performance(timer);
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "Error: " << e.what() << "\n";
        tool::print_performance(timer);
        return 1;
    }
}
