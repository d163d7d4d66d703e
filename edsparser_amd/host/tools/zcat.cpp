// edsx-zcat — inflate a gzip / BGZF file (BGZF blocks on the GPU), or print the block table of a BGZF file.
#include "gz_input.hpp"
#include "tool_front.hpp"

using namespace edsparser;

int main(int argc, char** argv)
{
    return tool::run([&] {
        cli::Parser opts("Inflate a gzip / BGZF file on the GPU");
        opts.add("help", 'h', false, false, "Show help message");
        opts.add("input", 'i', true, true, "Input file (.gz / .bgz, or plain: copied)");
        opts.add("output", 'o', true, false, "Output file (default: standard output)");
        opts.add("index", 0, false, false, "Print the BGZF block table as TSV instead: comp_off, out_off, comp_len, isize");
        opts.parse(argc, argv);
        if (opts.has("help")) {
            std::cout << "edsx-zcat - Inflate a gzip / BGZF file\n\n" << opts.usage() << "\n"
                      << "DESCRIPTION:\n"
                         "  BGZF (bgzip) files are inflated on the GPU, one wave per block, and every block's\n"
                         "  CRC-32 is checked there.  Any other gzip file is inflated on the host, on one thread.\n"
                         "  --index needs no GPU: it reads the headers and trailers of the blocks only.\n\n";
            return;
        }
        opts.notify();
        const std::filesystem::path input_file = opts.get("input");
        tool::MappedFile in(input_file, "input");
        if (opts.has("index")) {
            detail::Buf blocks;
            uint64_t text_size = 0;
            if (edsx_bgzf_index(in.data(), in.size(), &blocks.b, &text_size) != EDSX_OK) throw std::runtime_error("Not a BGZF file: " + input_file.string());
            const edsx_bgzf_block* b = reinterpret_cast<const edsx_bgzf_block*>(blocks.b.data);
            std::cout << "#comp_off\tout_off\tcomp_len\tisize\n";
            for (size_t i = 0; i < blocks.b.size / sizeof(edsx_bgzf_block); i++)
                std::cout << b[i].comp_off << "\t" << b[i].out_off << "\t" << b[i].comp_len << "\t" << b[i].isize << "\n";
            return;
        }
        tool::GzInput z(in, "input", false);
        detail::Buf text;
        const uint8_t* out = z.data;
        size_t n = z.size;
        if (z.kind == 1) {
            edsx_ctx* ctx = detail::context();
            const int rc = edsx_gz_inflate(ctx, z.data, z.size, &text.b);
            if (rc != EDSX_OK) detail::throw_status(rc, ctx);
            out = text.b.data; n = text.b.size;
        }
        if (opts.has("output")) tool::write_bytes(opts.get("output"), out, n, "output");
        else std::cout.write(reinterpret_cast<const char*>(out), static_cast<std::streamsize>(n));
        std::cerr << "  Compression: " << z.describe() << "\n";
    });
}
