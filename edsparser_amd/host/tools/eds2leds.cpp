// eds2leds — EDS -> l-EDS; LINEAR (phasing-aware) when --sources is given, else CARTESIAN.
// Flags, validation, naming and messages: src/cpp/tools/eds2leds.cpp:38-46, :98-124, :161-162, :176-196.
#include "edsparser/transforms/eds_transforms.hpp"
#include "edsx.h"
#include "../cli_util.hpp"
#include "../device.hpp"
#include "tool_common.hpp"

#include <memory>
#include <vector>

using namespace edsparser;

int main(int argc, char** argv)
{
    Timer timer;
    timer.start();
    try {
        cli::Parser opts("Transform EDS to l-EDS (length-constrained EDS)");
        opts.add("help", 'h', false, false, "Show help message");
        opts.add("input", 'i', true, true, "Input EDS file (.eds)");
        opts.add("output", 'o', true, false, "Output l-EDS file (default: <input>_l<N>.leds)");
        opts.add("context-length", 'l', true, true, "Minimum context length");
        opts.add("sources", 's', true, false, "Input source file (.seds) for linear (phasing-aware) merging");
        opts.add("full", 0, false, false, "Use full output format with brackets on all symbols (default: compact)");
        opts.add("threads", 't', true, false, "Number of threads for parallel processing");
        opts.add("gpus", 'g', true, false, "Spread the symbols over this many GPUs of the node by symbol range (RCCL exchanges; default 1)");
        opts.parse(argc, argv);
        if (opts.has("help")) {
            std::cout << "eds2leds - Transform EDS to l-EDS (length-constrained EDS)\n\n" << opts.usage() << "\n"
                      << "MERGING METHODS (auto-detected):\n"
                         "  WITH sources (-s):  phasing-aware (linear) merging\n"
                         "  WITHOUT sources:    all-combinations (cartesian) merging\n\n"
                         "OUTPUT MODES:\n"
                         "  Default (compact): ACGT{A,ACA}CGT      --full: {ACGT}{A,ACA}{CGT}\n\n"
                         "OUTPUT FILES:\n"
                         "  <input_base>_l<N>.leds, and <input_base>_l<N>.seds with sources\n\n"
                         "EXAMPLES:\n"
                         "  eds2leds -i in.eds -s in.seds -l 32            # in_l32.leds + in_l32.seds\n"
                         "  eds2leds -i in.eds -s in.seds -l 32 --gpus 8   # symbol ranges on GPUs 0..7, over RCCL\n\n";
            tool::print_performance(timer);
            return 0;
        }
        opts.notify();
        const unsigned long ngpu = opts.has("gpus") ? opts.get_unsigned("gpus", 1) : 0;
        if (opts.has("gpus") && (ngpu == 0 || ngpu > 64)) throw std::runtime_error("--gpus must be between 1 and 64");
        const std::filesystem::path input_file = opts.get("input");
        std::filesystem::path output_file = opts.get("output");
        const std::filesystem::path sources_file = opts.get("sources");
        const Length context_length = static_cast<Length>(opts.get_unsigned("context-length", 0));
        const long num_threads = opts.get_int("threads", 1);
        const bool compact_mode = !opts.has("full");

        if (input_file.extension() != ".eds") {
            std::cerr << "Error: Input file must be an EDS file (.eds)\n";
            std::cerr << "Got: " << input_file << "\n";
            tool::print_performance(timer);
            return 1;
        }
        if (num_threads < 1) {
            std::cerr << "Error: Number of threads must be >= 1\n";
            tool::print_performance(timer);
            return 1;
        }
        if (context_length == 0) {
            std::cerr << "Error: Context length must be > 0\n";
            tool::print_performance(timer);
            return 1;
        }
        if (output_file.empty())
            output_file = input_file.parent_path() / (input_file.stem().string() + "_l" + std::to_string(context_length) + ".leds");

        std::cout << "EDS → l-EDS transformation\n";
        std::cout << "  Input: " << input_file << "\n";
        std::cout << "  Output: " << output_file << "\n";
        std::cout << "  Context length: " << context_length << "\n";
        if (!sources_file.empty()) std::cout << "  Sources: " << sources_file << "\n";
        std::cout << "  Output mode: " << (compact_mode ? "compact" : "full") << "\n";
        std::cout << "  Threads: " << num_threads << (num_threads == 1 ? " (sequential)" : " (parallel)") << "\n";

        if (ngpu) {
            // both files are mapped and handed to the C ABI as they are; N rank threads inside the library, one per GPU
            // (devices 0 .. N-1): symbol ranges, RCCL exchanges
            tool::MappedFile eds_in(input_file, "EDS");
            std::unique_ptr<tool::MappedFile> seds_in;
            if (!sources_file.empty()) seds_in.reset(new tool::MappedFile(sources_file, "sources"));
            std::vector<int> devs(ngpu);
            for (unsigned long i = 0; i < ngpu; i++) devs[i] = static_cast<int>(i);
            edsx_multi* mg = nullptr;
            if (edsx_multi_create(devs.data(), static_cast<int>(ngpu), 1, &mg) != EDSX_OK)
                throw std::runtime_error("cannot use " + std::to_string(ngpu) + " GPUs (gfx950 devices 0.." + std::to_string(ngpu - 1) + " with RCCL)");
            detail::Buf leds, seds_out;
            const int rc = edsx_leds_merge_multi(mg, eds_in.data(), eds_in.size(), seds_in ? seds_in->data() : nullptr,
                                                 seds_in ? seds_in->size() : 0, context_length, compact_mode ? 1 : 0, &leds.b, &seds_out.b);
            const std::string what = rc != EDSX_OK ? edsx_multi_last_error(mg) : "";
            edsx_merge_multi_info info{};
            edsx_multi_last_merge(mg, &info);
            edsx_multi_destroy(mg);
            if (rc != EDSX_OK) throw std::runtime_error(what);
            std::cout << "  GPUs: " << ngpu << (info.partitioned ? " (symbol ranges)" : " (not partitioned: one GPU merges the file)") << "\n";
            tool::write_bytes(output_file, leds.b.data, leds.b.size, "output");
            if (seds_in) {
                std::filesystem::path output_sources = output_file;
                output_sources.replace_extension(".seds");
                std::cout << "  Output sources: " << output_sources << "\n";
                tool::write_bytes(output_sources, seds_out.b.data, seds_out.b.size, "sources");
            }
            std::cout << "Transformation complete!\n";
            tool::print_performance(timer);
            return 0;
        }

        std::ifstream input(input_file);
        if (!input) throw std::runtime_error("Cannot open input file: " + input_file.string());
        std::ofstream output(output_file);
        if (!output) throw std::runtime_error("Cannot open output file: " + output_file.string());

        std::unique_ptr<std::ifstream> sources_in;
        std::unique_ptr<std::ofstream> sources_out;
        if (!sources_file.empty()) {
            sources_in.reset(new std::ifstream(sources_file));
            if (!*sources_in) throw std::runtime_error("Cannot open sources file: " + sources_file.string());
            std::filesystem::path output_sources = output_file;
            output_sources.replace_extension(".seds");
            sources_out.reset(new std::ofstream(output_sources));
            if (!*sources_out) throw std::runtime_error("Cannot create output sources file: " + output_sources.string());
            std::cout << "  Output sources: " << output_sources << "\n";
        }
        if (sources_in)
            eds_to_leds_linear(input, output, context_length, sources_in.get(), sources_out.get(),
                               static_cast<size_t>(num_threads), compact_mode);
        else
            eds_to_leds_cartesian(input, output, context_length, static_cast<size_t>(num_threads), compact_mode);

        std::cout << "Transformation complete!\n";
        tool::print_performance(timer);
        return 0;
    } catch (const std::exception& e) {
        std::cerr << "Error: " << e.what() << "\n";
        tool::print_performance(timer);
        return 1;
    }
}
