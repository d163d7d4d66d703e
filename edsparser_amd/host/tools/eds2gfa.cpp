// eds2gfa — write an EDS, and the paths of its sources when it has them, as a GFA 1.0 graph, on the GPU
// (edsx_eds_gfa_graph, edsx_paths_gfa_walks).  Every non-empty string becomes a segment, adjacent symbols are fully
// linked (across symbols that hold an empty string), every path becomes a P line: the way from msa2eds / vcf2eds to graph
// viewers, vg-style toolchains and graph aligners.  Banner, "[Performance]" line and exit codes in the style of the other
// tools.  The graph is written first; the walks are appended in batches (--batch-mb), so host memory stays bounded.
#include "tool_front.hpp"

#include <algorithm>

using namespace edsparser;

int main(int argc, char** argv)
{
    return tool::run([&] {
        cli::Parser opts("Write an EDS and its paths as a GFA 1.0 graph");
        opts.add("help", 'h', false, false, "Show help message");
        opts.add("input", 'i', true, true, "Input EDS file (.eds / .leds)");
        opts.add("sources", 's', true, false, "Input source file (default: <input> with the .seds extension, if it exists)");
        opts.add("no-paths", 0, false, false, "Write the graph alone, even when there are sources");
        opts.add("output", 'o', true, false, "Output GFA file (default: <input stem>.gfa)");
        opts.add("paths", 'p', true, false, "Path ids and ranges, e.g. 1,5,7-9 (default: all paths)");
        opts.add("names", 0, true, false, "File whose line k names path k (default: <prefix><id>)");
        opts.add("prefix", 0, true, false, "Path name prefix (default: path)");
        opts.add("max-links", 0, true, false, "Refuse a graph of more links than this (default: 4294967296)");
        opts.add("batch-mb", 0, true, false, "Megabytes of P lines per batch (default: 4096)");
        opts.parse(argc, argv);
        if (opts.has("help")) {
            std::cout << "eds2gfa - an EDS and its paths as a GFA 1.0 graph\n\n" << opts.usage() << "\n"
                      << "Segments are the non-empty strings, numbered from 1 in file order.  The segments of a symbol are\n"
                         "linked to those of the next symbols up to and including the first one without an empty string.\n"
                         "A path lists the segments of the strings it takes; a path that takes only empty strings has no line.\n\n"
                         "EXAMPLES:\n"
                         "  eds2gfa -i in.eds                       # in.seds, if there, -> in.gfa with one P line per path\n"
                         "  eds2gfa -i in.eds --no-paths -o graph.gfa\n"
                         "  eds2gfa -i in.eds -p 1,5,7-9 --names samples.txt\n\n";
            return;
        }
        opts.notify();
        const tool::Files f = tool::files(opts, ".gfa");
        const bool no_paths = opts.has("no-paths");
        const unsigned long batch_mb = opts.get_unsigned("batch-mb", 4096);
        const unsigned long long max_links = opts.get_unsigned("max-links", 0);
        if (batch_mb == 0) tool::fail("--batch-mb must be > 0");
        tool::need_input(f);
        if (no_paths && (f.sources_given || opts.has("paths") || opts.has("names"))) tool::fail("--no-paths does not go with --sources, --paths or --names");
        const bool with_paths = !no_paths && std::filesystem::exists(f.sources);
        if (!no_paths && !with_paths && f.sources_given) tool::fail("Sources file does not exist: " + f.sources.string());
        if (!with_paths && (opts.has("paths") || opts.has("names"))) tool::fail("--paths and --names need sources (.seds): " + f.sources.string() + " does not exist");
        std::vector<uint64_t> ids = tool::path_list(opts, "paths");

        std::cout << "EDS → GFA export\n";
        std::cout << "  Input: " << f.input << "\n";
        if (with_paths) std::cout << "  Sources: " << f.sources << "\n";
        std::cout << "  Output: " << f.output << "\n";

        edsx_ctx* ctx = detail::context();
        const tool::MappedFile eds(f.input, "input");
        tool::Session ses;
        if (with_paths) ses.open(eds, f.sources);                // first: a text that does not match its sources writes nothing
        std::ofstream out;
        uint64_t total = 0;
        edsx_gfa_info info;
        {
            detail::Buf graph;
            tool::check(ctx, edsx_eds_gfa_graph(ctx, eds.data(), eds.size(), max_links, &graph.b, &info));
            out.open(f.output, std::ios::binary);
            if (!out) tool::fail("Cannot open output file: " + f.output.string());
            out.write(reinterpret_cast<const char*>(graph.b.data), static_cast<std::streamsize>(graph.b.size));
            if (!out) tool::fail("Cannot write output file: " + f.output.string());
            total = graph.b.size;
        }
        std::cout << "  Symbols: " << info.n_symbols << " (" << info.n_open_symbols << " with an empty string), strings: " << info.n_strings
                  << "\n  Segments: " << info.n_segments << ", links: " << info.n_links << "\n";

        uint64_t lines = 0, batches = 0, off_graph = 0;
        if (with_paths) {
            if (ids.empty()) ids = tool::all_paths(ses.info.num_paths);
            const tool::Names table(opts, "path");
            std::vector<std::string> name_text;
            if (table.given) name_text = table.names_of(ids);
            const std::vector<const char*> names = tool::c_strs(name_text);
            // a line has at most 12 bytes per symbol ("<ten digits>+,") behind its name
            const uint64_t per_path = 12 * ses.info.n_symbols + 256, budget = static_cast<uint64_t>(batch_mb) << 20;
            const size_t per_batch = static_cast<size_t>(std::max<uint64_t>(1, budget / per_path));
            std::vector<uint64_t> miss(ids.size()), steps(ids.size());
            for (size_t k0 = 0; k0 < ids.size(); k0 += per_batch) {
                const size_t k1 = std::min(ids.size(), k0 + per_batch);
                detail::Buf text;
                ses.check(edsx_paths_gfa_walks(ses.s, ids.data() + k0, k1 - k0, names.empty() ? nullptr : names.data() + k0, table.prefix.c_str(),
                                               &text.b, miss.data() + k0, steps.data() + k0));
                out.write(reinterpret_cast<const char*>(text.b.data), static_cast<std::streamsize>(text.b.size));
                if (!out) tool::fail("Cannot write output file: " + f.output.string());
                total += text.b.size;
                batches++;
            }
            for (size_t k = 0; k < ids.size(); k++) {
                if (steps[k]) lines++;
                else std::cerr << "Warning: path " << ids[k] << " takes no non-empty string and has no P line\n";
                if (miss[k]) off_graph++;
            }
            if (off_graph)
                std::cerr << "Warning: " << off_graph << (off_graph == 1 ? " path has" : " paths have")
                          << " no string in some symbol: consecutive steps of such a path may not be linked\n";
            std::cout << "  Paths written: " << lines << " of " << ids.size() << " in " << batches << (batches == 1 ? " batch" : " batches") << "\n";
        }
        std::cout << "  Bytes written: " << total << "\n";
        std::cout << "Export complete!\n";
    });
}
