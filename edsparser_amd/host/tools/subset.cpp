// edsparser-subset — restrict an EDS with sources to a chosen set of its paths, on the GPU (edsx_eds_subset).
// The result is again an .eds (FULL form) + .seds: one population out of a panel, a training / held-out split, "these 20
// assemblies only".  Every kept path spells the sequence it spelled before (eds2fasta).  Banner, "[Performance]" line and
// exit codes in the style of the other tools.
#include "tool_front.hpp"

#include <algorithm>

using namespace edsparser;

int main(int argc, char** argv)
{
    return tool::run([&] {
        cli::Parser opts("Restrict an EDS with sources to a set of paths");
        opts.add("help", 'h', false, false, "Show help message");
        opts.add("input", 'i', true, true, "Input EDS file (.eds / .leds)");
        opts.add("sources", 's', true, false, "Input source file (default: <input> with the .seds extension)");
        opts.add("output", 'o', true, false, "Output EDS file (default: <input stem>_subset.eds); the sources go beside it as .seds");
        opts.add("paths", 'p', true, false, "Path ids and ranges to keep, e.g. 1,5,7-9");
        opts.add("paths-file", 0, true, false, "File with one path id per line");
        opts.add("exclude", 0, false, false, "Keep every path of 1..P that is NOT listed");
        opts.add("keep-ids", 0, false, false, "Leave the path ids as they are (default: renumber 1..|K|)");
        opts.add("names", 0, true, false, "File whose line k names path k");
        opts.add("names-out", 0, true, false, "Receives the names of the kept paths in new-id order (for eds2fasta --names)");
        opts.parse(argc, argv);
        if (opts.has("help")) {
            std::cout << "edsparser-subset - restrict an EDS to a chosen set of paths\n\n" << opts.usage() << "\n"
                      << "A string is kept when its source set holds 0 or a kept path.  Symbols without a kept string go;\n"
                         "symbols left with one string that every kept path takes are joined with their neighbours.\n"
                         "The output is always in FULL form (braces around every symbol).\n\n"
                         "EXAMPLES:\n"
                         "  edsparser-subset -i in.eds -p 1,5,7-9          # in.seds -> in_subset.eds + in_subset.seds\n"
                         "  edsparser-subset -i in.eds --paths-file held_out.txt --exclude -o train.eds\n\n";
            return;
        }
        opts.notify();
        const tool::Files f = tool::files(opts, "_subset.eds");
        std::filesystem::path sources_out = f.output;
        sources_out.replace_extension(".seds");
        const bool exclude = opts.has("exclude"), keep_ids = opts.has("keep-ids");
        tool::need_files(f, false, "Path subsetting");
        if (opts.has("paths") && opts.has("paths-file")) tool::fail("--paths and --paths-file exclude each other");
        if (!opts.has("paths") && !opts.has("paths-file")) tool::fail("One of --paths and --paths-file is required");
        if (opts.has("names") != opts.has("names-out")) tool::fail("--names and --names-out go together");
        if (opts.has("names") && keep_ids) tool::fail("--names-out lists the names in new-id order: it does not go with --keep-ids");
        std::vector<uint64_t> ids = tool::path_list(opts, "paths");
        if (!opts.has("paths")) {
            size_t no = 0;
            for (const std::string& line : tool::read_lines(opts.get("paths-file"), "Cannot open paths file")) {
                no++;
                if (line.empty()) continue;
                size_t used = 0;
                unsigned long long v = 0;
                if (line[0] >= '0' && line[0] <= '9') { try { v = std::stoull(line, &used); } catch (...) { used = 0; } }
                if (used != line.size()) tool::fail("Paths file line " + std::to_string(no) + " is not a path id");
                ids.push_back(v);
            }
        }

        std::cout << "EDS path subsetting\n";
        std::cout << "  Input: " << f.input << "\n";
        std::cout << "  Sources: " << f.sources << "\n";
        std::cout << "  Output: " << f.output << "\n";
        std::cout << "  Output sources: " << sources_out << "\n";

        edsx_ctx* ctx = detail::context();
        const tool::MappedFile eds(f.input, "input"), seds(f.sources, "sources");
        if (exclude) {                                           // the complement within 1..P; P, the largest id of the
            uint64_t P = 0, cur = 0;                             // .seds, is read off the text (the library checks the text)
            for (size_t k = 0; k <= seds.size(); k++) {
                const uint8_t c = k < seds.size() ? seds.data()[k] : 0;
                if (c >= '0' && c <= '9') cur = cur > (1ull << 40) ? cur : cur * 10 + (c - '0');
                else { P = std::max(P, cur); cur = 0; }
            }
            if (P > (1ull << 31)) tool::fail("The sources name a path id above 2^31");
            std::vector<bool> drop(P + 1, false);
            for (uint64_t p : ids) {                             // (not tool::resolve_paths: per id, this check comes before the next one)
                if (p == 0 || p > P) tool::fail("Path id " + std::to_string(p) + " out of range (1.." + std::to_string(P) + ")");
                if (drop[p]) tool::fail("Path id " + std::to_string(p) + " given twice");
                drop[p] = true;
            }
            ids.clear();
            for (uint64_t p = 1; p <= P; p++) if (!drop[p]) ids.push_back(p);
        }
        detail::Buf e, s;
        edsx_subset_info info;
        tool::check(ctx, edsx_eds_subset(ctx, eds.data(), eds.size(), seds.data(), seds.size(), ids.data(), ids.size(), keep_ids ? 1 : 0, &e.b, &s.b, &info));
        tool::write_bytes(f.output, e.b.data, e.b.size, "output");
        tool::write_bytes(sources_out, s.b.data, s.b.size, "output sources");
        if (opts.has("names")) {
            const tool::Names table(opts, "");
            std::vector<uint64_t> kept(ids);
            std::sort(kept.begin(), kept.end());                 // new id = rank in ascending order
            std::string text;
            for (uint64_t p : kept) text += table.name_of(p) + "\n";
            tool::write_file(opts.get("names-out"), text, "names output");
        }
        std::cout << "  Paths: " << info.paths_in << " -> " << info.paths_out << ", symbols: " << info.symbols_in << " -> " << info.symbols_out
                  << " (" << info.symbols_removed << " removed, " << info.common_runs_merged << " common runs merged), strings: "
                  << info.strings_in << " -> " << info.strings_out << ", characters: " << info.chars_in << " -> " << info.chars_out << "\n";
        std::cout << "Subsetting complete!\n";
    });
}
