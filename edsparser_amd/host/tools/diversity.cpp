// edsparser-diversity — windowed diversity within and between groups of paths of an EDS with sources, on the GPU
// (edsx_paths_diversity): per window of choice symbols or alignment columns the segregating sites, pi, Watterson's theta and
// Tajima's D of every group, and d_xy and Hudson's F_ST of every two groups; on request the unfolded site frequency spectrum
// of every group.  The library returns integer sums; the statistics are derived on the host (div_stats.hpp) and the texts
// are written here:
//   output         "start end sites group paths segregating present diff comp pi theta_w tajima_d", one line per (window, group)
//   <output>.pairs "start end sites group_a group_b diff comp dxy fst", one line per (window, g < h); with two groups or more
//   --sfs          "group count sites": the strings j >= 1 of the complete choice symbols by the paths of the group that take them
// tab separated, floats as %.6g, NA where a denominator is zero.  Banner, "[Performance]" line and exit codes in the style of
// the other tools.
#include "tool_front.hpp"
#include "../div_stats.hpp"

#include <algorithm>
#include <cstdio>
#include <map>
#include <vector>

using namespace edsparser;

namespace {

struct Groups {
    std::vector<std::string> names;
    std::vector<std::vector<uint64_t>> ids;
    size_t find_or_add(const std::string& name)
    {
        for (size_t g = 0; g < names.size(); g++) if (names[g] == name) return g;
        if (name.empty() || name.find_first_of("\t \n") != std::string::npos) tool::fail("A group name is empty or holds a tab, blank or line feed");
        names.push_back(name);
        ids.emplace_back();
        return names.size() - 1;
    }
};

std::string number(bool defined, double v)
{
    if (!defined) return "NA";
    char buf[64];
    std::snprintf(buf, sizeof(buf), "%.6g", v);
    return buf;
}

} // namespace

int main(int argc, char** argv)
{
    return tool::run([&] {
        cli::Parser opts("Windowed diversity within and between groups of paths of an EDS with sources");
        opts.add("help", 'h', false, false, "Show help message");
        opts.add("input", 'i', true, true, "Input EDS file (.eds / .leds)");
        opts.add("sources", 's', true, false, "Input source file (default: <input> with the .seds extension)");
        opts.add("output", 'o', true, false, "Output file (default: <input stem>.div); pairs of groups go to <output>.pairs");
        opts.add("group", 'g', true, false, "A group as NAME=LIST, e.g. east=1,5,7-9; may repeat (default: one group 'all' of all paths)");
        opts.add("groups", 0, true, false, "Groups from a file of lines path<TAB>group");
        opts.add("names", 0, true, false, "File whose line k names path k: --groups then lists paths by these names");
        opts.add("unit", 0, true, false, "Window coordinates: symbols (choice symbols) or columns (default: symbols)");
        opts.add("window", 0, true, false, "Window size, 0 = one window over everything (default: 0)");
        opts.add("step", 0, true, false, "Distance between window starts, 0 = the window size (default: 0)");
        opts.add("max-windows", 0, true, false, "Refuse more windows than this, 0 = no limit (default: 0)");
        opts.add("sfs", 0, true, false, "Write the site frequency spectrum of every group to this file");
        opts.parse(argc, argv);
        if (opts.has("help")) {
            std::cout << "edsparser-diversity - pi, theta, Tajima's D, d_xy and F_ST per window of an EDS\n\n" << opts.usage() << "\n"
                      << "A path carries the first string of a symbol, in file order, that names it; equal texts are not merged.\n"
                         "Two paths are compared at a choice symbol when both have a string there.  Tajima's D is given for the\n"
                         "windows in which no path of the group lacks a string; NA marks a zero denominator.\n\n"
                         "EXAMPLES:\n"
                         "  edsparser-diversity -i in.eds --window 1000 --step 500                 # in.seds -> in.div\n"
                         "  edsparser-diversity -i in.eds -g a=1-50 -g b=51-100 --unit columns --window 10000 --sfs in.sfs -o ab.div\n\n";
            return;
        }
        opts.notify();
        const tool::Files f = tool::files(opts, ".div");
        edsx_div_opts o;
        const std::string unit = opts.get("unit", "symbols");
        if (unit != "symbols" && unit != "columns") tool::fail("the argument ('" + unit + "') for option '--unit' is invalid");
        o.unit = unit == "columns" ? EDSX_DIV_COLUMNS : EDSX_DIV_SYMBOLS;
        o.size = opts.get_unsigned("window", 0);
        o.step = opts.get_unsigned("step", 0);
        o.max_windows = opts.get_unsigned("max-windows", 0);
        Groups groups;
        for (const auto& gv : opts.given()) {
            if (gv.first != "group") continue;
            const size_t eq = gv.second.find('=');
            if (eq == std::string::npos || eq == 0) tool::fail("the argument ('" + gv.second + "') for option '--group' is invalid");
            const size_t g = groups.find_or_add(gv.second.substr(0, eq));
            for (uint64_t p : tool::parse_paths(gv.second.substr(eq + 1), "group")) groups.ids[g].push_back(p);
        }
        tool::need_files(f);
        if (opts.has("groups")) {
            std::map<std::string, uint64_t> by_name;
            if (opts.has("names")) {
                const std::vector<std::string> lines = tool::read_lines(opts.get("names"), "Cannot open names file");
                for (size_t k = 0; k < lines.size(); k++) by_name[lines[k]] = k + 1;
            }
            for (const std::string& line : tool::read_lines(opts.get("groups"), "Cannot open groups file")) {
                if (line.empty()) continue;
                const size_t tab = line.find('\t');
                if (tab == std::string::npos || tab == 0) tool::fail("A line of the groups file is not path<TAB>group: " + line);
                const std::string path = line.substr(0, tab);
                uint64_t p;
                if (opts.has("names")) {
                    const auto it = by_name.find(path);
                    if (it == by_name.end()) tool::fail("The names file has no path named " + path);
                    p = it->second;
                } else {
                    const std::vector<uint64_t> one = tool::parse_paths(path, "groups");
                    if (one.size() != 1) tool::fail("A line of the groups file is not path<TAB>group: " + line);
                    p = one[0];
                }
                groups.ids[groups.find_or_add(line.substr(tab + 1))].push_back(p);
            }
        }
        std::vector<uint64_t> off(1, 0), ids;
        for (const auto& g : groups.ids) {
            ids.insert(ids.end(), g.begin(), g.end());
            off.push_back(ids.size());
        }
        const size_t n_groups = groups.names.size();
        if (n_groups == 0) groups.names.push_back("all");

        std::cout << "EDS diversity\n";
        std::cout << "  Input: " << f.input << "\n";
        std::cout << "  Sources: " << f.sources << "\n";
        std::cout << "  Output: " << f.output << "\n";
        std::cout << "  Groups: " << groups.names.size() << ", unit: " << unit << ", window: " << o.size << ", step: " << o.step << "\n";

        tool::Session ses(f);
        detail::Buf wb, gb, pb, fb;
        edsx_div_info di;
        ses.check(edsx_paths_diversity(ses.s, off.data(), ids.data(), n_groups, &o, &wb.b, &gb.b, &pb.b, opts.has("sfs") ? &fb.b : nullptr, &di));
        std::cout << "  Paths: " << di.paths << ", choice symbols: " << di.choice_symbols << ", extent: " << di.extent << ", windows: " << di.windows << "\n";

        const uint64_t G = di.groups, NP = di.pairs;
        std::vector<uint64_t> K(G, 0);
        if (n_groups == 0) K[0] = di.paths;
        for (size_t g = 0; g < n_groups; g++) {
            std::vector<uint64_t> u(groups.ids[g]);
            std::sort(u.begin(), u.end());
            K[g] = static_cast<uint64_t>(std::unique(u.begin(), u.end()) - u.begin());
        }
        std::vector<divstats::Harmonic> hs;
        for (uint64_t k : K) hs.push_back(divstats::harmonic(k));
        auto pair_at = [&](uint64_t g, uint64_t h) { return g * G - g * (g + 1) / 2 + h; };
        const edsx_div_window* w = reinterpret_cast<const edsx_div_window*>(wb.b.data);
        const edsx_div_group* gr = reinterpret_cast<const edsx_div_group*>(gb.b.data);
        const edsx_div_pair* pr = reinterpret_cast<const edsx_div_pair*>(pb.b.data);
        std::string text = "start\tend\tsites\tgroup\tpaths\tsegregating\tpresent\tdiff\tcomp\tpi\ttheta_w\ttajima_d\n";
        std::string ptext = "start\tend\tsites\tgroup_a\tgroup_b\tdiff\tcomp\tdxy\tfst\n";
        for (uint64_t k = 0; k < di.windows; k++) {
            const uint64_t sites = w[k].rank_end - w[k].rank_first;
            const std::string head = std::to_string(w[k].start) + "\t" + std::to_string(w[k].end) + "\t" + std::to_string(sites) + "\t";
            std::vector<double> pi(G, 0.0);
            std::vector<char> has(G, 0);
            for (uint64_t g = 0; g < G; g++) {
                const edsx_div_group& a = gr[k * G + g];
                const edsx_div_pair& p = pr[k * NP + pair_at(g, g)];
                double th = 0.0, td = 0.0;
                has[g] = divstats::ratio(p.diff, p.comp, pi[g]) ? 1 : 0;
                const bool has_th = divstats::theta_w(a.segregating, hs[g], th);
                const bool has_td = divstats::tajima_d(K[g], a.segregating, p.diff, a.present, sites, hs[g], td);
                text += head + groups.names[g] + "\t" + std::to_string(K[g]) + "\t" + std::to_string(a.segregating) + "\t" + std::to_string(a.present) +
                        "\t" + std::to_string(p.diff) + "\t" + std::to_string(p.comp) + "\t" + number(has[g] != 0, pi[g]) + "\t" + number(has_th, th) +
                        "\t" + number(has_td, td) + "\n";
            }
            for (uint64_t g = 0; g < G; g++)
                for (uint64_t h = g + 1; h < G; h++) {
                    const edsx_div_pair& p = pr[k * NP + pair_at(g, h)];
                    double dxy = 0.0, fs = 0.0;
                    const bool has_xy = divstats::ratio(p.diff, p.comp, dxy);
                    const bool has_f = divstats::fst(has[g] != 0, pi[g], has[h] != 0, pi[h], has_xy, dxy, fs);
                    ptext += head + groups.names[g] + "\t" + groups.names[h] + "\t" + std::to_string(p.diff) + "\t" + std::to_string(p.comp) + "\t" +
                             number(has_xy, dxy) + "\t" + number(has_f, fs) + "\n";
                }
        }
        tool::write_bytes(f.output, reinterpret_cast<const uint8_t*>(text.data()), text.size(), "output");
        if (G >= 2) tool::write_bytes(f.output.string() + ".pairs", reinterpret_cast<const uint8_t*>(ptext.data()), ptext.size(), "pair");
        if (opts.has("sfs")) {
            std::string st = "group\tcount\tsites\n";
            const uint64_t* bins = reinterpret_cast<const uint64_t*>(fb.b.data);
            uint64_t at = 0;
            for (uint64_t g = 0; g < G && fb.b.size; g++)
                for (uint64_t c = 0; c <= K[g]; c++) st += groups.names[g] + "\t" + std::to_string(c) + "\t" + std::to_string(bins[at++]) + "\n";
            tool::write_bytes(opts.get("sfs"), reinterpret_cast<const uint8_t*>(st.data()), st.size(), "spectrum");
        }
        edsx_paths_timing t;
        edsx_paths_last_timing(ses.s, &t);
        std::cout << "  Device: sites " << t.copy_ms << " ms, scans and windows " << t.scan_ms << " ms\n";
        std::cout << "  Windows written: " << di.windows << ", " << text.size() << " bytes\n";
        std::cout << "Diversity complete!\n";
    });
}
