// test_div_shim — edsparser::path_diversity, built by tests/test_div_cpu.py and driven by tests/test_div_gpu.py (needs the GPU).
// One command per line of the file given as argv[1], tab separated; one answer line per command:
//   D <eds> <seds> <groups a,b;c,d;..|-> <unit symbols|columns> <size> <step>
//       ->  the windows, each as its four integers separated by commas and closed by ';', '#', the group records the same
//           way, '#', the pair records, '#', the spectrum bins each followed by a comma, '#', groups, paths, choice symbols,
//           windows, extent
// An exception answers <kind>:<what>.
#include "edsparser/transforms/eds_transforms.hpp"

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace edsparser;

static std::vector<std::string> split(const std::string& line, char sep)
{
    std::vector<std::string> f;
    size_t pos = 0;
    while (true) {
        const size_t end = line.find(sep, pos);
        f.push_back(line.substr(pos, end == std::string::npos ? std::string::npos : end - pos));
        if (end == std::string::npos) break;
        pos = end + 1;
    }
    return f;
}

static std::string answer(const std::vector<std::string>& f)
{
    if (f.size() < 7 || f[0] != "D") return "bad_command:";
    std::istringstream eds(f[1]), seds(f[2]);
    std::vector<std::vector<int>> groups;
    if (f[3] != "-")
        for (const auto& g : split(f[3], ';')) {
            groups.emplace_back();
            if (!g.empty()) for (const auto& t : split(g, ',')) groups.back().push_back(std::stoi(t));
        }
    DiversityOptions o;
    o.unit = f[4] == "columns" ? DiversityUnit::COLUMNS : DiversityUnit::SYMBOLS;
    o.size = std::stoull(f[5]); o.step = std::stoull(f[6]); o.sfs = true;
    const PathDiversity d = path_diversity(eds, seds, groups, o);
    std::string text;
    for (const DiversityWindow& w : d.windows)
        text += std::to_string(w.start) + ',' + std::to_string(w.end) + ',' + std::to_string(w.rank_first) + ',' + std::to_string(w.rank_end) + ';';
    text += '#';
    for (const DiversityGroup& g : d.groups) text += std::to_string(g.segregating) + ',' + std::to_string(g.present) + ';';
    text += '#';
    for (const DiversityPair& p : d.pairs) text += std::to_string(p.diff) + ',' + std::to_string(p.comp) + ';';
    text += '#';
    for (const auto& s : d.sfs) for (uint64_t v : s) text += std::to_string(v) + ',';
    return text + '#' + std::to_string(d.n_groups) + ',' + std::to_string(d.paths) + ',' + std::to_string(d.choice_symbols) + ',' +
           std::to_string(d.windows.size()) + ',' + std::to_string(d.extent);
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::cerr << "usage: test_div_shim <commands>\n"; return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::cerr << "cannot open " << argv[1] << "\n"; return 2; }
    for (std::string line; std::getline(in, line);) {
        std::string out;
        try { out = answer(split(line, '\t')); }
        catch (const std::invalid_argument& e) { out = std::string("invalid_argument:") + e.what(); }
        catch (const std::out_of_range& e) { out = std::string("out_of_range:") + e.what(); }
        catch (const std::exception& e) { out = std::string("runtime_error:") + e.what(); }
        std::cout << out << "\n";
    }
    return 0;
}
