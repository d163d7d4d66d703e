// test_ibs_shim — edsparser::path_ibs, driven by tests/test_ibs_gpu.py (needs the GPU).
// One command per line of the file given as argv[1], tab separated; one answer line per command:
//   I <eds> <seds> <paths a,b,..|-> <min_sites> <min_columns> <max_segments>
//       ->  the records, each as its seven integers separated by commas and closed by ';', then '#', pair_off separated by
//           commas, '#', paths, choice symbols, candidate segments
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
    if (f.size() < 7 || f[0] != "I") return "bad_command:";
    std::istringstream eds(f[1]), seds(f[2]);
    std::vector<int> paths;
    if (f[3] != "-") for (const auto& t : split(f[3], ',')) paths.push_back(std::stoi(t));
    IbsOptions o;
    o.min_sites = std::stoull(f[4]); o.min_columns = std::stoull(f[5]); o.max_segments = std::stoull(f[6]);
    const PathIbs d = path_ibs(eds, seds, paths, o);
    std::string text;
    for (const IbsSegment& s : d.segments) {
        for (uint64_t v : {s.x, s.y, s.symbol_first, s.symbol_last, s.sites, s.column_first}) text += std::to_string(v) + ',';
        text += std::to_string(s.column_end) + ';';
    }
    text += '#';
    for (size_t k = 0; k < d.pair_off.size(); k++) text += (k ? "," : "") + std::to_string(d.pair_off[k]);
    return text + '#' + std::to_string(d.paths) + ',' + std::to_string(d.choice_symbols) + ',' + std::to_string(d.candidate_segments);
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::cerr << "usage: test_ibs_shim <commands>\n"; return 2; }
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
