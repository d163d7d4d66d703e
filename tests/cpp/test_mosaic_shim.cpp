// test_mosaic_shim — edsparser::path_mosaic, driven by tests/test_mosaic_gpu.py (needs the GPU).
// One command per line of the file given as argv[1], tab separated; one answer line per command:
//   M <eds> <seds> <targets a,b,..|-> <donors a,b,..|-> <max_segments>
//       ->  the records, each as its seven integers separated by commas and closed by ';', then '#', target_off separated by
//           commas, '#', targets, donors, choice symbols, private segments, private symbols, switches
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
    if (f.size() < 6 || f[0] != "M") return "bad_command:";
    std::istringstream eds(f[1]), seds(f[2]);
    std::vector<int> targets, donors;
    if (f[3] != "-") for (const auto& t : split(f[3], ',')) targets.push_back(std::stoi(t));
    if (f[4] != "-") for (const auto& t : split(f[4], ',')) donors.push_back(std::stoi(t));
    MosaicOptions o;
    o.max_segments = std::stoull(f[5]);
    const PathMosaic d = path_mosaic(eds, seds, targets, donors, o);
    std::string text;
    for (const MosaicSegment& s : d.segments) {
        for (uint64_t v : {s.target, s.donor, s.symbol_first, s.symbol_last, s.sites, s.column_first}) text += std::to_string(v) + ',';
        text += std::to_string(s.column_end) + ';';
    }
    text += '#';
    for (size_t k = 0; k < d.target_off.size(); k++) text += (k ? "," : "") + std::to_string(d.target_off[k]);
    text += '#';
    const size_t numbers[] = {d.targets, d.donors, d.choice_symbols, d.private_segments, d.private_symbols, d.switches};
    for (size_t k = 0; k < 6; k++) text += (k ? "," : "") + std::to_string(numbers[k]);
    return text;
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::cerr << "usage: test_mosaic_shim <commands>\n"; return 2; }
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
