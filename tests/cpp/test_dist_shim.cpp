// test_dist_shim — edsparser::path_distances, driven by tests/test_dist_gpu.py (needs the GPU).
// One command per line of the file given as argv[1], tab separated; one answer line per command:
//   D <eds> <seds> <paths a,b,..|-> <columns|strings>
//       ->  K, '#', the K * K distances row by row, '#', the missing counts, '#', units
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
    if (f.size() < 5 || f[0] != "D" || (f[4] != "columns" && f[4] != "strings")) return "bad_command:";
    std::istringstream eds(f[1]), seds(f[2]);
    std::vector<int> paths;
    if (f[3] != "-") for (const auto& t : split(f[3], ',')) paths.push_back(std::stoi(t));
    const PathDistances d = path_distances(eds, seds, paths, f[4] == "columns" ? DistanceMetric::COLUMNS : DistanceMetric::STRINGS);
    std::string text = std::to_string(d.K) + '#';
    for (size_t a = 0; a < d.K; a++)
        for (size_t b = 0; b < d.K; b++) text += (a + b ? "," : "") + std::to_string(d.at(a, b));
    text += '#';
    for (size_t k = 0; k < d.missing.size(); k++) text += (k ? "," : "") + std::to_string(d.missing[k]);
    return text + '#' + std::to_string(d.units);
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::cerr << "usage: test_dist_shim <commands>\n"; return 2; }
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
