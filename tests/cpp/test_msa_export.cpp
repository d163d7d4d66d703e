// test_msa_export — edsparser::eds_to_msa, driven by tests/test_msa_export_gpu.py (needs the GPU).
// One command per line of the file given as argv[1], tab separated; one answer line per command:
//   M <eds> <seds> <line width> <paths a,b,..|-> <names a,b,..|-> <prefix> <gap character> <max bytes>
//       ->  the FASTA with '|' for every line feed, '#', the missing counts, '#', n_symbols,n_columns,n_zero_width_symbols,
//           widest_symbol,num_paths
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
    if (f.size() < 9 || f[0] != "M" || f[7].size() != 1) return "bad_command:";
    std::istringstream eds(f[1]), seds(f[2]);
    std::ostringstream out;
    std::vector<int> paths;
    if (f[4] != "-") for (const auto& t : split(f[4], ',')) paths.push_back(std::stoi(t));
    std::vector<std::string> names;
    if (f[5] != "-") names = split(f[5], ',');
    AlignInfo info;
    eds_to_msa(eds, seds, out, paths, std::stoul(f[3]), f[5] != "-" ? &names : nullptr, f[6], f[7][0], std::stoul(f[8]), &info);
    std::string text = out.str();
    for (char& c : text) if (c == '\n') c = '|';
    text += '#';
    for (size_t k = 0; k < info.missing.size(); k++) text += (k ? "," : "") + std::to_string(info.missing[k]);
    text += '#' + std::to_string(info.n_symbols) + ',' + std::to_string(info.n_columns) + ',' + std::to_string(info.n_zero_width_symbols) +
            ',' + std::to_string(info.widest_symbol) + ',' + std::to_string(info.num_paths);
    return text;
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::cerr << "usage: test_msa_export <commands>\n"; return 2; }
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
