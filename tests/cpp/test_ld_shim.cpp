// test_ld_shim — edsparser::path_ld, driven by tests/test_ld_gpu.py (needs the GPU).
// One command per line of the file given as argv[1], tab separated; one answer line per command:
//   L <eds> <seds> <paths a,b,..|-> <window> <min_r2> <min_count> <all_strings 0|1>
//       ->  the pairs, each as its eight integers and the bits of r2 separated by commas and closed by ';', then '#', the
//           alleles the same way, '#', paths, choice symbols, candidate pairs, undefined pairs
// An exception answers <kind>:<what>.
#include "edsparser/transforms/eds_transforms.hpp"

#include <cstring>
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
    if (f.size() < 8 || f[0] != "L") return "bad_command:";
    std::istringstream eds(f[1]), seds(f[2]);
    std::vector<int> paths;
    if (f[3] != "-") for (const auto& t : split(f[3], ',')) paths.push_back(std::stoi(t));
    LdOptions o;
    o.window = std::stoull(f[4]); o.min_r2 = std::stod(f[5]); o.min_count = std::stoull(f[6]); o.all_strings = f[7] == "1";
    const PathLd d = path_ld(eds, seds, paths, o);
    std::string text;
    for (const LdPair& p : d.pairs) {
        uint64_t bits;
        std::memcpy(&bits, &p.r2, 8);
        for (uint64_t v : {p.symbol_a, p.string_a, p.symbol_b, p.string_b, p.n_ab, p.n_a, p.n_b, p.n}) text += std::to_string(v) + ',';
        text += std::to_string(bits) + ';';
    }
    text += '#';
    for (const LdAllele& a : d.alleles)
        text += std::to_string(a.symbol) + ',' + std::to_string(a.string) + ',' + std::to_string(a.count) + ',' + std::to_string(a.present) + ';';
    return text + '#' + std::to_string(d.paths) + ',' + std::to_string(d.choice_symbols) + ',' + std::to_string(d.candidate_pairs) + ',' +
           std::to_string(d.undefined_pairs);
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::cerr << "usage: test_ld_shim <commands>\n"; return 2; }
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
