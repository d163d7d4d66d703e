// test_paths — EDS::max_path_id / EDS::path_sequence of the host container, driven by tests/test_paths_cpu.py.
// One command per line of the file given as argv[1], tab separated; one answer line per command:
//   A <eds> <seds|->            ->  P|seq1:missing1|seq2:missing2|...   (every path 1..P)
//   P <eds> <seds|-> <path>     ->  seq:missing
//   F <eds> <seds> <line width> <paths a,b,..|-> <names a,b,..|->   (needs the GPU: edsparser::eds_to_fasta)
//                               ->  the FASTA with '|' for every line feed, '#', the missing counts
// An exception answers <kind>:<what>.
#include "edsparser/formats/eds.hpp"
#include "edsparser/transforms/eds_transforms.hpp"

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace edsparser;

static std::vector<std::string> split_tabs(const std::string& line)
{
    std::vector<std::string> f;
    size_t pos = 0;
    while (true) {
        const size_t end = line.find('\t', pos);
        f.push_back(line.substr(pos, end == std::string::npos ? std::string::npos : end - pos));
        if (end == std::string::npos) break;
        pos = end + 1;
    }
    return f;
}

static std::vector<std::string> split_commas(const std::string& t)
{
    std::vector<std::string> f;
    std::stringstream ss(t);
    for (std::string item; std::getline(ss, item, ',');) f.push_back(item);
    return f;
}

static std::string fasta_answer(const std::vector<std::string>& f)
{
    std::istringstream eds(f[1]), seds(f[2]);
    std::ostringstream out;
    std::vector<int> paths;
    if (f[4] != "-") for (const auto& t : split_commas(f[4])) paths.push_back(std::stoi(t));
    std::vector<std::string> names;
    if (f[5] != "-") names = split_commas(f[5]);
    std::vector<size_t> missing;
    eds_to_fasta(eds, seds, out, paths, std::stoul(f[3]), f[5] != "-" ? &names : nullptr, &missing);
    std::string text = out.str();
    for (char& c : text) if (c == '\n') c = '|';
    text += '#';
    for (size_t k = 0; k < missing.size(); k++) text += (k ? "," : "") + std::to_string(missing[k]);
    return text;
}

static std::string answer(const std::vector<std::string>& f)
{
    if (f.size() < 3) return "bad_command:";
    if (f[0] == "F" && f.size() >= 6) return fasta_answer(f);
    EDS eds = f[2] == "-" ? EDS(f[1]) : EDS(f[1], f[2]);
    std::ostringstream os;
    if (f[0] == "A") {
        const int P = eds.max_path_id();
        os << P;
        for (int p = 1; p <= P; p++) {
            size_t miss = 0;
            const String s = eds.path_sequence(p, &miss);
            os << '|' << s << ':' << miss;
        }
    } else if (f[0] == "P" && f.size() >= 4) {
        size_t miss = 0;
        const String s = eds.path_sequence(std::stoi(f[3]), &miss);
        os << s << ':' << miss;
    } else {
        return "bad_command:";
    }
    return os.str();
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::cerr << "usage: test_paths <commands>\n"; return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::cerr << "cannot open " << argv[1] << "\n"; return 2; }
    for (std::string line; std::getline(in, line);) {
        std::string out;
        try { out = answer(split_tabs(line)); }
        catch (const std::invalid_argument& e) { out = std::string("invalid_argument:") + e.what(); }
        catch (const std::out_of_range& e) { out = std::string("out_of_range:") + e.what(); }
        catch (const std::exception& e) { out = std::string("runtime_error:") + e.what(); }
        std::cout << out << "\n";
    }
    return 0;
}
