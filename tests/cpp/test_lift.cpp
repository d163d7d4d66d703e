// test_lift — edsparser::lift_positions, driven by tests/test_lift_gpu.py (needs the GPU).
// One command per line of the file given as argv[1], tab separated; one answer line per command:
//   L <eds> <seds> <queries src:pos:dst,src:pos:dst,..|->
//       ->  per query dst_pos:status:symbol:string:offset:column:common_pos, joined by ','
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
    if (f.size() < 4 || f[0] != "L") return "bad_command:";
    std::istringstream eds(f[1]), seds(f[2]);
    std::vector<LiftQuery> queries;
    if (f[3] != "-")
        for (const auto& t : split(f[3], ',')) {
            const std::vector<std::string> q = split(t, ':');
            if (q.size() != 3) return "bad_command:";
            queries.push_back(LiftQuery{std::stoull(q[0]), std::stoull(q[1]), std::stoull(q[2])});
        }
    std::string text;
    for (const LiftResult& r : lift_positions(eds, seds, queries)) {
        if (!text.empty()) text += ',';
        text += std::to_string(r.dst_pos) + ':' + std::to_string(static_cast<unsigned>(r.status)) + ':' + std::to_string(r.symbol) + ':' +
                std::to_string(r.string) + ':' + std::to_string(r.offset) + ':' + std::to_string(r.column) + ':' + std::to_string(r.common_pos);
    }
    return text;
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::cerr << "usage: test_lift <commands>\n"; return 2; }
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
