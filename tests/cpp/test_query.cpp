// Query side of the edsparser::EDS container (check_position / extract / generate_patterns / the position tables),
// driven by tests/test_query_cpu.py: one command per input line (tab-separated fields), one result line per command.
//   C eds seds|- pos choices pattern     check_position      -> true | false | <exception kind>: <message>
//   X eds pos len changes                extract             -> =<string> | <exception kind>: <message>
//   G eds count length seed              generate_patterns   -> =<patterns joined by '|'> | <exception kind>: <message>
//   M eds                                metadata tables     -> <cum_common_positions>;<cum_degenerate_counts>
//   F eds_file seds_file|- queries_file   check_position of every "pos<TAB>choices<TAB>pattern" line of queries_file
//                                        against one EDS loaded from files -> one result line per query
//   W eds_file count length seed out_file generate_patterns into out_file -> ok | <exception kind>: <message>
//                                        (stderr: "sample_s <seconds>" of the sampling alone, without the load)
// choices / changes: comma-separated integers (may be empty).
#include "edsparser/formats/eds.hpp"

#include <chrono>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

using namespace edsparser;

namespace {

std::vector<std::string> split(const std::string& s, char sep)
{
    std::vector<std::string> out;
    std::string cur;
    for (char c : s) {
        if (c == sep) { out.push_back(cur); cur.clear(); }
        else cur += c;
    }
    out.push_back(cur);
    return out;
}

std::vector<int> ints(const std::string& s)
{
    std::vector<int> v;
    if (s.empty()) return v;
    for (const std::string& x : split(s, ',')) v.push_back(std::stoi(x));
    return v;
}

template <class F> std::string guarded(F&& f)
{
    try { return f(); }
    catch (const std::out_of_range& e) { return std::string("out_of_range: ") + e.what(); }
    catch (const std::invalid_argument& e) { return std::string("invalid_argument: ") + e.what(); }
    catch (const std::runtime_error& e) { return std::string("runtime_error: ") + e.what(); }
}

template <class T> std::string join(const std::vector<T>& v)
{
    std::string s;
    for (size_t i = 0; i < v.size(); i++) s += (i ? "," : "") + std::to_string(v[i]);
    return s;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 2) { std::cerr << "usage: test_query CASES\n"; return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        const std::vector<std::string> f = split(line, '\t');
        std::string r;
        if (f[0] == "C") {
            r = guarded([&] {
                const EDS e = f[2] == "-" ? EDS(f[1]) : EDS(f[1], f[2]);
                return std::string(e.check_position(std::stoull(f[3]), ints(f[4]), f[5]) ? "true" : "false");
            });
        } else if (f[0] == "X") {
            r = guarded([&] { return "=" + EDS(f[1]).extract(std::stoull(f[2]), static_cast<Length>(std::stoul(f[3])), ints(f[4])); });
        } else if (f[0] == "G") {
            r = guarded([&] {
                std::ostringstream os;
                EDS(f[1]).generate_patterns(os, std::stoull(f[2]), static_cast<Length>(std::stoul(f[3])), std::stoull(f[4]));
                std::string s = os.str();
                for (char& c : s) if (c == '\n') c = '|';
                return "=" + s;
            });
        } else if (f[0] == "M") {
            const EDS e(f[1]);
            r = join(e.get_metadata().cum_common_positions) + ";" + join(e.get_metadata().cum_degenerate_counts);
        } else if (f[0] == "F") {
            const EDS e = f[2] == "-" ? EDS::load(f[1]) : EDS::load(f[1], f[2]);
            std::ifstream qf(f[3]);
            std::string q, all;
            while (std::getline(qf, q)) {
                const std::vector<std::string> g = split(q, '\t');
                all += guarded([&] { return std::string(e.check_position(std::stoull(g[0]), ints(g[1]), g[2]) ? "true" : "false"); });
                all += '\n';
            }
            std::cout << all;
            continue;
        } else if (f[0] == "W") {
            r = guarded([&] {
                const EDS e = EDS::load(f[1]);
                std::ofstream out(f[5], std::ios::binary);
                const auto t0 = std::chrono::steady_clock::now();
                e.generate_patterns(out, std::stoull(f[2]), static_cast<Length>(std::stoul(f[3])), std::stoull(f[4]));
                out.flush();
                std::cerr << "sample_s " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << "\n";
                return std::string("ok");
            });
        } else {
            std::cerr << "bad command: " << line << "\n";
            return 2;
        }
        std::cout << r << "\n";
    }
    return 0;
}
