// test_gfa — edsparser::eds_to_gfa (the shim over edsx_eds_gfa_graph / edsx_paths_gfa_walks) on hand-written cases and on
// its errors, run by tests/test_gfa_cpp_gpu.py.  Exit code 0 and "ok" when everything holds; the first difference otherwise.
#include "edsparser/transforms/eds_transforms.hpp"

#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>

using namespace edsparser;

static int fail(const std::string& what)
{
    std::cout << "FAILED: " << what << "\n";
    return 1;
}

int main()
{
    // {,C} is open: A is linked to C and to G; path 2 takes the empty string there
    const std::string eds = "{A}{,C}{G,T}", seds = "{0}{2}{1}{1}{2}";
    const std::string graph = "H\tVN:Z:1.0\nS\t1\tA\nS\t2\tC\nS\t3\tG\nS\t4\tT\n"
                              "L\t1\t+\t2\t+\t0M\nL\t1\t+\t3\t+\t0M\nL\t1\t+\t4\t+\t0M\nL\t2\t+\t3\t+\t0M\nL\t2\t+\t4\t+\t0M\n";
    {
        std::istringstream e(eds);
        std::ostringstream out;
        GfaInfo info;
        eds_to_gfa(e, nullptr, out, {}, nullptr, "path", 0, &info);
        if (out.str() != graph) return fail("graph: " + out.str());
        if (info.n_symbols != 3 || info.n_strings != 5 || info.n_segments != 4 || info.n_empty_strings != 1 || info.n_open_symbols != 1 ||
            info.n_links != 5 || info.header_bytes != 11 || info.segment_bytes != 24 || info.link_bytes != 65 || !info.steps.empty())
            return fail("info");
    }
    {
        std::istringstream e(eds), s(seds);
        std::ostringstream out;
        GfaInfo info;
        eds_to_gfa(e, &s, out, {}, nullptr, "hap", 0, &info);
        if (out.str() != graph + "P\thap1\t1+,2+,3+\t*\nP\thap2\t1+,4+\t*\n") return fail("walks: " + out.str());
        if (info.steps != std::vector<size_t>{3, 2} || info.missing != std::vector<size_t>{0, 0}) return fail("steps");
    }
    {
        std::istringstream e(eds), s(seds);
        std::ostringstream out;
        const std::vector<std::string> names = {"b", "a"};
        eds_to_gfa(e, &s, out, {2, 1}, &names);
        if (out.str() != graph + "P\tb\t1+,4+\t*\nP\ta\t1+,2+,3+\t*\n") return fail("names: " + out.str());
    }
    {
        std::istringstream e(eds);
        std::ostringstream out;
        eds_to_gfa(e, nullptr, out, {}, nullptr, "path", 5);
        if (out.str() != graph) return fail("max_links at the count");
    }
    const std::vector<std::string> blank = {"a b"};
    const struct { bool sources; std::vector<int> ids; const std::vector<std::string>* names; size_t max_links; const char* text; } bad[] = {
        {false, {}, nullptr, 4, "Graph has 5 links, above the limit of 4"},
        {true, {3}, nullptr, 0, "Path id 3 out of range (1..2)"},
        {true, {1}, &blank, 0, "Path name 0 is not a GFA name"},
        {false, {1}, nullptr, 0, "paths and names need sources"}};
    for (const auto& b : bad) {
        std::istringstream e(eds), s(seds);
        std::ostringstream out;
        try {
            eds_to_gfa(e, b.sources ? &s : nullptr, out, b.ids, b.names, "path", b.max_links);
            return fail(std::string("no exception for: ") + b.text);
        } catch (const std::invalid_argument& ex) {
            if (std::string(ex.what()).find(b.text) == std::string::npos) return fail(std::string("text: ") + ex.what());
        }
        if (!out.str().empty()) return fail(std::string("output written for: ") + b.text);
    }
    std::cout << "ok\n";
    return 0;
}
