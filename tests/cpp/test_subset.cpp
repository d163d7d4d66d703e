// test_subset — edsparser::eds_subset (the shim over edsx_eds_subset) on one hand-written case and on its errors, run by
// tests/test_subset_cpp_gpu.py.  Exit code 0 and "ok" when everything holds; the first difference otherwise.
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
    // {G,T} loses both strings and goes; {AC} and {TT} fuse; {A,C} keeps both strings with renumbered sets
    const std::string eds = "{AC}{G,T}{TT}{A,C}", seds = "{0}{2}{4}{0}{1}{3}";
    {
        std::istringstream e(eds), s(seds);
        std::ostringstream eo, so;
        SubsetInfo info;
        eds_subset(e, s, eo, so, {3, 1}, false, &info);
        if (eo.str() != "{ACTT}{A,C}\n") return fail("eds: " + eo.str());
        if (so.str() != "{0}{1}{2}\n") return fail("seds: " + so.str());
        if (info.symbols_in != 4 || info.symbols_out != 2 || info.strings_in != 6 || info.strings_out != 3 || info.chars_in != 8 ||
            info.chars_out != 6 || info.paths_in != 4 || info.paths_out != 2 || info.symbols_removed != 1 || info.common_runs_merged != 1)
            return fail("info");
    }
    {
        std::istringstream e(eds), s(seds);
        std::ostringstream eo, so;
        eds_subset(e, s, eo, so, {3, 1}, true);
        if (eo.str() != "{ACTT}{A,C}\n" || so.str() != "{0}{1}{3}\n") return fail("keep_ids: " + eo.str() + " " + so.str());
    }
    const struct { std::vector<int> ids; const char* text; } bad[] = {
        {{}, "No paths selected"}, {{5}, "Path id 5 out of range (1..4)"}, {{0}, "Path id 0 out of range (1..4)"},
        {{2, 2}, "Path id 2 given twice"}};
    for (const auto& b : bad) {
        std::istringstream e(eds), s(seds);
        std::ostringstream eo, so;
        try {
            eds_subset(e, s, eo, so, b.ids);
            return fail(std::string("no exception for: ") + b.text);
        } catch (const std::invalid_argument& ex) {
            if (std::string(ex.what()).find(b.text) == std::string::npos) return fail(std::string("text: ") + ex.what());
        }
    }
    std::cout << "ok\n";
    return 0;
}
