// test_tool_front.cpp — the pieces of the tools' front end (edsparser_amd/host/tools/tool_front.hpp) that need no device:
// path lists, the -i / -s / -o defaults and the --names table.  Every line of the cases file is a kind and, tab
// separated, its fields; the answer is one line each, "error: <what>" for what the front end throws.
//   p OPTION TEXT            tool::parse_paths(TEXT, OPTION)                      -> the ids
//   r P TEXT|-               the list ("-": none), then tool::resolve_paths(.., P) -> the ids
//   f SUFFIX ARG...          tool::files of the command line ARG..., SUFFIX "-": none -> input|sources|output|sources_given
//   n CELL ID ARG...         tool::Names of the command line ARG... (default prefix "s"), name_of(ID, CELL)
//   v IDS ARG...             ... names_of(IDS) through tool::c_strs, joined with '|'
#include "tool_front.hpp"

#include <sstream>

namespace {

std::string join(const std::vector<uint64_t>& ids)
{
    std::string s;
    for (uint64_t p : ids) s += (s.empty() ? "" : " ") + std::to_string(p);
    return s;
}

edsparser::cli::Parser parser(const std::vector<std::string>& args, size_t from)
{
    edsparser::cli::Parser opts("test");
    for (const char* name : {"input", "sources", "output", "names", "prefix"}) opts.add(name, name[0], true, false, "");
    std::vector<char*> argv(1, const_cast<char*>("test"));
    for (size_t k = from; k < args.size(); k++) argv.push_back(const_cast<char*>(args[k].c_str()));
    opts.parse(static_cast<int>(argv.size()), argv.data());
    return opts;
}

std::string answer(const std::vector<std::string>& a)
{
    if (a[0] == "p") return join(tool::parse_paths(a.at(2), a.at(1)));
    if (a[0] == "r") {
        std::vector<uint64_t> ids;
        if (a.at(2) != "-") ids = tool::parse_paths(a[2], "paths");
        tool::resolve_paths(ids, std::stoull(a.at(1)));
        return join(ids);
    }
    if (a[0] == "f") {
        const tool::Files f = tool::files(parser(a, 2), a.at(1) == "-" ? "" : a[1]);
        return f.input.string() + "|" + f.sources.string() + "|" + f.output.string() + "|" + (f.sources_given ? "1" : "0");
    }
    if (a[0] == "n") return tool::Names(parser(a, 3), "s").name_of(std::stoull(a.at(2)), a.at(1) == "1");
    if (a[0] == "v") {
        const std::vector<std::string> names = tool::Names(parser(a, 2), "s").names_of(tool::parse_paths(a.at(1), "paths"));
        std::string s;
        for (const char* c : tool::c_strs(names)) s += (s.empty() ? "" : "|") + std::string(c);
        return s;
    }
    throw std::logic_error("unknown kind " + a[0]);
}

} // namespace

int main(int argc, char** argv)
{
    if (argc < 2) { std::cerr << "usage: test_tool_front cases.txt\n"; return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    for (std::string line; std::getline(in, line);) {
        std::vector<std::string> a;
        std::istringstream ls(line);
        for (std::string t; std::getline(ls, t, '\t');) a.push_back(t);
        if (line.empty() || line.back() == '\t') a.push_back("");          // a last field that is empty
        try { std::cout << answer(a) << "\n"; }
        catch (const std::logic_error& e) { std::cerr << e.what() << "\n"; return 2; }
        catch (const std::exception& e) { std::cout << "error: " << e.what() << "\n"; }
    }
    return 0;
}
