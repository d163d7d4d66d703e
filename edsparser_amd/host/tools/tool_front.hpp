// tool_front.hpp — the front end the command-line tools share: the frame of main(), the -i / -s / -o files and their
// defaults, the path session over an EDS and its sources, path list options and the --names table.  A tool writes what is
// its own: its options and help text, its banner, its checks of its own options, the library call and the text it prints.
// Everything here reports an error by throwing; tool::run prints it as the tools always have.
#pragma once
#include "edsx.h"
#include "../cli_util.hpp"
#include "../device.hpp"
#include "tool_common.hpp"

namespace tool {

[[noreturn]] inline void fail(const std::string& msg) { throw std::runtime_error(msg); }

// The frame of main(): body returns on the help path and at its end (exit status 0) and throws on an error ("Error: <what>",
// exit status 1); the "[Performance]" line ends every run.
template <class Body> int run(Body&& body)
{
    edsparser::Timer timer;
    timer.start();
    int status = 0;
    try { body(); }
    catch (const std::exception& e) { std::cerr << "Error: " << e.what() << "\n"; status = 1; }
    print_performance(timer);
    return status;
}

// <input stem><suffix> next to the input: the default name of an output
inline std::filesystem::path beside(const std::filesystem::path& input, const std::string& suffix)
{
    return input.parent_path() / (input.stem().string() + suffix);
}

// The files of -i, -s (default: the input with the .seds extension) and -o (default, for a tool that has one: <input stem><suffix>)
struct Files {
    std::filesystem::path input, sources, output;
    bool sources_given;
};

inline Files files(const edsparser::cli::Parser& opts, const std::string& suffix = "")
{
    Files f{opts.get("input"), opts.get("sources"), opts.get("output"), false};
    f.sources_given = !f.sources.empty();
    if (!f.sources_given) { f.sources = f.input; f.sources.replace_extension(".seds"); }
    if (f.output.empty() && !suffix.empty()) f.output = beside(f.input, suffix);
    return f;
}

inline void need_input(const Files& f, bool quoted = false)
{
    if (!std::filesystem::exists(f.input)) fail("Input file does not exist: " + (quoted ? "\"" + f.input.string() + "\"" : f.input.string()));
}

// the input, then the sources: what a tool that works on paths cannot do without
inline void need_files(const Files& f, bool quoted = false, const char* work = "Path spelling")
{
    need_input(f, quoted);
    if (!std::filesystem::exists(f.sources)) fail(std::string(work) + " needs sources (.seds): " + f.sources.string() + " does not exist");
}

// the status of a library call on ctx: its error text as the tool's
inline void check(edsx_ctx* ctx, int status) { if (status != EDSX_OK) fail(edsx_last_error(ctx)); }

// A path session (edsx_paths_*) on the context of this thread.  The files are mapped for the open alone: the session
// keeps what it needs on the device.  A Session without files has none (s == nullptr) until open().
struct Session {
    edsx_ctx* ctx = nullptr;
    edsx_paths_session* s = nullptr;
    edsx_paths_info_t info{};

    Session() = default;
    explicit Session(const Files& f)
    {
        ctx = edsparser::detail::context();
        open(MappedFile(f.input, "input"), f.sources);
    }
    ~Session() { edsx_paths_close(s); }
    Session(const Session&) = delete;
    Session& operator=(const Session&) = delete;

    // for a caller that goes on reading the EDS it has mapped
    void open(const MappedFile& eds, const std::filesystem::path& sources)
    {
        ctx = edsparser::detail::context();
        const MappedFile seds(sources, "sources");
        tool::check(ctx, edsx_paths_open(ctx, eds.data(), eds.size(), seds.data(), seds.size(), &s));
        edsx_paths_info(s, &info);
    }
    void check(int status) const { tool::check(ctx, status); }
};

// A path list option (-p, -t, -d): the ids as they were given, none without the option (a list that parses is never empty)
inline std::vector<uint64_t> path_list(const edsparser::cli::Parser& opts, const std::string& option)
{
    return opts.has(option) ? parse_paths(opts.get(option), option) : std::vector<uint64_t>();
}

inline std::vector<uint64_t> all_paths(uint64_t P)
{
    std::vector<uint64_t> ids;
    for (uint64_t p = 1; p <= P; p++) ids.push_back(p);
    return ids;
}

// ... and once P is known: 1..P for no list, and every id within 1..P (for the calls that index host arrays by them; the
// other tools leave the check, and its text, to the library)
inline void resolve_paths(std::vector<uint64_t>& ids, uint64_t P)
{
    if (ids.empty()) ids = all_paths(P);
    for (uint64_t p : ids)
        if (p == 0 || p > P) fail("Path id " + std::to_string(p) + " out of range (1.." + std::to_string(P) + ")");
}

// one entry per line, without its line end ('\n' or "\r\n"); a last line needs none
inline std::vector<std::string> read_lines(const std::string& path, const std::string& cannot_open)
{
    std::ifstream in(path);
    if (!in) fail(cannot_open + ": " + path);
    std::vector<std::string> lines;
    for (std::string line; std::getline(in, line);) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        lines.push_back(line);
    }
    return lines;
}

inline std::vector<const char*> c_strs(const std::vector<std::string>& text)
{
    std::vector<const char*> p;
    for (const std::string& t : text) p.push_back(t.c_str());
    return p;
}

// --names FILE, whose line k names path k, and --prefix.  Read where it is constructed.
struct Names {
    bool given;
    std::string prefix;
    std::vector<std::string> lines;

    Names(const edsparser::cli::Parser& opts, const std::string& default_prefix) : given(opts.has("names")), prefix(opts.get("prefix", default_prefix))
    {
        if (given) lines = read_lines(opts.get("names"), "Cannot open names file");
    }
    // The name of path p: its line, which has to be there and, unless the name is a table cell, not empty; without a file
    // <prefix><p - 1>, as eds2msa names its rows.  A table cell (dist, ibs, mosaic) takes no name, from either, that is empty or
    // holds a tab, blank or line feed.
    std::string name_of(uint64_t p, bool cell = false) const
    {
        if (given && (p == 0 || p > lines.size() || (!cell && lines[p - 1].empty()))) fail("The names file has no name for path " + std::to_string(p));
        const std::string name = given ? lines[p - 1] : prefix + std::to_string(p - 1);
        if (cell && (name.empty() || name.find_first_of("\t \n") != std::string::npos))
            fail("The name of path " + std::to_string(p) + " is empty or holds a tab, blank or line feed");
        return name;
    }
    std::vector<std::string> names_of(const std::vector<uint64_t>& ids, bool cell = false) const
    {
        std::vector<std::string> names;
        for (uint64_t p : ids) names.push_back(name_of(p, cell));
        return names;
    }
};

} // namespace tool
