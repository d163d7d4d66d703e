// slice_args.hpp — the region grammar of edsparser-slice, apart from the tool so that tests/cpp/test_slice_args.cpp can run
// it without a device:
//   -r PATH:START-END     PATH an id or --prefix + id, positions from 0, END exclusive
//   --columns START-END   columns of the alignment view
//   a BED3+ line          tab separated; column 1 names the path, column 4, if present and not empty, the output
// A region's default name is <path>_<start>_<end>, or cols_<start>_<end>.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace slice_args {

struct Region { uint64_t path = 0, start = 0, end = 0; std::string name; };

inline bool parse_u64(const std::string& t, uint64_t& v)
{
    if (t.empty() || t[0] < '0' || t[0] > '9') return false;
    size_t used = 0;
    try { v = std::stoull(t, &used); } catch (...) { return false; }
    return used == t.size();
}

// an id, or prefix + id
inline bool parse_path(const std::string& t, const std::string& prefix, uint64_t& v)
{
    if (parse_u64(t, v)) return true;
    return !prefix.empty() && t.size() > prefix.size() && t.compare(0, prefix.size(), prefix) == 0 && parse_u64(t.substr(prefix.size()), v);
}

inline std::string default_name(const Region& r)
{
    return (r.path ? std::to_string(r.path) : std::string("cols")) + "_" + std::to_string(r.start) + "_" + std::to_string(r.end);
}

// START-END
inline bool parse_range(const std::string& t, uint64_t& start, uint64_t& end)
{
    const size_t dash = t.find('-');
    return dash != std::string::npos && parse_u64(t.substr(0, dash), start) && parse_u64(t.substr(dash + 1), end);
}

// PATH:START-END; the path's name may hold colons itself: the last one counts.  Path 0 is not a path
inline bool parse_region(const std::string& t, const std::string& prefix, Region& r)
{
    const size_t colon = t.rfind(':');
    if (colon == std::string::npos || !parse_path(t.substr(0, colon), prefix, r.path) || r.path == 0) return false;
    if (!parse_range(t.substr(colon + 1), r.start, r.end)) return false;
    r.name = default_name(r);
    return true;
}

inline bool parse_columns(const std::string& t, Region& r)
{
    r.path = 0;
    if (!parse_range(t, r.start, r.end)) return false;
    r.name = default_name(r);
    return true;
}

// one BED line without its line feed (a trailing '\r' is dropped).  -> 1 a region, 0 a comment or an empty line, -1 malformed.
// A name that is empty, ".", ".." or holds a '/' cannot name a file: malformed
inline int parse_bed_line(std::string line, const std::string& prefix, Region& r)
{
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty() || line[0] == '#') return 0;
    std::vector<std::string> f;
    size_t pos = 0;
    while (pos <= line.size()) {
        size_t end = line.find('\t', pos);
        if (end == std::string::npos) end = line.size();
        f.push_back(line.substr(pos, end - pos));
        pos = end + 1;
    }
    if (f.size() < 3 || !parse_path(f[0], prefix, r.path) || r.path == 0 || !parse_u64(f[1], r.start) || !parse_u64(f[2], r.end)) return -1;
    r.name = f.size() > 3 && !f[3].empty() ? f[3] : default_name(r);
    if (r.name == "." || r.name == ".." || r.name.find('/') != std::string::npos) return -1;
    return 1;
}

} // namespace slice_args
