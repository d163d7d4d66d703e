// edsparser-lift — translate positions between the paths of an EDS with sources, on the GPU (edsx_paths_lift*).
// Queries are read from -q, or from standard input without it (tab or blank separated, one per line; '#' lines and empty
// lines are skipped), results are written as TSV to -o (default: standard output).  A path is named by its id or by
// --prefix + id, as the other tools print them; a result names it as the query did.  Positions count from 0.  Modes:
//   (default)   path pos dst          ->  path pos dst dst_pos status           (--to PATH: two columns, every query to PATH)
//   --sites     path pos              ->  path pos symbol string offset column common_pos status
//   --from-eds  symbol string offset dst  ->  symbol string offset dst dst_pos status   (the columns of an edsparser-locate hit)
//   --bed       BED3+ lines, column 1 names the path, with --to PATH
//                                     ->  PATH start end <further columns> status_of_start status_of_end
// status: SAME the very character, ALIGNED another one in the same alignment column, GAP dst_pos is the next character to
// the right, MISSING the path has no string in the symbol, RANGE no such character (every result field is "."); --sites:
// OK or RANGE.  common_pos is "." inside a degenerate symbol.  An interval [s, e) is lifted by its first and last
// character: start = pos(s), end = pos(e - 1), plus one when that character is there (SAME or ALIGNED); an interval that
// comes out empty is written, not dropped.  Argument and query-file errors are reported before a context is created.
#include "tool_front.hpp"

#include <sstream>

using namespace edsparser;

namespace {

const char* const STATUS[] = {"SAME", "ALIGNED", "GAP", "MISSING", "RANGE"};

std::string num(uint64_t v) { return v == UINT64_MAX ? std::string(".") : std::to_string(v); }

bool parse_u64(const std::string& t, uint64_t& v)
{
    if (t.empty() || t[0] < '0' || t[0] > '9') return false;
    size_t used = 0;
    try { v = std::stoull(t, &used); } catch (...) { return false; }
    return used == t.size();
}

// an id, or prefix + id
bool parse_path(const std::string& t, const std::string& prefix, uint64_t& v)
{
    if (parse_u64(t, v)) return true;
    return !prefix.empty() && t.size() > prefix.size() && t.compare(0, prefix.size(), prefix) == 0 && parse_u64(t.substr(prefix.size()), v);
}

} // namespace

int main(int argc, char** argv)
{
    return tool::run([&] {
        cli::Parser opts("Translate positions between the paths of an EDS");
        opts.add("help", 'h', false, false, "Show help message");
        opts.add("input", 'i', true, true, "Input EDS file (.eds / .leds)");
        opts.add("sources", 's', true, false, "Input source file (default: <input> with the .seds extension)");
        opts.add("queries", 'q', true, false, "Query file, one query per line (default: standard input)");
        opts.add("output", 'o', true, false, "Output TSV file (default: standard output)");
        opts.add("prefix", 0, true, false, "Path name prefix accepted in front of an id (default: path)");
        opts.add("to", 0, true, false, "Destination path of every query");
        opts.add("sites", 0, false, false, "path pos -> where the character lies in the EDS");
        opts.add("from-eds", 0, false, false, "symbol string offset dst -> the position on path dst");
        opts.add("bed", 0, false, false, "BED3+ intervals on the paths named in column 1 -> intervals on --to");
        opts.parse(argc, argv);
        if (opts.has("help")) {
            std::cout << "edsparser-lift - translate positions between the paths of an EDS\n\n" << opts.usage() << "\n"
                      << "EXAMPLES:\n"
                         "  edsparser-lift -i in.eds -q pos.tsv --to path1       # path<TAB>pos lines onto path 1\n"
                         "  edsparser-lift -i in.eds -q pos.tsv --sites          # symbol, string, offset, column\n"
                         "  cut -f3-5 hits.tsv | sed 's/$/\\t2/' | edsparser-lift -i in.eds --from-eds   # locate hits onto path 2\n"
                         "  edsparser-lift -i in.eds -q genes.bed --bed --to 7   # annotations of column 1's paths on path 7\n\n";
            return;
        }
        opts.notify();
        const tool::Files io = tool::files(opts);
        const std::filesystem::path query_file = opts.get("queries");
        const bool from_stdin = !opts.has("queries");
        const std::string prefix = opts.get("prefix", "path");
        const bool sites = opts.has("sites"), from_eds = opts.has("from-eds"), bed = opts.has("bed"), has_to = opts.has("to");
        if (sites + from_eds + bed > 1) tool::fail("--sites, --from-eds and --bed exclude each other");
        if (bed && !has_to) tool::fail("--bed needs --to");
        if (has_to && (sites || from_eds)) tool::fail("--to does not go with --sites or --from-eds");
        uint64_t to = 0;
        std::string to_text;
        if (has_to) {
            to_text = opts.get("to");
            if (!parse_path(to_text, prefix, to)) tool::fail("the argument ('" + to_text + "') for option '--to' is invalid");
        }
        tool::need_files(io, true);
        if (!from_stdin && !std::filesystem::exists(query_file)) tool::fail("Query file does not exist: \"" + query_file.string() + "\"");

        // the queries: a trailing '\r' is dropped, a missing final newline is fine
        std::vector<std::vector<std::string>> rows;              // the fields of every query line
        std::vector<uint64_t> a, b, c, d;                        // what the mode reads from them
        {
            std::ifstream file;
            if (!from_stdin) {
                file.open(query_file, std::ios::binary);
                if (!file) tool::fail("Cannot open query file: \"" + query_file.string() + "\"");
            }
            std::istream& in = from_stdin ? std::cin : file;
            size_t line_no = 0;
            for (std::string line; std::getline(in, line);) {
                line_no++;
                if (!line.empty() && line.back() == '\r') line.pop_back();
                if (line.empty() || line[0] == '#') continue;
                std::vector<std::string> f;
                if (bed) {                                       // tab separated, further columns pass through as they are
                    std::istringstream ls(line);
                    for (std::string t; std::getline(ls, t, '\t');) f.push_back(t);
                } else {
                    std::istringstream ls(line);
                    for (std::string t; ls >> t;) f.push_back(t);
                }
                auto bad = [&] { tool::fail("Query file line " + std::to_string(line_no) + " is malformed: \"" + line + "\""); };
                uint64_t v[4] = {0, 0, 0, 0};
                if (bed) {
                    if (f.size() < 3 || !parse_path(f[0], prefix, v[0]) || !parse_u64(f[1], v[1]) || !parse_u64(f[2], v[2]) || v[1] >= v[2])
                        bad();
                } else if (from_eds) {
                    if (f.size() != 4 || !parse_u64(f[0], v[0]) || !parse_u64(f[1], v[1]) || !parse_u64(f[2], v[2]) || !parse_path(f[3], prefix, v[3]))
                        bad();
                } else {
                    const size_t want = sites || has_to ? 2 : 3;
                    if (f.size() != want || !parse_path(f[0], prefix, v[0]) || !parse_u64(f[1], v[1]) ||
                        (want == 3 && !parse_path(f[2], prefix, v[2])))
                        bad();
                    if (has_to) v[2] = to;
                }
                a.push_back(v[0]); b.push_back(v[1]); c.push_back(v[2]); d.push_back(v[3]);
                rows.push_back(std::move(f));
            }
        }
        const size_t n = rows.size();

        std::cerr << "Loading EDS file: " << io.input << "\n";
        tool::Session ses(io);
        std::cerr << "Loaded EDS with " << ses.info.n_symbols << " symbols, " << ses.info.num_paths << " paths\n";
        std::cerr << "Lifting " << n << (bed ? " intervals" : " positions") << "...\n";

        std::string text;
        if (sites) {
            std::vector<edsx_lift_site> site(n);
            std::vector<uint8_t> st(n);
            ses.check(edsx_paths_lift_sites(ses.s, n, a.data(), b.data(), site.data(), st.data()));
            for (size_t q = 0; q < n; q++)
                text += rows[q][0] + "\t" + rows[q][1] + "\t" + num(site[q].symbol) + "\t" + num(site[q].string) + "\t" + num(site[q].offset) +
                        "\t" + num(site[q].column) + "\t" + num(site[q].common_pos) + "\t" + (st[q] ? "RANGE" : "OK") + "\n";
        } else if (from_eds) {
            std::vector<uint64_t> pos(n);
            std::vector<uint8_t> st(n);
            ses.check(edsx_paths_lift_place(ses.s, n, a.data(), b.data(), c.data(), d.data(), pos.data(), st.data()));
            for (size_t q = 0; q < n; q++)
                text += rows[q][0] + "\t" + rows[q][1] + "\t" + rows[q][2] + "\t" + rows[q][3] + "\t" + num(pos[q]) + "\t" + STATUS[st[q]] + "\n";
        } else if (bed) {                                        // both ends of every interval in one call
            std::vector<uint64_t> src(2 * n), at(2 * n), dst(2 * n, to), pos(2 * n);
            std::vector<uint8_t> st(2 * n);
            for (size_t q = 0; q < n; q++) { src[2 * q] = src[2 * q + 1] = a[q]; at[2 * q] = b[q]; at[2 * q + 1] = c[q] - 1; }
            ses.check(edsx_paths_lift(ses.s, 2 * n, src.data(), at.data(), dst.data(), pos.data(), st.data(), nullptr));
            for (size_t q = 0; q < n; q++) {
                const uint8_t s0 = st[2 * q], s1 = st[2 * q + 1];
                const bool there = s0 != EDSX_LIFT_RANGE && s1 != EDSX_LIFT_RANGE;
                text += to_text + "\t" + (there ? std::to_string(pos[2 * q]) : ".") + "\t" +
                        (there ? std::to_string(pos[2 * q + 1] + (s1 < EDSX_LIFT_GAP ? 1 : 0)) : ".");
                for (size_t k = 3; k < rows[q].size(); k++) text += "\t" + rows[q][k];
                text += std::string("\t") + STATUS[s0] + "\t" + STATUS[s1] + "\n";
            }
        } else {
            std::vector<uint64_t> pos(n);
            std::vector<uint8_t> st(n);
            ses.check(edsx_paths_lift(ses.s, n, a.data(), b.data(), c.data(), pos.data(), st.data(), nullptr));
            for (size_t q = 0; q < n; q++)
                text += rows[q][0] + "\t" + rows[q][1] + "\t" + (has_to ? to_text : rows[q][2]) + "\t" + num(pos[q]) + "\t" + STATUS[st[q]] + "\n";
        }
        if (opts.has("output")) tool::write_bytes(opts.get("output"), reinterpret_cast<const uint8_t*>(text.data()), text.size(), "output");
        else std::cout << text;
        edsx_paths_timing t;
        edsx_paths_last_timing(ses.s, &t);
        std::cerr << "Device: tables " << t.choose_ms + t.scan_ms << " ms, search and place " << t.copy_ms << " ms\n";
        if (opts.has("output")) std::cerr << "Output written to: " << opts.get("output") << "\n";
    });
}
