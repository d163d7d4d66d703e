// test_slice_args.cpp — the region grammar of edsparser-slice (edsparser_amd/host/tools/slice_args.hpp) without a device:
// every line of the file is a kind (r: a -r argument, c: a --columns argument, b: a BED line) and, behind one blank, the
// text; the answer is "path start end name", "skip" or "bad", one line each.
#include "slice_args.hpp"

#include <fstream>
#include <iostream>

int main(int argc, char** argv)
{
    if (argc < 3) { std::cerr << "usage: test_slice_args cases.txt prefix\n"; return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    const std::string prefix = argv[2];
    for (std::string line; std::getline(in, line);) {
        if (line.size() < 2) return 2;
        const std::string text = line.substr(2);
        slice_args::Region r;
        int rc;
        if (line[0] == 'r') rc = slice_args::parse_region(text, prefix, r) ? 1 : -1;
        else if (line[0] == 'c') rc = slice_args::parse_columns(text, r) ? 1 : -1;
        else rc = slice_args::parse_bed_line(text, prefix, r);
        if (rc > 0) std::cout << r.path << " " << r.start << " " << r.end << " " << r.name << "\n";
        else std::cout << (rc ? "bad" : "skip") << "\n";
    }
    return 0;
}
