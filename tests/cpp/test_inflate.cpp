// test_inflate.cpp — the host build of the DEFLATE decoder core (edsparser_amd/csrc/inflate.hpp) over a corpus file
// written by tests/test_bgzf_cpu.py; meant to be built with -fsanitize=address,undefined.
//
// Records (little endian): u32 type, u32 arg, u32 name_len, name, u64 data_len, data, u64 aux_len, aux
//   type 0  data inflates to aux; arg = the kind gz_probe must report (0 plain: inflate(x) is x)
//   type 1  data must be refused: aux = "<block>\n<reason>|<reason>..." (the block index and the reasons allowed)
//   type 2  data with one bit flipped must be refused at block arg: aux = pairs of u64 (byte, bit), one case each
// Every refusal is printed as "<name>\t<error text>" (tests/test_bgzf_gpu.py compares the device's texts with these).
#include "inflate.hpp"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

using namespace edsx::gz;

static const char* const REASONS[] = {"truncated", "not a gzip member", "block size beyond the end of the file", "invalid DEFLATE stream",
                                      "length mismatch", "CRC mismatch"};

static int failures = 0;
static void fail(const std::string& name, const std::string& what)
{
    std::fprintf(stderr, "FAIL %s: %s\n", name.c_str(), what.c_str());
    failures++;
}

// inflate(x) as the library defines it: plain input is itself
static bool inflate_any(const std::vector<uint8_t>& data, std::vector<uint8_t>& out, std::string& err)
{
    out.clear();
    if (gz_probe(data.data(), data.size()) == GZ_PLAIN) { out = data; return true; }
    return gz_inflate_host(data.data(), data.size(), out, "input", err);
}

// "Compressed input: block <k> at byte <off>: <reason>" with block k and a reason of `allowed` ('|'-separated; empty: any listed)
static bool refusal_ok(const std::string& err, unsigned long long block, const std::string& allowed)
{
    const std::string head = "Compressed input: block " + std::to_string(block) + " at byte ";
    if (err.compare(0, head.size(), head) != 0) return false;
    const size_t colon = err.find(": ", head.size());
    if (colon == std::string::npos) return false;
    const std::string reason = err.substr(colon + 2);
    bool listed = false;
    for (const char* r : REASONS) listed |= reason == r;
    if (!listed) return false;
    if (allowed.empty()) return true;
    return ("|" + allowed + "|").find("|" + reason + "|") != std::string::npos;
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: test_inflate corpus.bin\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    size_t at = 0, cases = 0;
    auto u32at = [&]() { uint32_t v; std::memcpy(&v, file.data() + at, 4); at += 4; return v; };
    auto u64at = [&]() { uint64_t v; std::memcpy(&v, file.data() + at, 8); at += 8; return v; };
    std::vector<uint8_t> out;
    std::string err;
    while (at < file.size()) {
        const uint32_t type = u32at(), arg = u32at(), name_len = u32at();
        const std::string name(reinterpret_cast<const char*>(file.data() + at), name_len); at += name_len;
        const uint64_t dn = u64at();
        std::vector<uint8_t> data(file.begin() + at, file.begin() + at + dn); at += dn;     // (its own allocation: the sanitizer sees its end)
        const uint64_t an = u64at();
        const std::vector<uint8_t> aux(file.begin() + at, file.begin() + at + an); at += an;
        if (type == 0) {
            cases++;
            if ((uint32_t)gz_probe(data.data(), data.size()) != arg) fail(name, "gz_probe: kind " + std::to_string(gz_probe(data.data(), data.size())));
            if (!inflate_any(data, out, err)) fail(name, "refused: " + err);
            else if (out != aux) fail(name, "text differs (" + std::to_string(out.size()) + " bytes, expected " + std::to_string(aux.size()) + ")");
            if (arg == GZ_BGZF) {
                unsigned long long text_size = 0, seen = 0;
                gz_walk(data.data(), data.size(), text_size, [&](const BgzfBlock&) { seen++; });
                if (text_size != aux.size() || seen == 0) fail(name, "block walk: text size " + std::to_string(text_size));
            }
        } else if (type == 1) {
            cases++;
            const std::string spec(aux.begin(), aux.end());
            const size_t nl = spec.find('\n');
            const unsigned long long block = std::stoull(spec.substr(0, nl));
            if (inflate_any(data, out, err)) fail(name, "accepted");
            else {
                if (!refusal_ok(err, block, spec.substr(nl + 1))) fail(name, "refused with: " + err);
                std::printf("%s\t%s\n", name.c_str(), err.c_str());
            }
        } else if (type == 2) {
            for (size_t i = 0; i + 16 <= aux.size(); i += 16) {
                cases++;
                uint64_t byte, bit;
                std::memcpy(&byte, aux.data() + i, 8); std::memcpy(&bit, aux.data() + i + 8, 8);
                const std::string cname = name + std::to_string(i / 16);
                data[byte] ^= (uint8_t)(1u << bit);
                if (inflate_any(data, out, err)) fail(cname, "accepted");
                else {
                    if (!refusal_ok(err, arg, "")) fail(cname, "refused with: " + err);
                    std::printf("%s\t%s\n", cname.c_str(), err.c_str());
                }
                data[byte] ^= (uint8_t)(1u << bit);
            }
        } else { fail(name, "unknown record type"); break; }
    }
    std::fprintf(stderr, "%zu cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
