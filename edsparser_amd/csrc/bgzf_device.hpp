// bgzf_device.hpp — gzip / BGZF input: BGZF blocks are inflated and CRC-checked on the device (bgzf_device.hip), other
// gzip files by the serial host inflater of inflate.hpp; the text ends in a DevBuf the VCF pipeline can read.
#pragma once

#include "inflate.hpp"
#include "msa_device.hpp"

#include <string>
#include <vector>

namespace edsx {

struct GzInfo {   // the layout of edsx_gz_info
    int kind = 0, inflated_on_device = 0;
    u64 blocks = 0, comp_bytes = 0, text_bytes = 0, h2d_bytes = 0, text_d2h_bytes = 0;
    double index_ms = 0, inflate_ms = 0, crc_ms = 0;
};

// inflate(x) of one input, wherever it came out: on the device (BGZF), on the host (gzip), or x itself (plain)
struct GzText {
    DevBuf dev; bool on_device = false;            // 256-byte aligned, 16 bytes of slack behind the n bytes
    std::vector<uint8_t> host; bool on_host = false;
    const uint8_t* plain = nullptr;                // kind 0: the caller's bytes
    u64 n = 0;
};

// what: "VCF", "FASTA" or "input" (the error texts).  Throws FormatError for a bad compressed layer.
void gz_open(const uint8_t* data, size_t size, const char* what, GzText& out, GzInfo& info, hipStream_t st);

} // namespace edsx
