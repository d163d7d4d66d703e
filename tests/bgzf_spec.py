"""BGZF / gzip test vectors: a pure-Python BGZF writer and reader (stdlib zlib only) and the corpus the compressed-input
tests share.  The reference for the compressed layer is Python's zlib / gzip, nothing else.

A BGZF block is a gzip member with FLG = 4 and one extra subfield 'B' 'C' (SLEN 2) that holds BSIZE = block size - 1;
its payload is one raw DEFLATE stream (wbits = -15) of at most 64 KiB of text, its trailer CRC-32 and ISIZE.
"""
import gzip
import random
import struct
import zlib

MAX_PAYLOAD = 65280
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

REASONS = ("truncated", "not a gzip member", "block size beyond the end of the file", "invalid DEFLATE stream",
           "length mismatch", "CRC mismatch")


def raw_deflate(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, full_flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if full_flush_at is None:
        return c.compress(payload) + c.flush()
    return c.compress(payload[:full_flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(payload[full_flush_at:]) + c.flush()


def block(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, full_flush_at=None):
    """One BGZF block around `payload` (at most MAX_PAYLOAD bytes)."""
    assert len(payload) <= MAX_PAYLOAD
    data = raw_deflate(payload, level, strategy, full_flush_at)
    size = 18 + len(data) + 8
    assert size <= 65536, "the block does not fit BSIZE"
    head = struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, size - 1)
    return head + data + struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload))


def write(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, payload=MAX_PAYLOAD, eof=True, full_flush=False):
    """(file bytes, block table): the table holds (comp_off, out_off, comp_len, isize) of every block, EOF block included."""
    out, table, off, at = [], [], 0, 0
    view = memoryview(text)
    for i in range(0, len(text), payload):
        piece = bytes(view[i:i + payload])
        b = block(piece, level, strategy, len(piece) // 2 if full_flush else None)
        table.append((at, off, len(b), len(piece)))
        out.append(b)
        off += len(piece)
        at += len(b)
    if eof:
        table.append((at, off, len(EOF_BLOCK), 0))
        out.append(EOF_BLOCK)
    return b"".join(out), table


def read(data):
    """The text of a BGZF file, block by block through zlib (every trailer checked)."""
    out, off = [], 0
    while off < len(data):
        assert data[off:off + 4] == b"\x1f\x8b\x08\x04"
        xlen = struct.unpack_from("<H", data, off + 10)[0]
        assert data[off + 12:off + 16] == b"BC\x02\x00"
        size = struct.unpack_from("<H", data, off + 16)[0] + 1
        piece = zlib.decompress(data[off + 12 + xlen:off + size - 8], -15)
        crc, isize = struct.unpack_from("<II", data, off + size - 8)
        assert (zlib.crc32(piece) & 0xffffffff, len(piece)) == (crc, isize)
        out.append(piece)
        off += size
    return b"".join(out)


def gzip_member(payload, level=6, fname=None, mtime=0):
    """One plain gzip member (RFC 1952), optionally with FNAME and a modification time."""
    flg = 8 if fname else 0
    head = struct.pack("<BBBBIBB", 0x1f, 0x8b, 8, flg, mtime, 0, 0xff) + ((fname + b"\0") if fname else b"")
    return head + raw_deflate(payload, level) + struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload) & 0xffffffff)


# ---- the texts ----------------------------------------------------------------------------------------------
def vcf_text(n_bytes, seed=1):
    rng = random.Random(seed)
    lines = [b"##fileformat=VCFv4.2\n", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\ts2\ts3\n"]
    size, pos = sum(map(len, lines)), 1
    while size < n_bytes:
        pos += rng.randint(1, 400)
        ref, alt = rng.choice("ACGT"), rng.choice(["A", "C", "G", "T", "AT", "GCC"])
        gts = "\t".join(rng.choice(["0|0", "0|1", "1|0", "1|1"]) for _ in range(3))
        line = ("chr1\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT\t%s\n" % (pos, ref, alt, gts)).encode()
        lines.append(line)
        size += len(line)
    return b"".join(lines)[:n_bytes]


def fasta_text(n_bytes, seed=2):
    rng = random.Random(seed)
    seq = "".join(rng.choice("ACGT") for _ in range(n_bytes))
    body = "\n".join(seq[i:i + 60] for i in range(0, len(seq), 60))
    return (">chr1 test\n" + body + "\n").encode()[:n_bytes]


def texts():
    return {
        "vcf": vcf_text(150000),
        "fasta": fasta_text(150000),
        "zeros": bytes(100000),
        "random": random.Random(3).randbytes(MAX_PAYLOAD),
        "empty": b"",
        "short": b"A",
    }


# every DEFLATE stream shape zlib writes: (name, level, strategy, full flush in the middle of every member)
SHAPES = [
    ("stored", 0, zlib.Z_DEFAULT_STRATEGY, False),
    ("level1", 1, zlib.Z_DEFAULT_STRATEGY, False),
    ("level6", 6, zlib.Z_DEFAULT_STRATEGY, False),
    ("level9", 9, zlib.Z_DEFAULT_STRATEGY, False),
    ("fixed", 6, zlib.Z_FIXED, False),
    ("rle", 6, zlib.Z_RLE, False),
    ("huffman_only", 6, zlib.Z_HUFFMAN_ONLY, False),
    ("full_flush", 6, zlib.Z_DEFAULT_STRATEGY, True),
]


def corpus():
    """[(name, file bytes, text, kind, block table or None)]: kind 1 BGZF, 2 gzip."""
    out = []
    for tname, text in texts().items():
        for sname, level, strategy, ff in SHAPES:
            # level 0 adds 5 bytes per 65535: a smaller payload keeps a stored block inside BSIZE
            data, table = write(text, level, strategy, payload=MAX_PAYLOAD if level else 65000, full_flush=ff)
            assert gzip.decompress(data) == text and read(data) == text
            out.append(("%s/%s" % (tname, sname), data, text, 1, table))
    t = texts()
    data, table = write(t["vcf"], eof=False)
    out.append(("vcf/no_eof_block", data, t["vcf"], 1, table))
    data, table = write(t["vcf"], payload=777)
    out.append(("vcf/small_blocks", data, t["vcf"], 1, table))
    multi = gzip_member(t["vcf"][:50000], fname=b"a.vcf", mtime=1700000000) + gzip_member(t["vcf"][50000:], 9, mtime=1)
    assert gzip.decompress(multi) == t["vcf"]
    out.append(("vcf/gzip_multi_fname_mtime", multi, t["vcf"], 2, None))
    big = gzip_member(t["fasta"])
    out.append(("fasta/gzip_over_64k", big, t["fasta"], 2, None))
    out.append(("fasta/gzip_module", gzip.compress(t["fasta"], 6), t["fasta"], 2, None))
    mixed = write(t["vcf"][:70000])[0] + gzip_member(t["vcf"][70000:])
    out.append(("vcf/bgzf_then_gzip", mixed, t["vcf"], 2, None))
    return out


# ---- corrupted streams --------------------------------------------------------------------------------------
def flip_positions(n=3000, seed=7):
    """(file bytes, [(byte, bit)]): n single-bit flips in the DEFLATE payload of block 1 (a full 65280-byte block) of a
    three-block level-6 file.  gzip.decompress raises on every one of them."""
    text = vcf_text(3 * MAX_PAYLOAD - 100, seed=11)
    data, table = write(text, 6)
    comp_off, _, comp_len, _ = table[1]
    lo, hi = comp_off + 18, comp_off + comp_len - 8
    rng = random.Random(seed)
    return data, [(rng.randrange(lo, hi), rng.randrange(8)) for _ in range(n)]


def flipped(data, at, bit):
    bad = bytearray(data)
    bad[at] ^= 1 << bit
    return bytes(bad)


def damaged_cases():
    """[(name, file bytes, expected block index or None, allowed reasons)]"""
    text = vcf_text(2 * 6000 - 50, seed=12)
    data, table = write(text, 6, payload=6000, eof=False)
    out = []
    for cut in range(2, len(data)):                    # (a file of fewer than two bytes is plain text)
        if cut == table[1][0]:
            continue                                   # exactly the first block: a valid file
        out.append(("truncated@%d" % cut, data[:cut], 0 if cut < table[1][0] else 1, REASONS))
    off1 = table[1][0]
    bad = bytearray(data); struct.pack_into("<H", bad, off1 + 16, 65535)
    out.append(("bsize_past_end", bytes(bad), 1, ("block size beyond the end of the file",)))
    bad = bytearray(data); struct.pack_into("<I", bad, off1 - 4, table[0][3] - 1)
    out.append(("isize_smaller", bytes(bad), 0, ("length mismatch",)))
    bad = bytearray(data); struct.pack_into("<I", bad, off1 - 4, table[0][3] + 1)
    out.append(("isize_larger", bytes(bad), 0, ("length mismatch",)))
    bad = bytearray(data); bad[off1 - 8] ^= 0x10
    out.append(("crc_altered", bytes(bad), 0, ("CRC mismatch",)))
    out.append(("trailing_garbage", data + b"garbage!", 2, ("not a gzip member",)))
    out.append(("trailing_magic_only", data + b"\x1f\x8b", 2, ("truncated",)))
    return out


# ---- the corpus as a file for tests/cpp/test_inflate.cpp, and that program -----------------------------------
def _record(kind, arg, name, data, aux):
    name = name.encode()
    return struct.pack("<III", kind, arg, len(name)) + name + struct.pack("<Q", len(data)) + data + struct.pack("<Q", len(aux)) + aux


def write_corpus_file(path):
    with open(path, "wb") as f:
        for name, data, text, kind, _ in corpus():
            f.write(_record(0, kind, name, data, text))
        for name, text in texts().items():
            f.write(_record(0, 0, "plain/" + name, text, text))
        for name, data, blk, reasons in damaged_cases():
            f.write(_record(1, 0, name, data, ("%d\n%s" % (blk, "|".join(reasons))).encode()))
        data, flips = flip_positions()
        f.write(_record(2, 1, "flip", data, b"".join(struct.pack("<QQ", at, bit) for at, bit in flips)))


def build_test_inflate(root, out):
    """tests/cpp/test_inflate.cpp with the address and undefined-behaviour sanitizers (host code only: no device library)."""
    import subprocess
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-I", root + "/edsparser_amd/csrc", root + "/tests/cpp/test_inflate.cpp", "-o", out]
    subprocess.run(cmd, check=True)
    return out


def host_refusals(root, workdir):
    """{case name: error text} of every damaged input, from the sanitized host decoder; asserts that it passes."""
    import os
    import subprocess
    exe = build_test_inflate(root, os.path.join(workdir, "test_inflate"))
    corpus_file = os.path.join(workdir, "corpus.bin")
    write_corpus_file(corpus_file)
    r = subprocess.run([exe, corpus_file], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return dict(line.split("\t", 1) for line in r.stdout.splitlines()), r.stderr
