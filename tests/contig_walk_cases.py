"""Directed inputs of contig selection (csrc/vcf_contig.hip, csrc/vcf_contig_walk.hpp) and the host program that runs its
per-thread code on the CPU (tests/cpp/test_contig_walk.cpp): case families, the build, the case and result files.  No
oracle imports: tests/test_contig_walk_cpu.py and tests/test_contig_walk_gpu.py bring the expected values, from
tests/contig_spec.py and the oracle.  Every family asserts its own premise: that the bytes it is about fall where it says.

A case is a dict: name, V, F, pick (names of the contigs to transform), and optionally fills, weak (the 4-bit hash
instantiation of the host program) and sweep (the host program also checks fi_next_newline / fi_nonnl_before against a
byte-by-byte count over a grid of arguments)."""
import os
import random
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILLS = (0x00, 0x0A, 0xFF, ord(">"), ord("\t"))
BLOCK, LANE, WORD = 1024, 16, 8
HEAD = [b"##fileformat=VCFv4.2", b"\t".join([b"#CHROM", b"POS", b"ID", b"REF", b"ALT", b"QUAL", b"FILTER", b"INFO", b"FORMAT", b"S0", b"S1"])]
OK, REFUSED, INCONSISTENT, DUPLICATE, SWEEP_DIFFERS = 0, 4, 5, 6, 7
REC_FIELDS = ("name_off", "name_len", "rec_start", "rec_end", "seq_start", "line_width", "seq_size", "vcf_records", "duplicate")
NONE = 2 ** 64 - 1


# ---- the program ---------------------------------------------------------------------------------------------------
def build_test_contig_walk(root, out, sanitize=True):
    """tests/cpp/test_contig_walk.cpp (host code only: no device library) with the address and undefined-behaviour
    sanitizers, as vcf_walk_cases.build_test_vcf_walk builds its program, or plain (for a caller that wants verdicts only)"""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread"] + san + ["-I", root + "/edsparser_amd/csrc", root + "/tests/cpp/test_contig_walk.cpp", "-o", out]
    subprocess.run(cmd, check=True)
    return out


def pick_indices(case, records):
    """indices of the FASTA records to transform: the first record of every picked name; records: contig_spec.fasta_records"""
    first = {}
    for i, (nm, _, _) in enumerate(records):
        first.setdefault(nm, i)
    return [first[nm] for nm in case["pick"]]


def write_cases(path, cases, records_of):
    with open(path, "wb") as f:
        for c in cases:
            fills, nm = bytes(c.get("fills", FILLS)), c["name"].encode()
            idx = pick_indices(c, records_of(c))
            f.write(struct.pack("<II", int(c.get("weak", 0)) | 2 * int(c.get("sweep", 0)), len(fills)) + fills + struct.pack("<I", len(nm)) + nm +
                    struct.pack("<Q", len(c["V"])) + c["V"] + struct.pack("<Q", len(c["F"])) + c["F"] +
                    struct.pack("<I%dI" % len(idx), len(idx), *idx))


def read_results(path):
    """{name: [run]} in fill order; a run is a dict (see the layout in test_contig_walk.cpp), arrays as numpy"""
    data = open(path, "rb").read()
    at, out = 0, {}

    def take(fmt):
        nonlocal at
        v = struct.unpack_from("<" + fmt, data, at)
        at += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]

    def arr(n, dt="<u8"):
        nonlocal at
        a = np.frombuffer(data, dtype=dt, count=n, offset=at)
        at += n * a.itemsize
        return a

    def blob():
        nonlocal at
        n = take("Q")
        b = data[at:at + n]
        at += n
        return b

    while at < len(data):
        name = data[at + 4:at + 4 + struct.unpack_from("<I", data, at)[0]].decode()
        at += 4 + len(name.encode())
        r = {"fill": take("I"), "status": take("I")}
        out.setdefault(name, []).append(r)
        if r["status"] != OK:
            r["detail"] = take("Q") if r["status"] == SWEEP_DIFFERS else 0
            continue
        K = r["K"] = take("Q")
        r["recs"] = arr(9 * K).reshape(K, 9)
        r["on_device"], r["passes"], r["undecidable"], r["oob"], nr = take("IIQQQ")
        r["nr"] = nr
        if r["on_device"]:
            r["keys"], r["lsorted"] = arr(nr), arr(nr)
            r["first"], r["counts"], r["unknown"] = arr(K + 1), arr(K), take("Q")
        r["host_total"], r["host_without_token"], r["host_unknown"] = take("QQQ")
        r["host_counts"], r["host_unknown_text"] = arr(K), blob()
        r["contigs"] = []
        for _ in range(take("I")):
            index, verdict, host_tok = take("III")
            r["contigs"].append({"index": index, "verdict": verdict, "host_tokeniser": host_tok, "eds": blob(), "seds": blob(), "text": blob()})
    return out


def run_program(exe, workdir, cases, records_of, tag="cases"):
    """Runs the cases; a sanitizer report ends the program with a non-zero status, which fails here with the report."""
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names), "case names must be unique"
    cf, rf = os.path.join(workdir, tag + ".bin"), os.path.join(workdir, tag + ".out")
    write_cases(cf, cases, records_of)
    r = subprocess.run([exe, cf, rf], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-6000:]
    res = read_results(rf)
    assert sum(len(v) for v in res.values()) == sum(len(c.get("fills", FILLS)) for c in cases)
    return res


# ---- pieces --------------------------------------------------------------------------------------------------------
def _seq(rng, n):
    return bytes(rng.choices(b"ACGT", k=n))


def _wrap(seq, w, eol=b"\n"):
    return eol.join(seq[i:i + w] for i in range(0, len(seq), w))


def _line(name, p, seq, rng):
    ref = seq[p - 1:p]
    alt = bytes([rng.choice([b for b in b"ACGT" if b != ref[0]])])
    return b"\t".join([name, b"%d" % p, b".", ref, alt, b".", b"PASS", b".", b"GT", b"%d|%d" % (rng.randint(0, 1), rng.randint(0, 1)),
                       b"%d|%d" % (rng.randint(0, 1), rng.randint(0, 1))])


def _lines(name, seq, k, rng):
    """k record lines of contig `name` at ascending, pairwise distinct positions of seq"""
    return [_line(name, p, seq, rng) for p in sorted(rng.sample(range(1, len(seq) + 1), min(k, len(seq))))]


def _vcf(lines, pad=None, end=b"\n"):
    head = [HEAD[0]] + ([b"##pad=" + b"x" * pad] if pad is not None else []) + [HEAD[1]]
    return b"\n".join(head + lines) + end


def structural_bytes(F):
    """offsets of every '>' that starts a record, every header newline, every name end and every record end of F (a record
    end is the offset of its last byte + 1); no contig_spec import: the definition is written out again here"""
    starts = [i for i in range(len(F)) if F[i:i + 1] == b">" and (i == 0 or F[i - 1:i] == b"\n")]
    out = set()
    for k, s in enumerate(starts):
        e = starts[k + 1] if k + 1 < len(starts) else len(F)
        nl = F.find(b"\n", s, e)
        hl = nl if nl >= 0 else e
        sp = F.find(b" ", s, hl)
        out |= {s, hl, sp if sp >= 0 else hl, e}
    return sorted(out)


# ---- FASTA index: shift sweep --------------------------------------------------------------------------------------
def sweep_body(rng):
    """about ten records with a bit of everything; ([(name, sequence)] of the records a VCF can name, the text)"""
    sa, sx, sw, so, sl = _seq(rng, 200), _seq(rng, 90), _seq(rng, 2500), _seq(rng, 3000), _seq(rng, 8)
    parts = [b">chrA some description\n" + _wrap(sa, 60) + b"\n",
             b">t\tab\n" + _wrap(_seq(rng, 5), 1) + b"\n",
             b">\n" + _wrap(_seq(rng, 70), 60) + b"\n",
             b">" + b"x" * 1500 + b"\n" + _wrap(sx, 60) + b"\n",
             b">a\n>b\n",
             b">blank\nACGT\n\nACGT\n",
             b">gt\nACGT\nAC>GT\nAC\n",
             b">w1024\n" + _wrap(sw, 1024) + b"\n",
             b">one\n" + so + b"\n",
             b">last d\n" + sl + b"\n"]
    return [(b"chrA", sa), (b"x" * 1500, sx), (b"w1024", sw), (b"one", so), (b"last", sl)], b"".join(parts)


def shift_values(body, front_len):
    """every p that puts a structural byte of the body 1 before, at or 1 after a multiple of 16 and of 1024, and 0..17"""
    ps = set(range(18))
    for o in structural_bytes(body):
        for m in (LANE, BLOCK):
            for d in (-1, 0, 1):
                ps.add((d - front_len - o) % m)
    return sorted(ps)


def shift_sweep(seed=7001, only=None):
    rng = random.Random(seed)
    contigs, body = sweep_body(rng)
    lines = [ln for nm, sq in contigs for ln in _lines(nm, sq, 3, rng)] + [_line(b"t", 1, b"A", rng), _line(b"nowhere", 2, b"AC", rng)]
    rng.shuffle(lines)
    V = _vcf(lines)
    front = lambda p: b">p\n" + b"A" * p + b"\n"
    ps = shift_values(body, len(front(0)))
    structural = structural_bytes(body)
    seen = {m: {o: set() for o in structural} for m in (LANE, BLOCK)}
    out = []
    for p in ps:
        F = front(p) + body
        for m in (LANE, BLOCK):
            for o in structural:
                seen[m][o].add((len(front(p)) + o) % m)
        if only is None or p in only:
            out.append({"name": "shift/%d" % p, "V": V, "F": F, "pick": [b"chrA", b"x" * 1500, b"one", b"last", b"p"][:4 if p == 0 else 5]})
    for m in (LANE, BLOCK):
        for o in structural:
            assert seen[m][o] >= {m - 1, 0, 1}, (m, o)
    assert len(structural) > 20 and set(range(18)) <= set(ps)
    return out


# ---- FASTA index: ends ---------------------------------------------------------------------------------------------
END_TARGETS = (1455, 1456, 1457, 2047, 2048, 2049)


def ends(seed=7002):
    rng = random.Random(seed)
    out = []
    sa, sz = _seq(rng, 150), _seq(rng, 7)
    for target in END_TARGETS:
        for ending in ("nl", "open", "header_only", "bare_gt", "crlf"):
            eol = b"\r\n" if ending == "crlf" else b"\n"
            tail = {"nl": b">z\n" + sz + b"\n", "open": b">z\n" + sz, "header_only": b">z\n" + sz + b"\n>last", "bare_gt": b">z\n" + sz + b"\n>",
                    "crlf": b">z d\r\n" + sz + b"\r\n"}[ending]
            headp = b">chrA desc" + eol + _wrap(sa, 60, eol) + eol + b">pad x" + eol
            k = target - len(headp) - len(eol) - len(tail)
            F = headp + b"C" * k + eol + tail
            assert len(F) == target and k > 0
            lines = _lines(b"chrA", sa, 3, rng) + _lines(b"z", sz, 2, rng) + [_line(b"pad", 1, b"C", rng)]
            out.append({"name": "ends/%d/%s" % (target, ending), "V": _vcf(lines), "F": F, "pick": [b"chrA", b"pad", b"z"]})
    assert {len(c["F"]) % LANE for c in out} == {0, 1, 15} and {len(c["F"]) % BLOCK for c in out} >= {0, 1, 1023}
    # '\n' as the last byte of a block (of a lane) and '>' as the first byte of the next: the f[i0 - 1] read across the edge
    for what, at in (("block", BLOCK), ("block2", 2 * BLOCK), ("lane", 3 * LANE), ("lane_in_block2", BLOCK + 5 * LANE)):
        k = at - len(b">f\n") - 1
        F = b">f\n" + b"G" * k + b"\n>edge x\n" + sa[:50] + b"\n"
        assert F[at - 1:at + 1] == b"\n>" and at % LANE == 0
        out.append({"name": "ends/edge/" + what, "V": _vcf(_lines(b"edge", sa[:50], 3, rng) + [_line(b"f", 2, b"GG", rng)]), "F": F, "pick": [b"edge", b"f"]})
    return out


# ---- FASTA index: long walks ---------------------------------------------------------------------------------------
def long_walks(seed=7003):
    rng = random.Random(seed)
    out = []
    sa = _seq(rng, 120)
    # a header line over 1, 2, 3 and 4 whole blocks, its newline at the first and at the last byte of a block
    for start in (0, 37):
        front = b"" if start == 0 else b">f\n" + b"T" * (start - 4) + b"\n"
        assert len(front) == start
        for nb in (1, 2, 3, 4):
            for where, nl_at in (("first", nb * BLOCK), ("last", nb * BLOCK + BLOCK - 1)):
                hdr = b">hd " + b"d" * (nl_at - start - 4)
                F = front + hdr + b"\n" + _wrap(sa, 60) + b"\n>after\nACGTAC\n"
                assert F[nl_at:nl_at + 1] == b"\n" and F.find(b"\n", start) == nl_at
                out.append({"name": "walk/header/%d/%d/%s" % (start, nb, where), "V": _vcf(_lines(b"hd", sa, 4, rng) + _lines(b"after", b"ACGTAC", 2, rng)),
                            "F": F, "pick": [b"hd", b"after"], "sweep": 1})
    # a sequence line that crosses three blocks, then the first newline behind seq_start in the same block, in the next
    # block, or nowhere (the record runs to the end of the file: `limit`)
    long_seq = _seq(rng, 3 * BLOCK + 200)
    for what, rec in (("same_block", b">s\n" + sa[:40] + b"\n" + sa[40:] + b"\n"),
                      ("next_block", b">s\n" + sa * 9 + b"\n" + sa + b"\n"),
                      ("three_blocks", b">s\n" + long_seq + b"\n" + sa + b"\n"),
                      ("absent_short", b">s\n" + sa),
                      ("absent_long", b">s\n" + long_seq),
                      ("header_only_long", b">s " + b"h" * (2 * BLOCK + 77))):
        F = b">l\n" + long_seq + b"\n" + rec
        sq = rec.split(b"\n", 1)[1].replace(b"\n", b"") if b"\n" in rec else b""
        lines = _lines(b"l", long_seq, 5, rng) + (_lines(b"s", sq, 3, rng) if sq else [_line(b"s", 1, b"A", rng)])
        out.append({"name": "walk/line/" + what, "V": _vcf(lines), "F": F, "pick": [b"l", b"s"], "sweep": 1})
    first_nl = {c["name"]: c["F"].find(b"\n", c["F"].rfind(b"\n>s") + 4) for c in out if c["name"].startswith("walk/line/")}
    ss = {c["name"]: c["F"].rfind(b"\n>s") + 4 for c in out if c["name"].startswith("walk/line/")}
    assert first_nl["walk/line/same_block"] // BLOCK == ss["walk/line/same_block"] // BLOCK
    assert first_nl["walk/line/next_block"] // BLOCK == ss["walk/line/next_block"] // BLOCK + 1
    assert first_nl["walk/line/three_blocks"] // BLOCK >= ss["walk/line/three_blocks"] // BLOCK + 3
    assert first_nl["walk/line/absent_short"] == first_nl["walk/line/absent_long"] == -1
    return out


# ---- FASTA index: two scan tiles -----------------------------------------------------------------------------------
def scan_tile(seed=7004):
    """2 MiB + 17 bytes: 2049 blocks, so two tiles of 2048 in both block scans, records on both sides of the tile edge"""
    rng = random.Random(seed)
    target = 2 * 1024 * 1024 + 17
    edge = 2048 * BLOCK
    pool = _seq(rng, 4000)
    parts, seqs, n, k = [], {}, 0, 0
    while True:
        L = rng.randint(300, 1800)
        o = rng.randrange(len(pool) - L)
        rec = b">s%d\n" % k + _wrap(pool[o:o + L], rng.choice((60, 70, 1024))) + b"\n"
        if n + len(rec) + 40 > edge:
            break
        parts.append(rec)
        seqs[k] = pool[o:o + L]
        n += len(rec)
        k += 1
    tail = [b">x\nACGT\n", b">y\nACGTACGTA\n"]                       # x straddles the edge, y lies behind it
    parts.append(b">fin\n" + b"N" * (edge - 4 - n - 6) + b"\n")
    F = b"".join(parts + tail)
    assert len(F) == target and (len(F) + BLOCK - 1) // BLOCK == 2049
    assert F.index(b">x\n") == edge - 4 and F.index(b">y\n") == edge + 4
    picks = [0, k // 2, k - 1]
    lines = [ln for i in picks for ln in _lines(b"s%d" % i, seqs[i], 3, rng)] + [ln for i in rng.sample(range(k), 200) for ln in _lines(b"s%d" % i, seqs[i], 2, rng)]
    lines += _lines(b"x", b"ACGT", 2, rng) + _lines(b"y", b"ACGTACGTA", 3, rng)
    rng.shuffle(lines)
    return [{"name": "tile/2MiB+17", "V": _vcf(lines), "F": F, "pick": [b"s%d" % i for i in picks] + [b"fin", b"x", b"y"]}]


# ---- classification: names -----------------------------------------------------------------------------------------
STEM = b"chromosome_number_twelve"             # 24 bytes: every prefix is a name, so every pair of names is a prefix pair


def _names_fasta(rng):
    names = [STEM[:k] for k in range(1, 25)] + [STEM[:k - 1] + b"+" for k in range(1, 25)]     # equal length, last byte differs
    seqs = {nm: _seq(rng, rng.randint(40, 100)) for nm in names}
    recs = [(nm, seqs[nm]) for nm in names]
    rng.shuffle(recs)
    recs.insert(rng.randint(len(recs) // 2, len(recs)), (STEM[:3], _seq(rng, 30)))            # a duplicate name ("chr")
    recs.append((b"quiet", _seq(rng, 50)))                                                    # a contig without lines
    F = b"".join(b">" + nm + rng.choice([b"", b" desc"]) + b"\n" + _wrap(sq, rng.choice((7, 60))) + b"\n" for nm, sq in recs)
    return names, seqs, F


def names(seed=7005):
    rng = random.Random(seed)
    nms, seqs, F = _names_fasta(rng)
    assert len(STEM) == 24 and {len(n) for n in nms} == set(range(1, 25))
    body = [ln for nm in nms for ln in _lines(nm, seqs[nm], 2, rng)]
    body += [_line(nm + b"!", 3, b"ACG", rng) for nm in nms[:24:5]]                           # a FASTA name plus one byte
    body += [_line(b"ghost", p, b"ACGTACGT", rng) for p in (1, 4)]                            # lines without a contig
    rng.shuffle(body)
    order = STEM[:5]                                                                          # equal and descending positions: file order counts
    sq = seqs[order]
    body += [b"\t".join([order, b"%d" % p, b".", sq[p - 1:p], alt, b".", b"PASS", b".", b"GT", b"0|1", b"1|0"])
             for p, alt in ((20, b"AT"), (20, b"ATT"), (9, b"GG"), (20, b"ATTT"), (9, b"GGG"), (2, b"CC"))]
    last_nm = STEM[:11]
    lasts = {"record": _line(last_nm, 5, seqs[last_nm], rng), "name_tab": last_nm + b"\t", "bare_name": last_nm}
    out = []
    for form, last in lasts.items():
        for pad in range(8):
            V = _vcf(body + [last], pad=pad, end=b"")
            out.append({"name": "names/%s/%d" % (form, pad), "V": V, "F": F, "pick": [STEM[:1], STEM[:3], STEM[:4], order, last_nm, STEM, STEM[:23] + b"+", b"quiet"]})
        fam = [c for c in out if c["name"].startswith("names/" + form)]
        assert {len(c["V"]) % WORD for c in fam} == set(range(WORD)), form
        starts = set()
        for c in fam:
            at = 0
            for ln in c["V"].split(b"\n"):
                if ln and not ln.startswith(b"#"):
                    starts.add((ln.split(b"\t")[0], at % WORD))
                at += len(ln) + 1
        assert all({r for n, r in starts if n == nm} == set(range(WORD)) for nm in nms), form       # every name at every residue
    out.append({"name": "names/final_newline", "V": _vcf(body), "F": F, "pick": [STEM[:3], order, b"quiet"]})
    return out


# ---- classification: host-bound ------------------------------------------------------------------------------------
def host_bound(seed=7006):
    rng = random.Random(seed)
    nms, seqs, F = _names_fasta(rng)
    body = [ln for nm in nms[:8] for ln in _lines(nm, seqs[nm], 2, rng)]
    nm = nms[3]
    rest = _line(nm, 4, seqs[nm], rng)[len(nm):]
    odd = {"empty_first_field": rest, "space": nm[:2] + b" " + nm[2:] + rest, "vtab": nm + b"\v" + rest, "formfeed": b"\f" + nm + rest,
           "cr": nm + b"\r" + rest, "whitespace_only": b"  \t "}
    out = [{"name": "hostbound/" + what, "V": _vcf(body[:5] + [ln] + body[5:]), "F": F, "pick": [nm, nms[0]]} for what, ln in odd.items()]
    out.append({"name": "hostbound/crlf_file", "V": _vcf(body).replace(b"\n", b"\r\n"), "F": F, "pick": [nm, nms[0]]})
    return out


# ---- record count switches -----------------------------------------------------------------------------------------
def _many(rng, K, nr, name):
    seqs = [_seq(rng, rng.randint(10, 40)) for _ in range(K)]
    F = b"".join(b">s%d\n%s\n" % (k, seqs[k]) for k in range(K))
    assert len(F) < 3_000_000
    subset = rng.sample(range(K), min(K, 300))
    picks = sorted({k for k in (0, 254, 255, 256, K - 1) if k < K}) + rng.sample(subset, 5)
    lines = []
    for k in picks:
        lines += _lines(b"s%d" % k, seqs[k], 2, rng)
    lines += [_line(b"s%d" % (K + j % 7), 1, b"A", rng) for j in range(20)]                    # absent contigs: the key K itself
    while len(lines) < nr:
        k = rng.choice(subset)
        lines.append(_line(b"s%d" % k, rng.randint(1, len(seqs[k])), seqs[k], rng))
    rng.shuffle(lines)
    assert len(lines) == nr
    return {"name": name, "V": _vcf(lines), "F": F, "pick": [b"s%d" % k for k in picks]}


def record_counts(seed=7007):
    rng = random.Random(seed)
    out = [_many(rng, K, 3000, "counts/K%d" % K) for K in (255, 256, 65535, 65536)]
    out += [_many(rng, 256, nr, "counts/K256/nr%d" % nr) for nr in (2047, 2048, 2049)]
    for c in out:
        if "K65" in c["name"]:
            c["fills"] = (0x0A, 0xFF)                                                         # (they dominate the CPU file's time)
    return out


# ---- all of them ---------------------------------------------------------------------------------------------------
def families():
    """{family: [case]} of everything the device and the full-hash host program run"""
    return {"shift": shift_sweep(), "ends": ends(), "walks": long_walks(), "tile": scan_tile(), "names": names(), "hostbound": host_bound(),
            "counts": record_counts()}


def weak_hash_cases():
    """host program only, 4-bit hash: the names family and K = 256"""
    out = [dict(c, name="weak/" + c["name"], weak=1) for c in names()]
    out += [dict(c, name="weak/" + c["name"], weak=1) for c in record_counts() if c["name"] == "counts/K256"]
    return out
