"""CPU: the record arithmetic of the path session's driver (edsparser_amd/csrc/path_records.hpp: header texts, record
layout, output batches) as host code under the address and undefined-behaviour sanitizers (tests/cpp/test_path_records.cpp,
a program of its own), against the texts themselves: every record is built here as bytes, and where it starts, where its
body starts and which records share an output batch are read off those bytes."""
import itertools
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPELL, ALIGN, WALKS = 0, 1, 2
END = 2 ** 64 - 1


def record_text(rule, name, L, line_width):
    """(header, body) of one record whose sequence, row or token text has L bytes; (b"", b"") for a walk without a step"""
    if rule == WALKS:
        if L == 0:
            return b"", b""
        return b"P\t" + name + b"\t", b"t" * (L - 1) + b"\t*\n"     # L token bytes, the last comma a tab, then "*\n"
    seq = b"A" * L
    lw = L if line_width == 0 else line_width                    # 0: one line; an empty sequence has no line
    body = b"".join(seq[i:i + lw] + b"\n" for i in range(0, L, lw)) if L else b""
    return b">" + name + b"\n", body


def expected(rule, line_width, KT, budget, ids, lens, sizes=None):
    """What the program writes for one case.  sizes (header bytes, body bytes) per record stand in for the texts where these
    would be too large to build"""
    n = len(ids)
    names = [b"path%d" % i for i in ids]
    heads = [(b"P\t" + nm + b"\t") if rule == WALKS else (b">" + nm + b"\n") for nm in names]
    if sizes is None:
        texts = [record_text(rule, nm, L, line_width) for nm, L in zip(names, lens)]
        sizes = [(len(h), len(b)) for h, b in texts]
        for (h, b), hd, L in zip(texts, heads, lens):
            assert h in (hd, b"") and (h == b"") == (rule == WALKS and L == 0)
    blob = b"".join(heads)
    off = [0]
    for h in heads:
        off.append(off[-1] + len(h))
    start = [0]
    for h, b in sizes:
        start.append(start[-1] + h + b)
    out = [len(blob)] + list(blob) + off + [start[n]]
    recs = []
    for k in range(n):
        L = lens[k]
        lw = 0 if rule == WALKS else (max(L, 1) if line_width == 0 or line_width > L else line_width)
        recs.append([L, lw, sizes[k][1], off[k], k % KT])
        out += recs[k] + [start[k]]
    batches = []
    for i0 in range(0, n, KT):
        i1 = min(n, i0 + KT)
        r0 = i0
        while r0 < i1:
            r1 = r0 + 1                                          # one record, then as many more as fit
            while r1 < i1 and start[r1 + 1] - start[r0] <= budget:
                r1 += 1
            inside = [k for k in range(r0, r1) if sizes[k][0] + sizes[k][1]]
            out += [i0, r0, r1, start[r1] - start[r0], len(inside), max([sizes[k][1] for k in inside], default=0)]
            for k in inside:
                L, lw, body, hdr_src, row = recs[k]
                out += [start[k] - start[r0], start[k] - start[r0] + sizes[k][0], hdr_src, L, lw, body, row]
            batches.append((r0, r1, start[r1] - start[r0], inside))
            r0 = r1
    return out + [END], start, sizes, batches


def properties(rule, budget, lens, start, sizes, batches):
    n = len(lens)
    assert sum(b[2] for b in batches) == start[n]
    assert sorted(k for b in batches for k in b[3]) == [k for k in range(n) if not (rule == WALKS and lens[k] == 0)]
    for r0, r1, nbytes, inside in batches:
        for k in inside:
            rec_off = start[k] - start[r0]
            assert 0 <= rec_off < rec_off + sizes[k][0] <= nbytes and rec_off + sizes[k][0] + sizes[k][1] <= nbytes
        if budget == 1:
            assert r1 == r0 + 1
    if rule == WALKS:
        for k in range(n):
            if lens[k] == 0:
                assert start[k + 1] == start[k] and sizes[k] == (0, 0)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    d = tmp_path_factory.mktemp("path_records")
    exe = str(d / "test_path_records")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-I", os.path.join(ROOT, "edsparser_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_path_records.cpp"), "-o", exe], check=True)
    return exe, d


def run_twin(twin, name, flat):
    exe, d = twin
    cf, rf = str(d / (name + ".bin")), str(d / (name + ".out"))
    open(cf, "wb").write(struct.pack("<%dQ" % len(flat), *flat))
    r = subprocess.run([exe, cf, rf], capture_output=True, text=True, env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert r.returncode == 0, r.stderr[-6000:]
    data = open(rf, "rb").read()
    return list(struct.unpack("<%dQ" % (len(data) // 8), data))


def test_path_records_under_sanitizers(twin):
    """Every combination of first length, line width, body rule, record count, table batch and output budget.  The lengths
    are taken around the line width (around 4 where there is none to be around); the records behind the first walk on
    through the same list, so that every batch mixes them - but for align, whose records all have one length"""
    flat, want, cases = [], [], 0
    for lw_kind in (0, 1, 3, 60, "larger"):
        base = lw_kind if lw_kind not in (0, "larger") else 4
        Ls = [0, 1, base - 1, base, base + 1, 2 * base]
        line_width = max(Ls) + 7 if lw_kind == "larger" else lw_kind
        for (li, L), rule, n in itertools.product(enumerate(Ls), (SPELL, ALIGN, WALKS), (1, 2, 5)):
            lens = [L] * n if rule == ALIGN else [Ls[(li + k) % len(Ls)] for k in range(n)]
            ids = [3 + 11 * k for k in range(n)]                 # names of one and two digits
            sizes = expected(rule, line_width, n, 1, ids, lens)[2]
            whole = [h + b for h, b in sizes]
            budgets = [1, whole[0], whole[0] + whole[min(1, n - 1)], max(sum(whole), 1)]
            for KT, budget in itertools.product(sorted({1, min(2, n), n}), budgets):
                e, start, sizes, batches = expected(rule, line_width, KT, budget, ids, lens)
                properties(rule, budget, lens, start, sizes, batches)
                flat += [rule, n, line_width, KT, budget] + ids + lens
                want += e
                cases += 1
    assert cases == 5 * 6 * 3 * (1 + 2 + 3) * 4               # table batches of {1}, {1, 2}, {1, 2, 5} records, four budgets each
    got = run_twin(twin, "cases", flat)
    assert len(got) == len(want) > 100000
    assert got == want


def test_path_records_starts_above_32_bits(twin):
    """Records of 3 * 10^9, 0 and 5 * 10^9 characters under each rule, from the lengths alone: starts and batch bytes on both
    sides of 2^32, budgets of 2^32 and of everything"""
    A, B, T = 3_000_000_000, 5_000_000_000, 2 ** 32
    ids, lens = [1, 22, 333], [A, 0, B]
    flat, want, top = [], [], 0
    for rule, line_width, KT, budget in itertools.product((SPELL, ALIGN, WALKS), (0, 60), (1, 3), (T, 2 ** 63)):
        ls = [B] * 3 if rule == ALIGN else lens
        sizes = []
        for i, L in zip(ids, ls):
            if rule == WALKS:
                sizes.append((len(b"P\tpath%d\t" % i), L + 2) if L else (0, 0))
            else:
                lw = L if line_width == 0 else line_width
                sizes.append((len(b">path%d\n" % i), L + -(-L // lw) if L else 0))
        e, start, sizes, batches = expected(rule, line_width, KT, budget, ids, ls, sizes)
        properties(rule, budget, ls, start, sizes, batches)
        assert start[-1] > A + B > T
        flat += [rule, 3, line_width, KT, budget] + ids + ls
        want += e
        top = max(top, start[-1])
    got = run_twin(twin, "big", flat)
    assert got == want
    assert top > 3 * B
