"""CPU: the GFA export specification (tests/gfa_spec.py) against the language of small EDSs and the path spelling
specification (tests/path_spec.py) on seeded random EDS + sEDS; the closed forms of the byte counts against len() of the
text; and the chunk functions of csrc/gfa_text.hpp, compiled for the host, against the specification byte for byte.  The
library is pinned to this specification in tests/test_gfa_gpu.py."""
import os
import random
import subprocess

import pytest

import gfa_spec as gs
import path_spec as ps
from test_subset_cpu import random_eds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def open_run_eds(rng, P=None, n=None, max_strings=4, max_len=5):
    """A random (eds, seds) with what the links turn on: runs of open symbols (an empty string among theirs), open first
    and last symbols, '{}' symbols, several empty strings in one symbol."""
    P = P or rng.randint(1, 6)
    n = n or rng.randint(1, 10)
    syms, sets = [], []
    open_run = 0
    for i in range(n):
        if open_run == 0 and rng.random() < 0.35:
            open_run = rng.randint(1, 4)
        is_open = open_run > 0 or (i in (0, n - 1) and rng.random() < 0.5)
        open_run = max(0, open_run - 1)
        k = rng.randint(1, max_strings)
        strings = ["".join(rng.choice("ACGT") for _ in range(rng.randint(1, max_len))).encode() for _ in range(k)]
        if is_open:
            for j in rng.sample(range(k), rng.choice([1, 1, 1, min(2, k)])):
                strings[j] = b""
        syms.append(strings)
        if k == 1 and rng.random() < 0.5:
            sets.append({0})
        else:
            for _ in range(k):
                sets.append({0} if rng.random() < 0.1 else set(rng.sample(range(1, P + 1), rng.randint(1, P))))
    if max(max(s) for s in sets) < P:
        sets[-1] = (sets[-1] - {0}) | {P}
    return (b"".join(b"{" + b",".join(s) + b"}" for s in syms),
            b"".join(b"{" + b",".join(b"%d" % p for p in sorted(s)) + b"}" for s in sets))


def cases(seed, count):
    rng = random.Random(seed)
    out = []
    for k in range(count):
        out.append(random_eds(rng) if k % 2 else open_run_eds(rng))
    return out


CASES = cases(20250607, 300)


def test_complete_walks_spell_the_language():
    rng = random.Random(11)
    small = [open_run_eds(rng, n=rng.randint(1, 6), max_strings=3, max_len=2) for _ in range(200)]
    small += [(b"{}{,}", b"{0}{1}{2}"), (b"{,A}{C}", b"{1}{2}{0}"), (b"{A}{C,}", b"{0}{1}{2}"), (b"{A}{,C}{G}", b"{0}{1}{2}{0}")]
    nonempty = 0
    for eds, _ in small:
        syms = gs.parse_eds(eds)
        segs, lks, paths = gs.read(gs.graph(eds)[0])
        assert gs.complete_walk_words(syms, segs, lks) == gs.language(syms) - {b""}, eds
        nonempty += 1 if segs else 0
    assert nonempty >= 150


def test_walks_spell_the_paths_and_follow_links():
    walked = linked = 0
    for eds, seds in CASES:
        syms, sets, P = ps.parse(eds, seds)
        text, info = gs.gfa(eds, seds)
        segs, lks, paths = gs.read(text)
        lines, miss, steps = gs.walks(eds, seds)
        lset, by_name = set(lks), dict(paths)
        assert len(lks) == len(lset) == info["n_links"] and lks == sorted(lks) and len(segs) == info["n_segments"]
        for p in range(1, P + 1):
            seq, m = ps.spell(syms, sets, p)
            walk = by_name.get(b"path%d" % p, [])
            assert b"".join(segs[x] for x in walk) == seq and m == miss[p - 1] and len(walk) == steps[p - 1]
            assert (b"path%d" % p in by_name) == (steps[p - 1] > 0)
            walked += 1
            if m == 0:
                assert all(pair in lset for pair in zip(walk, walk[1:])), (eds, seds, p)
                linked += len(walk) > 1
    assert walked >= 800 and linked >= 300


def test_closed_form_byte_counts():
    rng = random.Random(5)
    extra = [(b"".join(b"{" + b",".join(b"A" * (k % 3) for k in range(w)) + b"}" for w in ws), None)
             for ws in ([12, 7, 30], [101, 1, 99, 2], [1] * 120, [3] * 40, [1005, 2], [2, 1005])]
    for eds, _ in CASES + extra:
        text, info = gs.graph(eds)
        sb, nl, lb = gs.closed_form_counts(gs.parse_eds(eds))
        assert (sb, nl, lb) == (info["segment_bytes"], info["n_links"], info["link_bytes"]), eds
        assert len(text) == info["header_bytes"] + sb + lb
    assert [gs.dsum(x) for x in (0, 1, 9, 10, 99, 100, 12345)] == [sum(len(str(k)) for k in range(1, x + 1))
                                                                   for x in (0, 1, 9, 10, 99, 100, 12345)]


# ---- csrc/gfa_text.hpp on the host ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gfa_text") / "test_gfa_text")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", os.path.join(ROOT, "tests", "cpp", "test_gfa_text.cpp"), "-o", exe],
                   check=True)

    def run(jobs):
        """jobs: (eds, seds or None, lead) -> the texts"""
        inp = b"".join(e + b" " + (s if s is not None else b"-") + b" %d\n" % lead for e, s, lead in jobs)
        out = subprocess.run([exe], input=inp, capture_output=True, check=True).stdout
        texts, k = [], 0
        for _ in jobs:
            nl = out.index(b"\n", k)
            size = int(out[k:nl])
            texts.append(out[nl + 1:nl + 1 + size])
            k = nl + 1 + size
        assert k == len(out)
        return texts
    return run


def test_chunk_functions_against_the_spec(chunker):
    jobs = [(e, s, k % 16) for k, (e, s) in enumerate(CASES) if e]
    wide = lambda w, t: b"{" + b",".join(t for _ in range(w)) + b"}"
    # ids across 9/10, 99/100, 999/1000 inside one block of links, long strings, open runs of wide symbols
    jobs += [(wide(7, b"AC") + wide(120, b"G") + wide(1100, b"T") + wide(3, b"ACGTACGTACGTACGTACGTACGTACGTACGTACGTA"), None, lead)
             for lead in (0, 11, 5)]
    jobs += [(wide(2, b"A") + b"".join(b"{,C,GG}" for _ in range(40)) + wide(2, b"T"), None, 11),
             (b"".join(b"{,C,GG}" for _ in range(30)), None, 3), (b"{" + b"ACGT" * 700 + b"}{A,C}", None, 11)]
    got = chunker(jobs)
    for (eds, seds, lead), text in zip(jobs, got):
        want = gs.gfa(eds, seds)[0][len(gs.HEADER):]
        assert text == want, (eds[:200], seds and seds[:200], lead)
