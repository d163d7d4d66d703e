"""CPU: the contract of the pattern search (tests/locate_oracle.py, the restatement the GPU tests compare against) agrees
with EDS::check_position as the project pins it - in both directions against tests/query_oracle.py, and for a sample of
hits against the edsparser::EDS container - and the edsparser-locate argument errors that end before any device work."""
import itertools
import os
import random
import subprocess

import pytest

import locate_oracle as lo
import query_oracle as qo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "edsparser_amd", "host")
BUILD = os.path.join(HOST, "build")
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "edsparser_amd")
LENGTHS = (1, 2, 3, 5)


def _build_host():
    import edsparser_amd.build as b
    b.build()
    subprocess.run(["make", "-s", "-C", HOST], check=True)


def _patterns(rng, L):
    if L <= 3:
        return ["".join(p) for p in itertools.product("AC", repeat=L)]
    return ["".join(rng.choice("AC") for _ in range(L)) for _ in range(8)]


@pytest.fixture(scope="module")
def cases():
    """[(eds, seds, Eds, patterns, oracle result)]: 150 random EDSs of 1-8 symbols, each with and without sources"""
    rng = random.Random(20240)
    out = []
    for k in range(150):
        n = rng.randint(1, 8)
        eds, seds = lo.random_eds(rng, n, True)
        pats = [p for L in LENGTHS for p in _patterns(rng, L)]
        for sd in (None, seds):
            e = qo.Eds(eds, sd)
            out.append((eds, sd, e, pats, lo.locate(e, pats, max_hits=10 ** 6)))
    return out


def _hits(r, q):
    for h in range(r["hit_off"][q], r["hit_off"][q + 1]):
        yield r["hits"][h], r["choices"][r["choice_off"][h]:r["choice_off"][h + 1]]


def test_common_start_hits_check_true(cases):
    total = common = 0
    for eds, seds, e, pats, r in cases:
        assert r["flags"] == [0] * len(pats) and r["totals"] == [b - a for a, b in zip(r["hit_off"], r["hit_off"][1:])]
        for q, P in enumerate(pats):
            for (pos, s, j, o), ch in _hits(r, q):
                total += 1
                if pos == lo.U64_MAX:
                    assert e.deg[s]
                    continue
                common += 1
                assert not e.deg[s] and j == 0 and pos == e.cum_common[s] + o
                assert qo.check(e, pos, ch, P) is True, (eds, seds, P, pos, ch)
    print("hits", total, "common-start", common)
    assert common > 2000 and total > common


def test_every_true_check_is_a_hit(cases):
    found = 0
    for eds, seds, e, pats, r in cases:
        for q, P in enumerate(pats):
            hits = {(pos, tuple(ch)) for (pos, _, _, _), ch in _hits(r, q) if pos != lo.U64_MAX}
            want = set()
            for pos in range(e.C):
                for ch in lo.walks(e, pos, len(P)):
                    if qo.check(e, pos, ch, P) is True:
                        want.add((pos, tuple(ch)))
            assert hits == want, (eds, seds, P, sorted(hits ^ want))
            found += len(want)
    assert found > 2000


def test_order_and_caps():
    e = qo.Eds("{A,A}{A,A}{A,A}")
    full = lo.locate(e, ["AAA"], max_hits=9)
    assert full["totals"] == [8] and full["flags"] == [0] and len(full["hits"]) == 8
    keys = [(h[1:], tuple(full["choices"][a:b])) for h, a, b in zip(full["hits"], full["choice_off"], full["choice_off"][1:])]
    assert keys == sorted(keys) and len(set(keys)) == 8
    exact = lo.locate(e, ["AAA"], max_hits=8)
    assert (exact["totals"], exact["flags"], exact["hits"]) == ([8], [0], full["hits"])
    cut = lo.locate(e, ["AAA"], max_hits=3)
    assert cut["flags"] == [1] and cut["hits"] == full["hits"][:3] and cut["choices"] == full["choices"][:6]
    assert cut["totals"] == [6]                                 # two starts, each stops at 3 of its 4
    deep = lo.locate(qo.Eds("C" + "{A,}" * 64 + "G"), ["CG"])
    assert deep["totals"] == [1] and deep["flags"] == [0] and deep["choices"] == [2 * i + 1 for i in range(64)]
    deeper = lo.locate(qo.Eds("C" + "{A,}" * 65 + "G"), ["CG"])
    assert deeper["totals"] == [0] and deeper["flags"] == [2]


@pytest.fixture(scope="module")
def container():
    _build_host()
    exe = os.path.join(BUILD, "test_query_locate")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, os.path.join(ROOT, "tests", "cpp", "test_query.cpp"),
                    os.path.join(BUILD, "libedsparser_lib.a"), "-L", LIBDIR, "-ledsx", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    return exe


def test_sample_of_hits_through_the_container(cases, container, tmp_path):
    rng = random.Random(5)
    cmds = []
    for eds, seds, e, pats, r in cases:
        for q, P in enumerate(pats):
            for (pos, _, _, _), ch in _hits(r, q):
                if pos != lo.U64_MAX and rng.random() < 0.15:
                    cmds.append(("C", eds, "-" if seds is None else seds, pos, ",".join(str(c) for c in ch), P))
    assert len(cmds) > 300 and any(c[2] != "-" for c in cmds)
    f = tmp_path / "cmds.txt"
    f.write_text("".join("\t".join(str(x) for x in c) + "\n" for c in cmds))
    r = subprocess.run([container, str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[:-1] == ["true"] * len(cmds)


def test_locate_cli_argument_errors(tmp_path):
    _build_host()
    exe = os.path.join(BUILD, "edsparser-locate")
    eds, pats, bad, out = tmp_path / "x.eds", tmp_path / "p.txt", tmp_path / "bad.txt", tmp_path / "hits.tsv"
    eds.write_text("{ACGT}{A,C}")
    pats.write_text("AC\r\nGT")
    bad.write_text("AC\nGT\n\r\nA\n")
    io = ["-i", str(eds), "-p", str(pats), "-o", str(out)]
    cases = [
        ([], "the option '--input' is required but missing"),
        (["-i", str(eds), "-o", str(out)], "the option '--patterns' is required but missing"),
        (["-i", str(tmp_path / "missing.eds"), "-p", str(pats), "-o", str(out)], "Error: Input file does not exist:"),
        (["-i", str(eds), "-p", str(tmp_path / "missing.txt"), "-o", str(out)], "Error: Pattern file does not exist:"),
        (io + ["-s", str(tmp_path / "missing.seds")], "Error: Sources file does not exist:"),
        (io + ["--max-hits", "x"], "for option '--max-hits' is invalid"),
        (io + ["--max-hits", "-1"], "for option '--max-hits' is invalid"),
        (io + ["--max-hits", "0"], "Error: --max-hits must be at least 1"),
        (["-i", str(eds), "-p", str(bad), "-o", str(out)], "Error: Pattern file line 3 is empty"),
        (io + ["--bogus"], "unrecognised option '--bogus'"),
    ]
    for args, msg in cases:
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)
        assert "[Performance] Runtime:" in r.stderr
    assert not out.exists()
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--input", "--sources", "--patterns", "--output", "--max-hits", "--common-only", "--count-only"):
        assert flag in r.stdout
