"""GPU: edsx_eds_genpatterns / edsx_eds_check_positions (k_pat_sample / k_pat_check) against the edsparser::EDS
container's seeded sampler and check_position, and the edsparser-genpatterns CLI."""
import glob
import json
import os
import random
import subprocess

import numpy as np
import pytest

import query_oracle as qo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "edsparser_amd", "host")
BUILD = os.path.join(HOST, "build")
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "edsparser_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = json.load(open(os.path.join(GOLDEN, "query_cases.json")))
SEEDS = (0, 1, 2**63 + 5)
KIND = {1: True, 0: False, -1: "out_of_range", -2: "invalid_argument"}

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    return edsparser_amd.Context(0)


@pytest.fixture(scope="module")
def runner(tmp_path_factory):
    import edsparser_amd.build as b
    b.build()
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    exe = os.path.join(BUILD, "test_query")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", INC, os.path.join(ROOT, "tests", "cpp", "test_query.cpp"),
                    os.path.join(BUILD, "libedsparser_lib.a"), "-L", LIBDIR, "-ledsx", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    d = tmp_path_factory.mktemp("qgpu")

    def run(cmds):
        f = d / "cmds.txt"
        f.write_text("".join("\t".join(str(x) for x in c) + "\n" for c in cmds))
        r = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.split("\n")[:-1]
    run.dir = d
    return run


def _norm(r):
    return (r == "true") if r in ("true", "false") else r.split(":", 1)[0]


def _host_patterns(runner, eds, count, length, seed):
    (r,) = runner([("G", eds, count, length, seed)])
    return r


def _device_patterns(ctx, eds, count, length, seed):
    import edsparser_amd
    try:
        return "=" + ctx.eds_genpatterns(eds.encode(), count, length, seed).decode().replace("\n", "|")
    except edsparser_amd.EdsxError as x:
        assert x.code == 3, x
        return "runtime_error: " + x.message


def test_sampler_bytes_equal_host_twin(ctx, runner):
    inputs = [open(f).read().strip() for f in sorted(glob.glob(os.path.join(GOLDEN, "ref_data", "eds", "*.eds")))]
    inputs += ["ACGT{A,C}GG", "{A,C}{G,T}", "{,A}{,}{TTT}{G,GG,GGG}"]
    cmds, dev = [], []
    for eds in inputs:
        for count in (1, 63, 64, 65):
            for seed in SEEDS:
                for length in (5, 37):                       # 37: longer than most of these EDSs (the wrap path)
                    cmds.append(("G", eds, count, length, seed))
                    dev.append(_device_patterns(ctx, eds, count, length, seed))
    for eds in inputs[:4] + inputs[-3:]:
        for seed in SEEDS:
            cmds.append(("G", eds, 10000, 12, seed))
            dev.append(_device_patterns(ctx, eds, 10000, 12, seed))
    host = runner(cmds)
    for c, h, d in zip(cmds, host, dev):
        assert d == h, (c[1], c[2:], h[:200], d[:200])
    # the wrap reaches symbol 1 of {A}{,}, which has no non-empty string: an error instead of the reference's endless loop
    h = _host_patterns(runner, "{A}{,}", 1, 3, 0)
    d = _device_patterns(ctx, "{A}{,}", 1, 3, 0)
    assert h.startswith("runtime_error:") and "symbol 1" in h and d == h
    assert ctx.eds_genpatterns(b"{ACGT}", 0, 4, 1) == b""
    import edsparser_amd
    for eds, length, msg in ((b"", 4, "Cannot generate patterns from empty EDS"),
                             (b"{ACGT}", 0, "Pattern length must be greater than 0")):
        with pytest.raises(edsparser_amd.EdsxError) as ei:
            ctx.eds_genpatterns(eds, 3, length, 1)
        assert ei.value.code == 3 and ei.value.message == msg


def _witness_queries(pos, off, deg, text, length):
    """(kept indices, positions, choice_off, choices, pattern_off, patterns) of the non-wrapped witnesses (a wrapped
    pattern has no choices, so the kept patterns' choices are all of deg)"""
    keep = np.nonzero(pos != np.uint64(2**64 - 1))[0]
    arr = np.frombuffer(text, dtype=np.uint8).reshape(-1, length + 1)[keep, :length]
    coff = np.append(off[keep], off[-1]).astype(np.uint64)
    poff = np.arange(len(keep) + 1, dtype=np.uint64) * np.uint64(length)
    return keep, pos[keep], coff, deg.astype(np.int32), poff, arr.tobytes()


def test_witnesses_check_true(ctx, runner):
    for eds in ("{ACGT}{A,ACA}{CGT}{T,TG}", "ACGT{A,C}GG", "{,A}{,}{TTT}{G,GG,GGG}", "{AC}{A,,C}{G}{T,TT,}CCA{G,A}"):
        for seed in SEEDS:
            text, pos, off, deg = ctx.eds_genpatterns(eds.encode(), 200, 4, seed, witness=True)
            keep, p, coff, ch, poff, pats = _witness_queries(pos, off, deg, text, 4)
            assert len(keep) > 0
            st = ctx.eds_check_positions(eds.encode(), p, coff, ch, poff, pats)
            assert (st == 1).all(), (eds, seed)
            cmds = [("C", eds, "-", int(p[k]), ",".join(str(x) for x in ch[int(coff[k]):int(coff[k + 1])]),
                     pats[4 * k:4 * k + 4].decode()) for k in range(len(keep))]
            assert runner(cmds) == ["true"] * len(cmds)
            want = qo.generate(qo.Eds(eds), 200, 4, seed)[1]
            for k, (wp, wc) in enumerate(want):
                assert (wp is None) == (int(pos[k]) == 2**64 - 1)
                if wp is not None:
                    assert int(pos[k]) == wp and list(deg[int(off[k]):int(off[k + 1])]) == wc


def _device_check(ctx, eds, seds, queries):
    pos = [q[0] for q in queries]
    coff = np.zeros(len(queries) + 1, dtype=np.uint64)
    coff[1:] = np.cumsum([len(q[1]) for q in queries])
    ch = np.array([c for q in queries for c in q[1]], dtype=np.int32)
    pats = "".join(q[2] for q in queries).encode()
    poff = np.zeros(len(queries) + 1, dtype=np.uint64)
    poff[1:] = np.cumsum([len(q[2]) for q in queries])
    st = ctx.eds_check_positions(eds.encode() if isinstance(eds, str) else eds, pos, coff, ch, poff, pats,
                                 seds=(seds.encode() if isinstance(seds, str) else seds))
    return [KIND[int(x)] for x in st]


def test_device_check_fixture_cases(ctx):
    for c in CASES["check"]:
        (got,) = _device_check(ctx, c["eds"], c["seds"], [(c["pos"], c["choices"], c["pattern"])])
        assert got == c["expected"], c["src"]
    # malformed CSR offsets are invalid_argument, not a read past the arrays
    st = ctx.eds_check_positions(b"{ACGT}{A,C}", [0, 0], [0, 5, 1], [0], [0, 2, 3], b"ACG")
    assert list(st) == [-2, -2]


def _random_queries(rng, text, pos, off, deg, length, n, total_deg, C):
    rec = length + 1
    qs = []
    for _ in range(n):
        i = rng.randrange(len(pos))
        p = int(pos[i])
        pat = text[i * rec:i * rec + length].decode()
        ch = [int(x) for x in deg[int(off[i]):int(off[i + 1])]]
        if p == 2**64 - 1:
            p = rng.randrange(C + 3)
        r = rng.random()
        if r < 0.2:
            j = rng.randrange(len(pat))
            pat = pat[:j] + rng.choice("ACGTN") + pat[j + 1:]
        elif r < 0.3 and ch:
            ch[rng.randrange(len(ch))] = rng.randrange(total_deg)
        elif r < 0.35 and ch:
            ch[rng.randrange(len(ch))] = total_deg + rng.randrange(5)
        elif r < 0.4 and ch:
            ch[rng.randrange(len(ch))] = -rng.randint(1, 5)
        elif r < 0.5 and ch:
            ch.pop()
        elif r < 0.55:
            ch.append(rng.randrange(-1, total_deg + 1))
        elif r < 0.6:
            pat = ""
        elif r < 0.65:
            p = C + rng.randrange(3)
        elif r < 0.7:
            p = max(0, p + rng.choice([-1, 1]))
        qs.append((p, ch, pat))
    return qs


def test_device_check_equals_container_16mb(ctx, runner):
    eds, seds, _ = ctx.genrandomeds(16_000_000, seed=5)
    d = runner.dir
    (d / "r.eds").write_bytes(eds)
    (d / "r.seds").write_bytes(seds)
    text, pos, off, deg = ctx.eds_genpatterns(eds, 60_000, 24, 3, witness=True)
    info = ctx.query_last_info()
    rng = random.Random(3)
    qs = _random_queries(rng, text, pos, off, deg, 24, 100_000, int(info["num_degenerate_strings"]), int(info["num_common_chars"]))
    (d / "q.txt").write_text("".join("%d\t%s\t%s\n" % (p, ",".join(str(x) for x in ch), pat) for p, ch, pat in qs))
    for sd in (None, seds):
        dev = _device_check(ctx, eds, sd, qs)
        host = [_norm(r) for r in runner([("F", str(d / "r.eds"), str(d / "r.seds") if sd is not None else "-", str(d / "q.txt"))])]
        assert len(host) == len(qs)
        bad = [k for k in range(len(qs)) if host[k] != dev[k]]
        assert not bad, [(qs[k], host[k], dev[k]) for k in bad[:5]]
        assert {str(x) for x in dev} == {"True", "False", "out_of_range", "invalid_argument"}


def test_scale_256mb_chunks(ctx, runner):
    eds, _, _ = ctx.genrandomeds(256_000_000, seed=9)
    L, count = 32, 4_000_000                               # 3.8 chunks of 2**20 patterns
    text, pos, off, deg = ctx.eds_genpatterns(eds, count, L, 77, witness=True)
    assert len(text) == count * (L + 1)
    lines = np.frombuffer(text, dtype=np.uint8).reshape(count, L + 1)
    assert (lines[:, L] == ord("\n")).all() and not (lines[:, :L] == ord("\n")).any()
    keep, p, coff, ch, poff, pats = _witness_queries(pos, off, deg, text, L)
    assert len(keep) > count * 0.99
    assert (ctx.eds_check_positions(eds, p, coff, ch, poff, pats) == 1).all()
    d = runner.dir
    (d / "big.eds").write_bytes(eds)
    assert runner([("W", str(d / "big.eds"), count, L, 77, str(d / "big.txt"))]) == ["ok"]
    assert (d / "big.txt").read_bytes() == text


def test_genpatterns_cli(ctx, runner, tmp_path):
    exe = os.path.join(BUILD, "edsparser-genpatterns")
    eds = "{ACGT}{A,ACA}{CGT}{T,TG}GGA{C,}TT"
    (tmp_path / "x.eds").write_text(eds)
    r = subprocess.run([exe, "-i", str(tmp_path / "x.eds"), "-o", str(tmp_path / "p.txt"), "-n", "500", "-l", "6", "--seed", "42",
                        "--witness", str(tmp_path / "w.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "Loaded EDS with 7 symbols, 10 strings" in r.stderr and "Seed: 42" in r.stderr
    assert "Successfully generated 500 patterns" in r.stderr and "[Performance] Runtime:" in r.stderr
    text = (tmp_path / "p.txt").read_bytes()
    assert text == ctx.eds_genpatterns(eds.encode(), 500, 6, 42)
    wl = (tmp_path / "w.txt").read_text().split("\n")[:-1]
    pl = text.decode().split("\n")[:-1]
    assert len(wl) == len(pl) == 500
    cmds = []
    for w, p in zip(wl, pl):
        if w == "-":
            continue
        pos, ch = w.split("\t")
        cmds.append(("C", eds, "-", pos, ch, p))
    assert len(cmds) > 0 and runner(cmds) == ["true"] * len(cmds)
    r = subprocess.run([exe, "-i", str(tmp_path / "x.eds"), "-o", str(tmp_path / "q.txt"), "-l", "40"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "Warning: Pattern length (40) is greater than total EDS size (20)" in r.stderr
    assert len((tmp_path / "q.txt").read_bytes()) == 100 * 41
    (tmp_path / "e.eds").write_text("")
    r = subprocess.run([exe, "-i", str(tmp_path / "e.eds"), "-o", str(tmp_path / "e.txt")], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: Cannot generate patterns from empty EDS" in r.stderr
