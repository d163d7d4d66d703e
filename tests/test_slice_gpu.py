"""GPU: edsx_paths_slice / edsx_eds_slice (k_slice_ends / _count / _place / _seds / _copy) byte for byte against the Python
restatement of the specification (tests/slice_spec.py): both buffers, every field of `region` and `status`.  Per tiny EDS
every (start, end) of every path and every column window in one call, shuffled and with repeats; edge symbols of 300 and
5 000 strings; a string of 10 000 characters cut at every offset class modulo 16; bitsets of one, two, three and sixteen
words; regions out of range among good ones; the byte limit and the other call errors; and, without the specification, the
alignment of a slice against the column window of the alignment of the input, tiling column regions, the one-shot call
and the edsparser-slice tool."""
import os
import subprocess

import numpy as np
import pytest

import path_spec as ps
import slice_spec as ss
from test_paths_cpu import BUILD, HOST

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    return edsparser_amd.Context(0)


def _error(fn, *a, **kw):
    import edsparser_amd
    with pytest.raises(edsparser_amd.EdsxError) as ei:
        fn(*a, **kw)
    return ei.value.code, ei.value.message


def all_regions(m, seed=1, extra=200):
    """(path, start, end): every 0 <= start <= end <= length + 1 of every path and of the columns (path 0) - so that empty
    regions and regions one past the end are among them - shuffled, the first `extra` once more at the end"""
    q = [(p, s, e) for p in range(m.P + 1) for L in [m.length(p)] for s in range(L + 2) for e in range(s, L + 2)]
    q = np.array(q, dtype=np.uint64).reshape(-1, 3)
    q = q[np.random.default_rng(seed).permutation(len(q))]
    q = np.concatenate([q, q[:extra]])
    return q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy()


def check(got, m, path, start, end):
    """the three results of a slice call against the specification -> number of regions that are not RANGE"""
    eds, seds, reg = got
    w_eds, w_seds, w_reg, w_st = m.slice([int(x) for x in path], [int(x) for x in start], [int(x) for x in end])
    assert list(reg["status"]) == w_st
    for f in ss.FIELDS:
        assert reg[f].dtype == np.uint64 and [int(x) for x in reg[f]] == w_reg[f], f
    assert bytes(seds) == w_seds
    assert bytes(eds) == w_eds
    return w_st.count(ss.OK)


def check_eds(ctx, eds, seds, regions=None):
    m = ss.Model(eds, seds)
    path, start, end = regions if regions is not None else all_regions(m)
    with ctx.paths_open(eds, seds) as s:
        got = s.slice(path, start, end)
        t = s.timing
        assert t["bytes_written"] == len(got[0]) + len(got[1]) and t["copy_ms"] > 0 and t["scan_ms"] > 0
    return check(got, m, path, start, end)


# leading and inner symbols of width 0, {} and {,}, a region inside one alternative, symbols a path skips ("" for path 3 in
# the third symbol) or misses (path 2 in {CG,C}, path 3 in {,})
TINY = [(b"{}{AC}{G,TTT,}{A}{}{,}{CG,C}{T}", b"{0}{0}{1}{2}{3}{0}{0}{1}{2}{1}{3}{0}"),
        (b"{ACGT}", b"{1}"),
        (b"{A,C}{}{GG,T,}{}", b"{1}{2,3}{0}{3}{1}{2}{0}"),
        (b"{,}{ACGTACG,AC}{,TT}{G}", b"{1}{2}{1}{2}{2}{1}{0}"),
        (b"{AAAA,CC,G}{T}{ACGTA,,TTTTTTT}", b"{1}{2}{3,4}{0}{4}{1,2}{3}")]


def random_eds(rng, n_symbols, paths):
    eds, seds = [], []
    for _ in range(n_symbols):
        k = int(rng.choice([1, 1, 2, 3]))
        strings = ["".join(rng.choice(list("ACGT"), int(rng.choice([0, 0, 1, 2, 3, 5])))) for _ in range(k)]
        eds.append("{" + ",".join(strings) + "}")
        for _ in range(k):
            ids = {0} if (k == 1 and rng.random() < 0.6) else set(int(x) for x in rng.choice(np.arange(1, paths + 1), int(rng.integers(1, 3))))
            seds.append("{" + ",".join(str(i) for i in sorted(ids)) + "}")
    return "".join(eds).encode(), "".join(seds).encode()


def test_thousands_of_regions_in_one_call(ctx):
    """A random EDS of 40 symbols: every region of every path and every column window, several thousand in one call, so
    that the tiles of the fill kernels span many workgroups"""
    eds, seds = random_eds(np.random.default_rng(11), 40, 4)
    m = ss.Model(eds, seds)
    q = all_regions(m, extra=500)
    assert len(q[0]) > 3000
    assert check_eds(ctx, eds, seds, q) > 2500


def wide_edge(k):
    """a symbol of k strings at either end of a region: the count's reduction crosses a wave, the place tiles a workgroup"""
    rng = np.random.default_rng(k)
    strings = ["".join(rng.choice(list("ACGT"), int(n))) for n in rng.integers(0, 8, k)]
    strings[1], strings[2] = "ACGTACG", "TTTTTTT"                # paths 2 and 3 reach every cut offset
    eds = ("{ACG}{" + ",".join(strings) + "}{GT,A}{" + ",".join(reversed(strings)) + "}{C}").encode()
    sets = ["{%d}" % (1 + j % 5) for j in range(k)]
    seds = ("{0}" + "".join(sets) + "{1,2}{3,4,5}" + "".join(reversed(sets)) + "{0}").encode()
    path, start, end = all_regions(ss.Model(eds, seds), extra=0)
    keep = np.random.default_rng(1).permutation(len(path))[:150]
    return eds, seds, (path[keep], start[keep], end[keep])


def long_string():
    """{15}{16}{17}{10 000,17}{17}{16}{15}: regions that begin at each of 40 consecutive offsets around the start of the long
    string and end at each of 40 around its end - every class modulo 16 on both sides, copy tiles that end inside it - and
    regions whose edges are the strings of 15, 16 and 17 characters"""
    rng = np.random.default_rng(5)
    s = lambda n: "".join(rng.choice(list("ACGT"), n))
    eds = ("{%s}{%s}{%s}{%s,%s}{%s}{%s}{%s}" % (s(15), s(16), s(17), s(10000), s(17), s(17), s(16), s(15))).encode()
    seds = b"{0}{0}{0}{1}{2}{0}{0}{0}"
    m = ss.Model(eds, seds)
    L = m.length(1)
    assert L == 10096
    q = [(1, a, e) for a in range(30, 70) for e in range(L - 70, L - 30)]
    q += [(p, a, e) for p in (0, 1, 2) for a in range(0, 50, 3) for e in (15, 16, 31, 32, 48, 49, m.length(p) - 15, m.length(p) - 16, m.length(p))]
    q += [(1, a, a + w) for a in (48, 49, 4095, 4096, 4100, 8191) for w in (1, 15, 16, 17, 33, 4096, 4097)]
    q = np.array(q, dtype=np.uint64)
    return eds, seds, (q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy())


def bitset_words(P):
    """P = 64, 65, 130: two, two and three words per set (bit 0 is the universal path); 1000: sixteen.  Ids of one to four
    digits at the digit boundaries, where they exist"""
    ids = [i for i in (1, 9, 10, 63, 64, 65, 99, 100, 127, 128, 129, 130, 999, 1000) if i <= P]
    rest = [i for i in range(1, P + 1) if i not in ids]
    sets = [ids[0::2] + [P], ids[1::2], rest if rest else [P]]
    eds = b"{ACGT}{AC,G,TTT}{GG}{,A,CC}{T}"
    seds = ("{0}%s{0}%s{0}" % ("".join("{" + ",".join(str(i) for i in sorted(set(q))) + "}" for q in sets),
                               "".join("{" + ",".join(str(i) for i in sorted(set(q))) + "}" for q in reversed(sets)))).encode()
    m = ss.Model(eds, seds)
    assert m.P == P
    regions = [(p, a, e) for p in sorted(set([0, 1, 2, 9, 10, P - 1, P])) if p <= P for a in range(0, 6) for e in range(a + 1, m.length(p) + 1)]
    q = np.array(regions, dtype=np.uint64)
    return eds, seds, (q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy())


# name, make() -> (eds, seds, regions), regions of the shape that are not RANGE at the least
SHAPES = [("tiny %d" % k, (lambda k=k: TINY[k] + (all_regions(ss.Model(*TINY[k])),)), 1) for k in range(len(TINY))]
SHAPES += [("edge symbol of %d strings" % k, (lambda k=k: wide_edge(k)), 100) for k in (300, 5000)]
SHAPES += [("string of 10 000 characters", long_string, 1600)]
SHAPES += [("P = %d" % P, (lambda P=P: bitset_words(P)), 60) for P in (64, 65, 130, 1000)]


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapes(ctx, shape):
    eds, seds, regions = shape[1]()
    assert check_eds(ctx, eds, seds, regions) >= shape[2]


def test_mixed_ok_and_range(ctx):
    eds, seds = TINY[0]
    m = ss.Model(eds, seds)
    L, W = m.length(1), m.W
    q = [(1, 0, L), (1, 0, L + 1), (1, 3, 3), (1, L - 1, L), (1, L, L + 1), (0, 0, W), (0, 0, W + 1), (0, W - 1, W), (0, 4, 4), (2, 5, 2),
         (3, 0, 2 ** 64 - 1), (2, 0, 1), (0, 2 ** 64 - 1, 0), (1, 0, L)]
    path, start, end = (np.array(c, dtype=np.uint64) for c in zip(*q))
    with ctx.paths_open(eds, seds) as s:
        got = s.slice(path, start, end)
        alone = s.slice([1], [0], [L])
    assert list(got[2]["status"]) == [0, 4, 4, 0, 4, 0, 4, 0, 4, 4, 4, 0, 4, 0]
    assert check(got, m, path, start, end) == 6
    first = bytes(got[0])[:int(got[2]["eds_len"][0])]
    assert first == bytes(alone[0]) and bytes(got[0]).endswith(first)     # the good regions are what they are alone


def test_limits_and_errors(ctx):
    eds, seds = TINY[0]
    m = ss.Model(eds, seds)
    path, start, end = all_regions(m, extra=10)
    w_eds, w_seds, _, _ = m.slice([int(x) for x in path], [int(x) for x in start], [int(x) for x in end])
    total = len(w_eds) + len(w_seds)
    with ctx.paths_open(eds, seds) as s:
        assert _error(s.slice, path, start, end, max_bytes=total - 1) == (3, "Slices have %d bytes, above the limit of %d" % (total, total - 1))
        got = s.slice(path, start, end, max_bytes=total)
        assert check(got, m, path, start, end) > 0
        os.environ["EDSX_PATHS_BUDGET"] = "1"                    # the site search with one path per table
        try:
            assert check(s.slice(path, start, end), m, path, start, end) > 0
        finally:
            del os.environ["EDSX_PATHS_BUDGET"]
        assert _error(s.slice, [1, m.P + 1], [0, 0], [1, 1]) == (3, "Path id %d out of range (1..%d)" % (m.P + 1, m.P))
        e, q, reg = s.slice([], [], [])
        assert len(e) == 0 and len(q) == 0 and all(len(v) == 0 for v in reg.values())
        with pytest.raises(ValueError):
            s.slice([1, 2], [0], [1, 2])
        assert s.spell(None, 0)[0] == ps.fasta(eds, seds, None, 0)[0]                # the session is as usable as before
    assert _error(ctx.eds_slice, eds, None, [1], [0], [1]) == (3, "Path spelling needs sources (.seds)")


def _rows(s, gap=b"-"):
    import msa_export_spec as ms
    return dict((int(name[4:]), row) for name, row in ms.rows_of(bytes(s.align(None, line_width=0)[0])))


def test_alignment_of_a_slice_is_the_column_window(ctx):
    """Without the specification: for every path the alignment rows of a session opened on a slice are the columns
    [column_first, column_end) of the rows of the input; column regions that tile [a, b) spell, path by path, what the
    region [a, b) spells; the one-shot call gives what the session gives"""
    eds, seds = random_eds(np.random.default_rng(3), 12, 4)
    m = ss.Model(eds, seds)
    path, start, end = all_regions(m, seed=4, extra=0)
    path, start, end = path[:60], start[:60], end[:60]
    with ctx.paths_open(eds, seds) as s:
        whole = _rows(s)
        e, q, reg = s.slice(path, start, end)
        W = s.align_info()["n_columns"]
        cuts = [0, 1, 2, 5, 6, W - 2, W]
        te, tq, treg = s.slice([0] * (len(cuts) - 1), cuts[:-1], cuts[1:])
        ae, aq, areg = s.slice([0], [0], [W])
    one = ctx.eds_slice(eds, seds, path, start, end)
    assert bytes(one[0]) == bytes(e) and bytes(one[1]) == bytes(q) and all(np.array_equal(one[2][f], reg[f]) for f in reg)
    e, q, te, tq = bytes(e), bytes(q), bytes(te), bytes(tq)
    checked = 0
    for r in range(len(path)):
        if reg["status"][r]:
            continue
        se = e[int(reg["eds_off"][r]):int(reg["eds_off"][r] + reg["eds_len"][r])]
        sq = q[int(reg["seds_off"][r]):int(reg["seds_off"][r] + reg["seds_len"][r])]
        with ctx.paths_open(se, sq) as t:
            rows = _rows(t)
            if path[r]:
                seq = bytes(s_spell(ctx, eds, seds, int(path[r])))
                assert bytes(t.spell([int(path[r])], 0)[0]).split(b"\n")[1] == seq[int(start[r]):int(end[r])]
        for p, row in rows.items():
            assert row == whole[p][int(reg["column_first"][r]):int(reg["column_end"][r])], (r, p)
        checked += 1
    assert checked >= 20
    # tiling
    parts = {}
    for r in range(len(cuts) - 1):
        se = te[int(treg["eds_off"][r]):int(treg["eds_off"][r] + treg["eds_len"][r])]
        sq = tq[int(treg["seds_off"][r]):int(treg["seds_off"][r] + treg["seds_len"][r])]
        syms, sets, _ = ps.parse(se, sq)
        for p in range(1, m.P + 1):
            parts[p] = parts.get(p, b"") + ps.spell(syms, sets, p)[0]
    syms, sets, _ = ps.parse(bytes(ae), bytes(aq))
    for p in range(1, m.P + 1):
        assert parts[p] == ps.spell(syms, sets, p)[0] == ps.spell(m.syms, m.sets, p)[0]


def s_spell(ctx, eds, seds, p):
    with ctx.paths_open(eds, seds) as s:
        return bytes(s.spell([p], 0)[0]).split(b"\n")[1]


def test_session_timing_is_filled_with_kernel_timing_off(ctx):
    """The two timings are separate: with edsx_set_timing off no slice kernel is listed by name, and the session's own
    timing of the call is filled all the same"""
    eds, seds = b"{AC,G}{T}{,GA}", b"{1}{2}{0}{2}{1}"
    ctx.set_timing(False)
    with ctx.paths_open(eds, seds) as s:
        got = s.slice([1], [1], [4])
        t = s.timing
    assert (bytes(got[0]), bytes(got[1])) == (b"{C,}{T}{,G}\n", b"{1}{2}{0}{2}{1}\n")
    assert not [name for name, *_ in ctx.get_timing() if name.startswith("k_slice_")]
    assert t["scan_ms"] > 0 and t["copy_ms"] > 0 and t["bytes_written"] == len(got[0]) + len(got[1])


def test_kernels_come_back_by_name(ctx):
    eds, seds = TINY[0]
    ctx.set_timing(True)
    try:
        with ctx.paths_open(eds, seds) as s:
            s.slice([1, 0], [0, 0], [3, 2])
        names = set(t[0] for t in ctx.get_timing())
    finally:
        ctx.set_timing(False)
    assert {"k_slice_ends", "k_slice_count", "scan_regions", "k_slice_place", "k_slice_seds", "k_slice_copy"} <= names


def test_edsparser_slice_cli(tmp_path):
    subprocess.run(["make", "-s", "-C", HOST], check=True)        # (libedsx.so itself comes from build())
    exe = os.path.join(BUILD, "edsparser-slice")
    eds, seds = b"{ACGTAC}{A,ACA,}{CGTTTTT}{,T}{GG}{C,G}{TTTTTTTTTT}{}", b"{0}{1,3}{2}{4}{0}{1,2}{3,4}{0}{1,2,3}{5}{0}{0}"
    m = ss.Model(eds, seds)
    (tmp_path / "x.eds").write_bytes(eds)
    (tmp_path / "x.seds").write_bytes(seds)
    (tmp_path / "r.bed").write_text("# a comment\npath2\t3\t12\tgene one\t+\n4\t0\t5\npath1\t20\t90\tpast\n")
    out = tmp_path / "out"
    r = subprocess.run([exe, "-i", str(tmp_path / "x.eds"), "-r", "1:2-9", "-r", "path3:0-4", "--columns", "5-20", "--bed", str(tmp_path / "r.bed"),
                        "--output-dir", str(out), "--table"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    regions = [(1, 2, 9, "1_2_9"), (3, 0, 4, "3_0_4"), (0, 5, 20, "cols_5_20"), (2, 3, 12, "gene one"), (4, 0, 5, "4_0_5"), (1, 20, 90, "past")]
    w_eds, w_seds, w_reg, w_st = m.slice(*[[q[k] for q in regions] for k in range(3)])
    assert w_st == [0, 0, 0, 0, 0, 4]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == 6
    for k, (p, a, e, name) in enumerate(regions):
        f = lines[k].split("\t")
        assert f[0] == name and f[-1] == ("RANGE" if w_st[k] else "OK")
        if w_st[k]:
            assert not (out / (name + ".eds")).exists() and name in r.stderr
            continue
        assert [int(x) for x in f[1:11]] == [w_reg[x][k] for x in ss.FIELDS[:8]] + [w_reg["eds_len"][k], w_reg["seds_len"][k]]
        assert (out / (name + ".eds")).read_bytes() == w_eds[w_reg["eds_off"][k]:w_reg["eds_off"][k] + w_reg["eds_len"][k]]
        assert (out / (name + ".seds")).read_bytes() == w_seds[w_reg["seds_off"][k]:w_reg["seds_off"][k] + w_reg["seds_len"][k]]
    r = subprocess.run([exe, "-i", str(tmp_path / "x.eds"), "-r", "2:3-12", "-o", str(tmp_path / "one.eds")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "one.eds").read_bytes() == (out / "gene one.eds").read_bytes()
    assert (tmp_path / "one.seds").read_bytes() == (out / "gene one.seds").read_bytes()
    r = subprocess.run([exe, "-i", str(tmp_path / "x.eds"), "-r", "6:0-1", "-o", str(tmp_path / "no.eds")], capture_output=True, text=True)
    assert r.returncode == 1 and "Error: Path id 6 out of range (1..5)" in r.stderr
    r = subprocess.run([exe, "-i", str(tmp_path / "x.eds"), "-r", "1:0-20", "--max-bytes", "10", "-o", str(tmp_path / "no.eds")], capture_output=True, text=True)
    assert r.returncode == 1 and "above the limit of 10" in r.stderr
