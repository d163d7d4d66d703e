"""GPU: edsx_paths_lift_sites / _lift_place / _lift / edsx_eds_lift (k_lift_group / k_lift_find / k_lift_place) field for
field against the Python restatement of the specification (tests/lift_spec.py).  Per EDS every (a, x) with x up to and
including the length of a - so that RANGE is hit - is lifted to every b, shuffled and with duplicates: the shapes of
tests/test_msa_export_gpu.py, symbol counts around the sampled LDS table, an EDS without a choice symbol, a path of
length 0, query counts around a workgroup and above one query chunk, forced table batches, the merge and VCF fixtures,
the errors, eds_locate hits placed on the paths they were cut from, the edsparser-lift tool in its four modes and the
edsparser::lift_positions shim."""
import os
import subprocess

import numpy as np
import pytest

import lift_spec as ls
import path_spec as ps
from test_msa_export_gpu import many_narrow, one_wide, zero_widths
from test_paths_cpu import BUILD, HOST, INC, LIBDIR, ROOT, merge_fixture_inputs, vcf_fixture_outputs

pytestmark = pytest.mark.gpu

TOP = 2048                                                       # sampled symbols of k_lift_find's LDS table
TILE = 16384


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    return edsparser_amd.Context(0)


def _error(fn, *a, **kw):
    import edsparser_amd
    with pytest.raises(edsparser_amd.EdsxError) as ei:
        fn(*a, **kw)
    return ei.value.code, ei.value.message


def all_queries(m, seed=1, extra=300):
    """(src, pos, dst): every (a, x <= len(a), b), shuffled, the first `extra` of them once more at the end"""
    q = [(a, x, b) for a in range(1, m.P + 1) for x in range(m.pos[a][-1] + 1) for b in range(1, m.P + 1)]
    q = np.array(q, dtype=np.uint64).reshape(-1, 3)
    q = q[np.random.default_rng(seed).permutation(len(q))]
    q = np.concatenate([q, q[:extra]])
    return q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy()


def expected(m, src, pos, dst):
    """-> (dst_pos, status, sites) of the specification as the library's arrays"""
    n = len(src)
    out, st, sites = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=ls_site())
    for k in range(n):
        p, s, site = m.lift(int(src[k]), int(pos[k]), int(dst[k]))
        out[k], st[k], sites[k] = p, s, site
    return out, st, sites


def ls_site():
    import edsparser_amd._capi as c
    return c.LIFT_SITE


def check_eds(ctx, eds, seds, queries=None):
    """lift, lift_sites and lift_place of one session against the specification -> number of queries"""
    m = ls.Model(eds, seds)
    src, pos, dst = queries if queries is not None else all_queries(m)
    want_pos, want_st, want_sites = expected(m, src, pos, dst)
    with ctx.paths_open(eds, seds) as s:
        got_pos, got_st, got_sites = s.lift(src, pos, dst, with_sites=True)
        assert np.array_equal(got_sites, want_sites)
        assert np.array_equal(got_st, want_st) and np.array_equal(got_pos, want_pos)
        t = s.timing
        assert t["bytes_written"] == len(src) * 49 and (t["copy_ms"] > 0 or len(src) == 0)
        p2, st2 = s.lift(src, pos, dst)
        assert np.array_equal(p2, want_pos) and np.array_equal(st2, want_st)
        sites, sst = s.lift_sites(src, pos)
        assert np.array_equal(sites, want_sites)
        assert np.array_equal(sst, np.where(want_sites["symbol"] == np.uint64(ls.U64_MAX), ls.RANGE, 0).astype(np.uint8))
        ok = sst == 0                                            # the two steps apart: the sites through the host
        p3, st3 = s.lift_place(sites["symbol"][ok], sites["string"][ok], sites["offset"][ok], dst[ok])
        assert np.array_equal(p3, want_pos[ok]) and np.array_equal(st3, want_st[ok])
    return len(src)


def check_place_ranges(ctx, eds, seds):
    """every (i, j, o) one past what the EDS has, on every path"""
    m = ls.Model(eds, seds)
    q = [(i, j, o, t) for t in range(1, m.P + 1) for i in range(m.n + 1) for j in range(len(m.syms[i]) + 1 if i < m.n else 1)
         for o in list(range(len(m.syms[i][j]) + 1 if i < m.n and j < len(m.syms[i]) else 1)) + [ls.U64_MAX]]
    q = np.array(q, dtype=np.uint64)
    want = [m.place(int(i), int(j), int(o), int(t)) for i, j, o, t in q]
    with ctx.paths_open(eds, seds) as s:
        p, st = s.lift_place(q[:, 0], q[:, 1], q[:, 2], q[:, 3])
    assert [(int(a), int(b)) for a, b in zip(p, st)] == want


# ---- shapes -----------------------------------------------------------------------------------------------------------
SHAPES = [("narrow 20000", lambda: many_narrow(20000))]
SHAPES += [("narrow %d" % n, (lambda n=n: many_narrow(n))) for n in (1, 2, TOP - 1, TOP, TOP + 1, 2 * TOP + 1)]
SHAPES += [("wide %d" % n, (lambda n=n: one_wide(n))) for n in (TOP - 1, TOP, TOP + 1, TILE - 1, TILE, TILE + 1)]
SHAPES += [("zero widths %d" % n, (lambda n=n: zero_widths(n))) for n in (5, TILE)]
SHAPES += [("no choice symbol", lambda: (b"{ACGT}{GG}{}{T}", b"{0,2}{0}{0,1}{0}")),
           ("empty path", lambda: (b"{A,}{C,G}{,}", b"{1}{2}{1}{3}{2}{1}")),
           ("missing", lambda: (b"{AC}{G,TTTTTTTTTTTTTTTTTTTT}{A}{C,}", b"{0}{1}{3}{0}{1}{3}")),
           ("one path", lambda: (b"{AC}{GTT}", b"{0}{1}"))]


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapes(ctx, shape):
    eds, seds = shape[1]()
    assert check_eds(ctx, eds, seds) > 0
    if len(eds) < 100:
        check_place_ranges(ctx, eds, seds)


def test_shapes_are_what_they_claim(ctx):
    with ctx.paths_open(*SHAPES[-4][1]()) as s:
        assert s.info["n_choice_symbols"] == 0 and s.info["num_paths"] == 2
    eds, seds = SHAPES[-3][1]()
    m = ls.Model(eds, seds)
    assert m.pos[2][-1] == 0                                     # path 2: empty, missing, empty
    with ctx.paths_open(eds, seds) as s:
        ln, ms_ = s.lengths()
        assert list(ln) == [m.pos[p][-1] for p in (1, 2, 3)] and ms_[1] == 1
        _, st = s.lift_sites([2, 2], [0, 1])
        assert list(st) == [ls.RANGE] * 2
        pos, st = s.lift([1, 3, 1], [0, 0, 1], [2, 2, 2])
        assert list(pos) == [0, 0, 0] and set(st) <= {ls.GAP, ls.MISSING}
    with ctx.paths_open(*many_narrow(2 * TOP + 1)) as s:
        assert s.info["n_symbols"] == 2 * TOP + 1 and s.info["num_paths"] == 3


@pytest.mark.parametrize("count", [1, 255, 256, 257, 70001])
def test_query_counts(ctx, count):
    """one path pair, so that all queries fall into one table row: below, at and above the threshold of the LDS table,
    and (70 001) more than one work item; then the same count spread over all pairs"""
    eds, seds = many_narrow(2 * TOP + 1)
    m = ls.Model(eds, seds)
    rng = np.random.default_rng(count)
    pos = rng.integers(0, m.pos[2][-1] + 2, count).astype(np.uint64)
    one = np.full(count, 2, dtype=np.uint64)
    check_eds(ctx, eds, seds, (one, pos, one + np.uint64(1)))
    check_eds(ctx, eds, seds, (rng.integers(1, 4, count).astype(np.uint64), pos, rng.integers(1, 4, count).astype(np.uint64)))


def test_forced_batches_equal_one_batch(ctx):
    """EDSX_PATHS_BUDGET stands in for the free HBM: tables of one and two paths, with src and dst in different batches,
    and 70 001 queries in two chunks."""
    eds, seds = many_narrow(2 * TOP + 1)
    m = ls.Model(eds, seds)
    rng = np.random.default_rng(3)
    n = 70001
    src, dst = rng.integers(1, 4, n).astype(np.uint64), rng.integers(1, 4, n).astype(np.uint64)
    pos = rng.integers(0, m.pos[1][-1] + 2, n).astype(np.uint64)
    want = expected(m, src, pos, dst)
    with ctx.paths_open(eds, seds) as s:
        nc = s.info["n_choice_symbols"]
        try:
            for budget in (1, 16 * nc + 64, 2 * (16 * nc + 64), 900_000):
                os.environ["EDSX_PATHS_BUDGET"] = str(budget)
                got = s.lift(src, pos, dst, with_sites=True)
                assert all(np.array_equal(g, w) for g, w in zip(got, want)), budget
                got = s.lift([1, 3], [5, 7], [3, 1])             # src != dst, one path per table
                assert all(np.array_equal(g, w) for g, w in zip(got, expected(m, [1, 3], [5, 7], [3, 1])[:2]))
        finally:
            del os.environ["EDSX_PATHS_BUDGET"]
        got = s.lift(src, pos, dst, with_sites=True)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("which", ["merge", "vcf"])
def test_fixtures(ctx, which):
    ran = queries = 0
    for eds, seds in (merge_fixture_inputs() if which == "merge" else vcf_fixture_outputs()):
        try:
            P = ps.parse(eds, seds)[2]
        except ValueError:
            continue
        if P == 0:
            continue
        queries += check_eds(ctx, eds, seds)
        ran += 1
    assert ran >= 100 and queries > 10000


def test_errors_and_one_shot(ctx):
    eds, seds = b"{AC}{G,TTT,}{A}", b"{0}{1}{2}{3}{0}"
    m = ls.Model(eds, seds)
    assert _error(ctx.eds_lift, eds, None, [1], [0], [1]) == (3, "Path spelling needs sources (.seds)")
    assert _error(ctx.eds_lift, eds, seds, [1, 9], [0, 0], [1, 1]) == (3, "Path id 9 out of range (1..3)")
    assert _error(ctx.eds_lift, eds, seds, [1, 1], [0, 0], [1, 0]) == (3, "Path id 0 out of range (1..3)")
    src, pos, dst = all_queries(m, extra=5)
    want = expected(m, src, pos, dst)
    got = ctx.eds_lift(eds, seds, src, pos, dst, with_sites=True)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    with ctx.paths_open(eds, seds) as s:
        assert _error(s.lift_sites, [4], [0]) == (3, "Path id 4 out of range (1..3)")
        assert _error(s.lift_place, [0], [0], [0], [0]) == (3, "Path id 0 out of range (1..3)")
        with pytest.raises(ValueError):
            s.lift([1, 2], [0], [1, 2])
        for a in s.lift([], [], []):                             # no query: empty arrays
            assert len(a) == 0
        sites, st = s.lift_sites([1, 1], [2 ** 64 - 1, 0])       # a query out of range does not fail the others
        assert list(st) == [ls.RANGE, 0] and tuple(sites[0]) == ls.NO_SITE and tuple(sites[1]) == m.site(1, 0)[0]
        assert s.spell(None, 0)[0] == ps.fasta(eds, seds, None, 0)[0]                # the session is as usable as before
    check_place_ranges(ctx, eds, seds)


def test_locate_hits_placed_on_their_paths(ctx):
    """200 patterns of 12 characters cut from the spelled paths of a 200 kbp EDS: the cut's own site is among the hits
    of eds_locate, and lift_place takes the hit columns as they are and puts that hit back at the cut."""
    eds, seds, _ = ctx.genrandomeds(200_000, seed=23)
    m = ls.Model(eds, seds)
    rng = np.random.default_rng(9)
    with ctx.paths_open(eds, seds) as s:
        fasta = s.spell(None, 0)[0].split(b"\n")
        seqs = {p: fasta[2 * p - 1] for p in range(1, m.P + 1)}
        cuts = [(int(p), int(rng.integers(0, len(seqs[int(p)]) - 12))) for p in rng.integers(1, m.P + 1, 200)]
        hit_off, hits, _, _, _, flags = ctx.eds_locate(eds, [seqs[p][x:x + 12] for p, x in cuts], seds, max_hits=4096)
        own, _ = s.lift_sites([p for p, _ in cuts], [x for _, x in cuts])
        which = np.repeat(np.arange(200), np.diff(hit_off).astype(np.int64))
        dst = np.array([cuts[q][0] for q in which], dtype=np.uint64)
        pos, st = s.lift_place(hits["symbol"], hits["string"], hits["offset"], dst)
        want = [m.place(int(h["symbol"]), int(h["string"]), int(h["offset"]), int(t)) for h, t in zip(hits, dst)]
        assert [(int(a), int(b)) for a, b in zip(pos, st)] == want
        checked = 0
        for q, (p, x) in enumerate(cuts):
            assert tuple(own[q]) == m.site(p, x)[0]
            if flags[q]:
                continue
            mine = [k for k in range(int(hit_off[q]), int(hit_off[q + 1]))
                    if (hits[k]["symbol"], hits[k]["string"], hits[k]["offset"]) == (own[q]["symbol"], own[q]["string"], own[q]["offset"])]
            assert mine, (p, x)
            assert all(hits[k]["common_pos"] == own[q]["common_pos"] for k in mine)       # locate's coordinate is the site's
            assert all((int(pos[k]), int(st[k])) == (x, ls.SAME) for k in mine)
            checked += 1
        assert checked >= 150


# ---- offsets above 2^32 ---------------------------------------------------------------------------------------------------
def test_path_longer_than_4gib(ctx):
    """{A x 2.2e9}, 3000 x {C,G}, {T x 2.2e9}{,AA}{GG}: both paths are longer than 2^32 characters (the text takes the host
    tokenisers) and there are more symbols than the sampled table has entries, so that table, the search, the columns, the
    common positions and the places hold values on both sides of 2^32; the answers in closed form from the lengths alone."""
    from bisect import bisect_right
    A = B = 2_200_000_000
    K, T, none = 3000, 2 ** 32, ls.U64_MAX
    eds = b"".join([b"{", b"A" * A, b"}", b"{C,G}" * K, b"{", b"T" * B, b"}{,AA}{GG}"])
    seds = b"{0}" + b"{1}{2}" * K + b"{0}{1}{2}{0}"
    lens = [[A]] + [[1, 1]] * K + [[B], [0, 2], [2]]
    n = len(lens)
    chosen = {1: [0] * n, 2: [0] + [1] * K + [0, 1, 0]}
    col, cc, at = [0], [0], {1: [0], 2: [0]}
    for i, l in enumerate(lens):
        col.append(col[-1] + max(l))
        cc.append(cc[-1] + (l[0] if len(l) == 1 else 0))
        for p in (1, 2):
            at[p].append(at[p][-1] + l[chosen[p][i]])
    assert n > TOP and at[1][-1] == A + K + B + 2 > T and at[2][-1] == A + K + B + 4

    def site(p, x):
        if x >= at[p][-1]:
            return (none,) * 5, ls.RANGE
        i = bisect_right(at[p], x) - 1
        o = x - at[p][i]
        return (i, chosen[p][i], o, col[i] + o, cc[i] + o if len(lens[i]) == 1 else none), 0

    def place(i, j, o, t):
        if i >= n or j >= len(lens[i]) or o >= lens[i][j]:
            return none, ls.RANGE
        lc = lens[i][chosen[t][i]]
        return (at[t][i] + lc, ls.GAP) if o >= lc else (at[t][i] + o, ls.SAME if chosen[t][i] == j else ls.ALIGNED)

    E = A + K + B
    xs = [0, A - 1, A, A + 1, A + K - 1, A + K, T - 1, T, T + 1, E - 1, E, E + 1, E + 2, E + 3, E + 4, none]
    q = np.array([(a, x, b) for a in (1, 2) for x in xs for b in (1, 2)] * 150, dtype=np.uint64)      # enough for the LDS table
    q = q[np.random.default_rng(2).permutation(len(q))]
    src, pos, dst = q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy()
    want_sites = [site(int(a), int(x)) for a, x in zip(src, pos)]
    want = [(none, ls.RANGE) if st else place(s[0], s[1], s[2], int(b)) for (s, st), b in zip(want_sites, dst)]
    assert (K + 1, 0, T - A - K, col[K + 1] + T - A - K, A + T - A - K) in [w[0] for w in want_sites]
    with ctx.paths_open(eds, seds) as s:
        del eds
        assert not s.info["tokenised_on_device"] and [int(x) for x in s.lengths()[0]] == [at[1][-1], at[2][-1]]
        got_pos, got_st, got_sites = s.lift(src, pos, dst, with_sites=True)
        assert [tuple(int(v) for v in x) for x in got_sites] == [w[0] for w in want_sites]
        assert [(int(a), int(b)) for a, b in zip(got_pos, got_st)] == want
        sites, st = s.lift_sites(src, pos)
        assert np.array_equal(sites, got_sites) and [int(x) for x in st] == [w[1] for w in want_sites]
        pl = [(K + 1, 0, T - A - K, 1), (K + 1, 0, T - A - K, 2), (K + 1, 0, B - 1, 2), (K + 1, 0, B, 2), (K + 3, 0, 1, 1), (K + 3, 0, 1, 2),
              (K + 2, 1, 1, 1), (K + 2, 1, 1, 2), (0, 0, A - 1, 2), (1, 0, 0, 2), (n, 0, 0, 1)]
        p3, st3 = s.lift_place(*[np.array(c, dtype=np.uint64) for c in zip(*pl)])
        assert [(int(a), int(b)) for a, b in zip(p3, st3)] == [place(*t) for t in pl]
        assert int(p3[0]) == T and int(p3[5]) == E + 3 and (int(p3[6]), int(st3[6])) == (E, ls.GAP)


# ---- the tool and the C++ shim ------------------------------------------------------------------------------------------
NAMES = ("SAME", "ALIGNED", "GAP", "MISSING", "RANGE")


def _dot(v):
    return "." if v == ls.U64_MAX else str(v)


def test_edsparser_lift_cli(tmp_path):
    subprocess.run(["make", "-s", "-C", HOST], check=True)        # (libedsx.so itself comes from build())
    exe = os.path.join(BUILD, "edsparser-lift")
    eds, seds = b"{ACGTAC}{A,ACA,}{CGTTTTT}{,T}{GG}{C,G}{TTTTTTTTTT}{}", b"{0}{1,3}{2}{4}{0}{1,2}{3,4}{0}{1,2,3}{5}{0}{0}"
    m = ls.Model(eds, seds)
    assert m.P == 5 and None in m.chosen[5] and None in m.chosen[4]
    (tmp_path / "x.eds").write_bytes(eds)
    (tmp_path / "x.seds").write_bytes(seds)
    rng = np.random.default_rng(4)
    q = [(int(a), int(x), int(b)) for a, x, b in zip(rng.integers(1, 6, 300), rng.integers(0, 30, 300), rng.integers(1, 6, 300))]

    class run:                                                   # started at once: the tools run side by side
        def __init__(self, name, lines, *args, rc=0, stdin=False):
            (tmp_path / (name + ".in")).write_text("".join(lines))
            self.rc, self.text = rc, "".join(lines) if stdin else None
            q = [] if stdin else ["-q", str(tmp_path / (name + ".in"))]      # without -q the queries come from standard input
            self.p = subprocess.Popen([exe, "-i", str(tmp_path / "x.eds")] + q + list(args), stdin=subprocess.PIPE if stdin else None,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)

        def done(self):
            self.stdout, self.stderr = self.p.communicate(self.text)
            assert self.p.returncode == self.rc, self.stderr
            assert "[Performance] Runtime:" in self.stderr
            return self

    # path pos dst, names with the prefix and bare ids mixed, a comment and an empty line
    r_lift = run("lift", ["# a comment\n", "\n"] + ["%s\t%d\t%s\n" % ("path%d" % a if k % 2 else a, x, "path%d" % b if k % 3 else b) for k, (a, x, b) in enumerate(q)])
    want = "".join("%s\t%d\t%s\t%s\t%s\n" % (("path%d" % a if k % 2 else a, x, "path%d" % b if k % 3 else b) +
                                           (lambda p, s, _: (_dot(p), NAMES[s]))(*m.lift(a, x, b))) for k, (a, x, b) in enumerate(q))
    want_lift = want
    # --to, another prefix, an output file
    r_to = run("to", ["hap%d %d\n" % (a, x) for a, x, _ in q], "--to", "hap2", "--prefix", "hap", "-s", str(tmp_path / "x.seds"), "-o", str(tmp_path / "to.tsv"))
    want = "".join("hap%d\t%d\thap2\t%s\t%s\n" % ((a, x) + (lambda p, s, _: (_dot(p), NAMES[s]))(*m.lift(a, x, 2))) for a, x, _ in q)
    want_to = want
    # --sites
    r_sites = run("sites", ["%d\t%d\n" % (a, x) for a, x, _ in q], "--sites", stdin=True)
    want_sites = "".join("%d\t%d\t%s\t%s\n" % (a, x, "\t".join(_dot(v) for v in m.site(a, x)[0]), "RANGE" if m.site(a, x)[1] else "OK") for a, x, _ in q)
    # --from-eds: every (symbol, string, offset) and one past, on every path
    trip = [(i, j, o, t) for t in range(1, 6) for i in range(m.n + 1) for j in range(len(m.syms[i]) + 1 if i < m.n else 1)
            for o in range(len(m.syms[i][j]) + 1 if i < m.n and j < len(m.syms[i]) else 1)]
    r_place = run("place", ["%d\t%d\t%d\tpath%d\n" % t for t in trip], "--from-eds")
    want_place = "".join("%d\t%d\t%d\tpath%d\t%s\t%s\n" % (t + (lambda p, s: (_dot(p), NAMES[s]))(*m.place(*t))) for t in trip)
    # --bed: further columns pass through, an interval that comes out empty is written, one past the end is RANGE
    bed = [(a, s, s + 1 + int(w), "gene %d" % k, "+") for k, ((a, s, _), w) in enumerate(zip(q[:120], rng.integers(0, 6, 120)))]
    bed += [(2, 7, 8, "inserted", "-"), (2, 7, 9, "inserted too", "-"), (1, 20, 40, "past the end", "+")]
    r_bed = run("bed", ["path%d\t%d\t%d\t%s\t%s\n" % t for t in bed], "--bed", "--to", "3")
    want, empty, gone = "", 0, 0
    for a, s, e, name, strand in bed:
        p0, st0, _ = m.lift(a, s, 3)
        p1, st1, _ = m.lift(a, e - 1, 3)
        if ls.RANGE in (st0, st1):
            want += "3\t.\t.\t%s\t%s\t%s\t%s\n" % (name, strand, NAMES[st0], NAMES[st1])
            gone += 1
        else:
            assert (p0, p1 + (1 if st1 < ls.GAP else 0), st0, st1) == m.interval(a, s, e, 3)
            want += "3\t%d\t%d\t%s\t%s\t%s\t%s\n" % (p0, p1 + (1 if st1 < ls.GAP else 0), name, strand, NAMES[st0], NAMES[st1])
            empty += p0 == p1 + (1 if st1 < ls.GAP else 0)
    r_range = run("range", ["1\t0\t6\n"], rc=1)
    r = r_lift.done()
    assert r.stdout == want_lift and "Lifting 300 positions" in r.stderr
    assert (tmp_path / "to.tsv").read_text() == want_to and r_to.done().stdout == ""
    assert r_sites.done().stdout == want_sites
    assert r_place.done().stdout == want_place
    assert r_bed.done().stdout == want and empty >= 1 and gone >= 1
    assert "Error: Path id 6 out of range (1..5)" in r_range.done().stderr
    # errors: the line number of a malformed line, a path out of range, options that do not go together
    r = run("bad", ["1\t0\t2\n", "1\tx\t2\n"], rc=1).done()
    assert 'Error: Query file line 2 is malformed: "1\tx\t2"' in r.stderr and r.stdout == ""
    r = run("bad2", ["1\t0\n"], rc=1).done()
    assert "Error: Query file line 1 is malformed" in r.stderr
    r = run("bad3", ["path1\t5\t5\n"], "--bed", "--to", "2", rc=1).done()
    assert "Error: Query file line 1 is malformed" in r.stderr
    r = run("opts", ["1\t0\n"], "--bed", rc=1).done()
    assert "Error: --bed needs --to" in r.stderr


def test_lift_positions_cpp_shim(tmp_path):
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    exe = os.path.join(BUILD, "test_lift")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", INC, os.path.join(ROOT, "tests", "cpp", "test_lift.cpp"),
                    os.path.join(BUILD, "libedsparser_lib.a"), "-L", LIBDIR, "-ledsx", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    eds, seds = b"{ACGTAC}{A,ACA,}{CGTTTTT}{,T}{GG}{C,G}{TTTTTTTTTT}{}", b"{0}{1,3}{2}{4}{0}{1,2}{3,4}{0}{1,2,3}{4}{0}{0}"
    m = ls.Model(eds, seds)
    src, pos, dst = all_queries(m, extra=3)
    q = b",".join(b"%d:%d:%d" % (a, x, b) for a, x, b in zip(src, pos, dst))
    cmds = [(b"L", eds, seds, q), (b"L", eds, seds, b"-"), (b"L", eds, seds, b"1:0:5"), (b"L", eds, b"{0}", b"1:0:1")]
    (tmp_path / "cmds.txt").write_bytes(b"".join(b"\t".join(c) + b"\n" for c in cmds))
    r = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split(b"\n")[:-1]
    want = []
    for a, x, b in zip(src, pos, dst):
        p, st, site = m.lift(int(a), int(x), int(b))
        want.append(":".join(str(v) for v in (p, st) + tuple(site)))
    assert out[0].decode() == ",".join(want)
    assert out[1] == b""
    assert out[2] == b"invalid_argument:Path id 5 out of range (1..4)"
    assert out[3] == b"runtime_error:sEDS: Source count (1) does not match EDS cardinality (12)"
