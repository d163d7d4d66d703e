"""GPU: edsx_eds_gfa_graph / edsx_paths_gfa_walks / edsx_eds_gfa (gfa_device.hip, path_device.hip) against the Python
restatement of their specification (tests/gfa_spec.py), byte for byte and in info / steps / missing: hand-written cases,
fixtures, shapes at the kernels' own boundaries, both tokenisers; and against independent machinery: path spelling, msa2eds
of an alignment, path subsetting; the link limit; errors; the eds2gfa tool."""
import glob
import os
import random
import subprocess

import pytest

import gfa_spec as gs
import path_spec as ps
from test_gfa_cpu import open_run_eds
from test_paths_cpu import BUILD, HOST, ROOT, merge_fixture_inputs, vcf_fixture_outputs
from test_subset_cpu import random_eds

pytestmark = pytest.mark.gpu

# read from gfa_device.hip / path_device.hip / dev_util.hpp: threads per block, output bytes per block step of the two graph
# emitters (GFA_TILE) and of the walk kernel (CP_TILE), elements per scan tile
BLOCK, GFA_TILE, WALK_TILE, SCAN_TILE = 256, 16384, 16384, 2048
H = gs.HEADER


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    return edsparser_amd.Context(0)


def _error(fn, *a, **kw):
    import edsparser_amd
    with pytest.raises(edsparser_amd.EdsxError) as ei:
        fn(*a, **kw)
    return ei.value.code, ei.value.message


def _info(d):
    return {k: d[k] for k in gs.INFO_KEYS}


def check_graph(ctx, eds):
    """The graph of the library against the specification's; -> the specification's result."""
    want = gs.graph(eds)
    got = ctx.eds_gfa_graph(eds)
    assert got[0] == want[0], eds[:200]
    assert _info(got[1]) == want[1], eds[:200]
    return want


def check(ctx, eds, seds, paths=None, names=None, prefix=None):
    """Graph, walks of a session and the one-shot call against the specification; -> (graph text, lines, missing, steps)."""
    text, info = check_graph(ctx, eds)
    want = gs.walks(eds, seds, paths, names, prefix.encode() if prefix else b"path")
    with ctx.paths_open(eds, seds) as s:
        got = s.gfa_walks(paths, names, prefix)
    assert got[0] == want[0], (eds[:200], seds[:200], paths)
    assert [int(x) for x in got[1]] == want[1] and [int(x) for x in got[2]] == want[2], (eds[:200], seds[:200], paths)
    if paths is None and names is None:
        whole = ctx.eds_gfa(eds, seds, prefix=prefix)
        assert whole[0] == text + want[0] and _info(whole[1]) == info
    return (text,) + want


def _text(syms, sets=None):
    eds = b"".join(b"{" + b",".join(s) + b"}" for s in syms)
    if sets is None:
        return eds
    return eds, b"".join(b"{" + b",".join(b"%d" % p for p in sorted(s)) + b"}" for s in sets)


def S(*seqs):
    return b"".join(b"S\t%d\t%s\n" % (k + 1, s) for k, s in enumerate(seqs))


def L(*pairs):
    return b"".join(b"L\t%d\t+\t%d\t+\t0M\n" % p for p in pairs)


# ---- hand-written cases ------------------------------------------------------------------------------------------------
HAND = [
    ("open_middle", b"{A}{,C}{G}", H + S(b"A", b"C", b"G") + L((1, 2), (1, 3), (2, 3))),
    ("open_first", b"{,A}{C}", H + S(b"A", b"C") + L((1, 2))),
    ("open_last", b"{A}{C,}", H + S(b"A", b"C") + L((1, 2))),
    ("nothing", b"{}{,}", H),
    ("empty_text", b"", H),
    ("adjacent_degenerate", b"{A,C}{G,T}", H + S(b"A", b"C", b"G", b"T") + L((1, 3), (1, 4), (2, 3), (2, 4))),
    ("open_run", b"{AC}{,G}{T,}{}{CC,A}", H + S(b"AC", b"G", b"T", b"CC", b"A") +
     L((1, 2), (1, 3), (1, 4), (1, 5), (2, 3), (2, 4), (2, 5), (3, 4), (3, 5))),
    ("compact_form", b"AC{G,T}A", H + S(b"AC", b"G", b"T", b"A") + L((1, 2), (1, 3), (2, 4), (3, 4))),
]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_written_graphs(ctx, case):
    _, eds, want = case
    got = ctx.eds_gfa_graph(eds)
    assert got[0] == want
    assert (got[0], _info(got[1])) == gs.graph(eds)


def test_hand_written_walks(ctx):
    # a one-string symbol with an explicit set that path 2 misses: its walk steps over a pair that is no link
    eds, seds = b"{A}{C}{G,T}", b"{0}{1}{1}{2}"
    text, lines, miss, steps = check(ctx, eds, seds)
    assert text == H + S(b"A", b"C", b"G", b"T") + L((1, 2), (2, 3), (2, 4))
    assert lines == b"P\tpath1\t1+,2+,3+\t*\nP\tpath2\t1+,4+\t*\n" and miss == [0, 1] and steps == [3, 2]
    # a path whose chosen strings are all empty has no line; names, request order, duplicates
    eds, seds = b"{,A}{C,}", b"{1}{2}{2}{1}"
    with ctx.paths_open(eds, seds) as s:
        got = s.gfa_walks()
        assert got[0] == b"P\tpath2\t1+,2+\t*\n" and list(got[1]) == [0, 0] and list(got[2]) == [0, 2]
        got = s.gfa_walks([2, 1, 2], names=["x", "y", "z|1"])
        assert got[0] == b"P\tx\t1+,2+\t*\nP\tz|1\t1+,2+\t*\n" and list(got[2]) == [2, 0, 2]
        assert s.gfa_walks([2], prefix="hap_")[0] == b"P\thap_2\t1+,2+\t*\n"
    assert ctx.eds_gfa(eds, seds, prefix="h")[0] == H + S(b"A", b"C") + L((1, 2)) + b"P\th2\t1+,2+\t*\n"
    assert ctx.eds_gfa(eds)[0] == H + S(b"A", b"C") + L((1, 2))


# ---- fixtures ----------------------------------------------------------------------------------------------------------
def test_golden_ref_data(ctx):
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref_data", "**", "*.eds"), recursive=True))
    assert len(files) >= 20
    with_sources = 0
    for f in files:
        eds = open(f, "rb").read()
        sf = f[:-4] + ".seds"
        if os.path.exists(sf):
            check(ctx, eds, open(sf, "rb").read())
            with_sources += 1
        else:
            check_graph(ctx, eds)
    assert with_sources >= 2


@pytest.mark.parametrize("which", ["merge", "vcf"])
def test_fixture_sets(ctx, which):
    inputs = merge_fixture_inputs() if which == "merge" else vcf_fixture_outputs()
    done = 0
    for eds, seds in inputs:
        try:
            P = ps.parse(eds, seds)[2]
        except ValueError:
            continue
        if P == 0:
            continue
        check(ctx, eds, seds)
        done += 1
    assert done >= 100


def test_random_texts(ctx):
    rng = random.Random(31)
    for k in range(60):
        eds, seds = open_run_eds(rng) if k % 2 else random_eds(rng)
        check(ctx, eds, seds)


def test_both_tokenisers_give_identical_output(ctx):
    plain = (b"{ACGT}{A,ACA,}{CGTTTTT}{,T}{GG}{C,G}{TTTTTTTTTT}", b"{0}{1,3}{2}{4}{0}{1,2}{3,4}{0}{1,2,3}{4}{0}")
    odd = (b"{AC GT}{A,A CA,}\n{CGTTTTT}{,T}{GG}\t{C,G}{TTTTT TTTTT}\n", b"{0}{1, 3}{2}{4}\n{0}{1,2}{3,4}{0}{1,2,3}{4}{0}\n")
    a, b = ctx.eds_gfa_graph(plain[0]), ctx.eds_gfa_graph(odd[0])
    assert a[1]["tokenised_on_device"] and not b[1]["tokenised_on_device"]
    assert a[0] == b[0] == gs.graph(plain[0])[0] and _info(a[1]) == _info(b[1])
    wa, wb = ctx.eds_gfa(*plain), ctx.eds_gfa(*odd)
    assert wa[0] == wb[0] == gs.gfa(*plain)[0]
    with ctx.paths_open(*plain) as s, ctx.paths_open(*odd) as t:
        assert s.info["tokenised_on_device"] and not t.info["tokenised_on_device"]
        x, y = s.gfa_walks(), t.gfa_walks()
        assert x[0] == y[0] and list(x[1]) == list(y[1]) and list(x[2]) == list(y[2])


# ---- shapes at the kernels' own boundaries -----------------------------------------------------------------------------
@pytest.mark.parametrize("M", [9, 10, 99, 100, 999, 1000, 9999, 10_000, 99_999, 100_000])
def test_segment_counts_either_side_of_a_digit(ctx, M):
    """M one-character segments in M symbols, every third one with a second, empty string: the ids gain a digit at the end."""
    rng = random.Random(M)
    syms = [[rng.choice("ACGT").encode()] + ([b""] if k % 3 == 1 else []) for k in range(M)]
    want = check_graph(ctx, _text(syms))
    assert want[1]["n_segments"] == M


@pytest.mark.parametrize("n", [1, 2, BLOCK - 1, BLOCK, BLOCK + 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1])
def test_symbol_counts_at_the_tiles(ctx, n):
    rng = random.Random(n)
    eds, seds = open_run_eds(rng, P=3, n=n)
    check(ctx, eds, seds)


@pytest.mark.parametrize("m", [BLOCK - 1, BLOCK, BLOCK + 1, SCAN_TILE - 2, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1])
def test_string_counts_at_the_tiles(ctx, m):
    """m strings (m + 1 scan entries) in symbols of 1..4 strings, empty ones among them."""
    rng = random.Random(m)
    syms, left = [], m
    while left:
        k = min(left, rng.choice([1, 1, 2, 3, 4]))
        syms.append([("".join(rng.choice("ACGT") for _ in range(rng.randint(0, 3)))).encode() for _ in range(k)])
        left -= k
    check_graph(ctx, _text(syms))


@pytest.mark.parametrize("end", [GFA_TILE - 1, GFA_TILE, GFA_TILE + 1, 2 * GFA_TILE, 2 * GFA_TILE + 1])
def test_sections_end_at_the_emitter_tile(ctx, end):
    """The S lines end `end` bytes into the text (one long string, then "S\\t2\\tC\\n"), so the L lines start there."""
    long = b"A" * (end - len(H) - 5 - 6)
    want = check_graph(ctx, b"{" + long + b"}{C}{G,T}")
    assert want[1]["header_bytes"] + want[1]["segment_bytes"] == end + 12      # + the two S lines of {G,T}


def test_one_pair_of_300_by_300(ctx):
    rng = random.Random(300)
    word = lambda: "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 4))).encode()
    syms = [[b"ACGT"], [word() for _ in range(300)], [word() for _ in range(300)], [b"T"]]
    want = check_graph(ctx, _text(syms))
    assert want[1]["n_links"] == 300 + 90_000 + 300 and want[1]["link_bytes"] > 50 * GFA_TILE


@pytest.mark.parametrize("where", ["middle", "start", "end"])
def test_64_open_symbols_in_a_row(ctx, where):
    rng = random.Random(64)
    run = [[b"", rng.choice("ACGT").encode(), rng.choice("ACGT").encode() * 2] for _ in range(64)]
    syms = {"middle": [[b"AC"]] + run + [[b"GT"]], "start": run + [[b"GT"]], "end": [[b"AC"]] + run}[where]
    sets = []
    for s in syms:
        sets += [{0}] if len(s) == 1 else [{1}, {2}, {3}]
    text, lines, miss, steps = check(ctx, *_text(syms, sets))
    assert steps[0] == len(syms) - 64 and steps[1] == len(syms)
    assert gs.graph(_text(syms))[1]["n_links"] > 64 * 63 * 2


def test_one_string_of_100_000_characters(ctx):
    rng = random.Random(100)
    long = bytes(rng.choice(b"ACGT") for _ in range(100_000))
    check_graph(ctx, b"{AC}{" + long + b",G}{T}")


@pytest.mark.parametrize("lead", list(range(16)))
def test_strings_of_15_16_17_at_every_pool_residue(ctx, lead):
    rng = random.Random(lead)
    word = lambda k: bytes(rng.choice(b"ACGT") for _ in range(k))
    syms = [[word(lead)] if lead else [b""], [word(15), word(16), word(17)], [word(17), word(16), word(15)], [word(33), b"", word(16)]]
    check_graph(ctx, _text(syms))


@pytest.mark.parametrize("P", [63, 64, 65, 129])
def test_bitset_widths(ctx, P):
    rng = random.Random(P)
    eds, seds = random_eds(rng, P=P, n=40)
    assert ps.parse(eds, seds)[2] == P
    check(ctx, eds, seds)
    check(ctx, eds, seds, [P, 1, P // 2, P])


def test_three_table_batches_and_lines_of_several_stretches(ctx):
    """EDSX_PATHS_BUDGET stands in for the free HBM: 24 bytes per (path, choice symbol), two paths per table batch."""
    rng = random.Random(6000)
    syms = [[rng.choice("AC").encode(), rng.choice("GT").encode() * 2] if k % 4 else [b"ACGT"] for k in range(8000)]
    sets = []
    for s in syms:
        if len(s) == 1:
            sets.append({0})
        else:
            a = set(rng.sample(range(1, 6), rng.randint(1, 4)))
            sets += [a, set(range(1, 6)) - a]
    eds, seds = _text(syms, sets)
    want = gs.walks(eds, seds)
    assert min(len(l) for l in want[0].split(b"\n")[:-1]) > 2 * WALK_TILE
    with ctx.paths_open(eds, seds) as s:
        nc = s.info["n_choice_symbols"]
        assert nc == 6000
        one = s.gfa_walks()
        assert one[0] == want[0] and [int(x) for x in one[2]] == want[2]
        try:
            for budget in (2 * (24 * nc + 64) + 100, 1):
                os.environ["EDSX_PATHS_BUDGET"] = str(budget)
                got = s.gfa_walks()
                assert got[0] == want[0] and [int(x) for x in got[1]] == want[1] and [int(x) for x in got[2]] == want[2], budget
        finally:
            del os.environ["EDSX_PATHS_BUDGET"]
        assert s.spell([3], 0)[0] == ps.fasta(eds, seds, [3], 0)[0]          # spelling is as it was, after the walks


# ---- independent machinery -----------------------------------------------------------------------------------------------
def _spell_walks(graph_text, lines):
    segs, _, paths = gs.read(graph_text + lines)
    return {name: b"".join(segs[x] for x in walk) for name, walk in paths}, set(gs.read(graph_text)[1])


def test_walks_through_the_segments_equal_path_spelling(ctx):
    eds, seds, _ = ctx.genrandomeds(150_000, seed=29)
    graph = ctx.eds_gfa_graph(eds)[0]
    with ctx.paths_open(eds, seds) as s:
        P = s.info["num_paths"]
        lines, miss, steps = s.gfa_walks()
        fa = s.spell(None, 0)[0].split(b"\n")
    spelled, lset = _spell_walks(graph, lines)
    assert P >= 4 and len(spelled) == P
    segs, lks, paths = gs.read(graph + lines)
    for p in range(1, P + 1):
        assert fa[2 * (p - 1)] == b">path%d" % p and spelled[b"path%d" % p] == fa[2 * (p - 1) + 1]
        if miss[p - 1] == 0:
            walk = dict(paths)[b"path%d" % p]
            assert all(pair in lset for pair in zip(walk, walk[1:]))


def test_msa_rows_come_back_through_the_walks(ctx):
    rng = random.Random(77)
    base = [rng.choice("ACGT") for _ in range(3000)]
    rows = []
    for _ in range(12):
        row = list(base)
        for c in rng.sample(range(3000), 100):
            row[c] = rng.choice("ACGT-")
        a, g = rng.randrange(2900), rng.randint(1, 30)
        row[a:a + g] = "-" * g
        rows.append("".join(row))
    msa = "".join(">s%d\n%s\n" % (i, r) for i, r in enumerate(rows)).encode()
    for l in (0, 6):
        eds, seds = ctx.msa_transform(msa, l)
        text = ctx.eds_gfa(eds, seds)[0]
        segs, lks, paths = gs.read(text)
        lset = set(lks)
        assert len(paths) == 12
        for r, (name, walk) in enumerate(paths):
            assert name == b"path%d" % (r + 1) and b"".join(segs[x] for x in walk) == rows[r].replace("-", "").encode()
            assert all(pair in lset for pair in zip(walk, walk[1:]))


def test_subset_graph_has_only_segments_of_the_input_graph(ctx):
    """Paths 1 and 2 of three: every degenerate symbol keeps two strings and loses the one only path 3 takes, so nothing is
    joined and the subset's segments are segments of the input, fewer of them.  On a genrandomeds text, where common runs
    are joined, the kept paths walk the same sequences through both graphs."""
    rng = random.Random(12)
    word = lambda: bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 6)))
    syms, sets = [], []
    for k in range(400):
        syms.append([b"N" + word()]); sets.append({0})
        syms.append([word() + b"a", word() + b"b", word() + b"c"]); sets += [{1}, {2}, {3}]
    eds, seds = _text(syms, sets)
    have = gs.read(ctx.eds_gfa_graph(eds)[0])[0]
    se, ss_, _ = ctx.eds_subset(eds, seds, [1, 2])
    sub = gs.read(ctx.eds_gfa_graph(se)[0])[0]
    assert len(have) == 1600 and len(sub) == 1200 and set(sub.values()) <= set(have.values())
    assert not any(t.endswith(b"c") for t in sub.values())

    eds, seds, _ = ctx.genrandomeds(60_000, seed=5)
    se, ss_, info = ctx.eds_subset(eds, seds, [1, 3])
    assert info["common_runs_merged"] > 0
    before = _spell_walks(*_graph_and_walks(ctx, eds, seds, [1, 3]))[0]
    after = _spell_walks(*_graph_and_walks(ctx, se, ss_, [1, 2]))[0]
    assert after[b"path1"] == before[b"path1"] and after[b"path2"] == before[b"path3"] and len(after[b"path1"]) > 50_000


def _graph_and_walks(ctx, eds, seds, paths):
    with ctx.paths_open(eds, seds) as s:
        return ctx.eds_gfa_graph(eds)[0], s.gfa_walks(paths)[0]


# ---- the link limit, errors, timing ---------------------------------------------------------------------------------------
def test_max_links(ctx):
    eds = b"{A,C}{,G,T}{A,C,G}{T}"
    want = gs.graph(eds)
    nl = want[1]["n_links"]
    assert nl == 4 + 6 + 6 + 3
    assert _error(ctx.eds_gfa_graph, eds, nl - 1) == (3, "Graph has %d links, above the limit of %d" % (nl, nl - 1))
    assert _error(ctx.eds_gfa, eds, b"{1}{2}{1}{2}{2}{1}{2}{2}{0}", nl - 1) == (3, "Graph has %d links, above the limit of %d" % (nl, nl - 1))
    assert ctx.eds_gfa_graph(eds, nl)[0] == want[0]
    assert ctx.eds_gfa_graph(eds)[0] == want[0]


def test_errors_leave_the_context_and_sessions_usable(ctx):
    eds, seds = b"{AC}{G,T}{A}", b"{0}{1}{2,3}{0}"
    with ctx.paths_open(eds, seds) as s:
        assert _error(s.gfa_walks, [1], names=["a b"]) == (3, "Path name 0 is not a GFA name")
        assert _error(s.gfa_walks, [1, 2], names=["ok", "a\tb"]) == (3, "Path name 1 is not a GFA name")
        assert _error(s.gfa_walks, [1, 2], names=["ok", ""]) == (3, "Path name 1 is not a GFA name")
        assert _error(s.gfa_walks, [1], names=["a\nb"]) == (3, "Path name 0 is not a GFA name")
        assert _error(s.gfa_walks, [1], prefix="my path") == (3, "Path name 0 is not a GFA name")
        assert _error(s.gfa_walks, [0]) == (3, "Path id 0 out of range (1..3)")
        assert _error(s.gfa_walks, [1, 4]) == (3, "Path id 4 out of range (1..3)")
        assert _error(ctx.paths_open, eds, None) == (3, "Path spelling needs sources (.seds)")
        assert _error(ctx.eds_gfa, eds, b"{0}{1}{2,3}") == _error(ctx.paths_open, eds, b"{0}{1}{2,3}")
        assert _error(ctx.eds_gfa_graph, b"{AC}{G") == _error(ctx.leds_merge, b"{AC}{G", None, 1)
        assert s.gfa_walks([3, 1])[0] == b"P\tpath3\t1+,3+,4+\t*\nP\tpath1\t1+,2+,4+\t*\n"
        assert ctx.eds_gfa_graph(eds)[0] == gs.graph(eds)[0]
        assert s.spell([3], 0)[0] == b">path3\nACTA\n"


def test_timing_names_the_graph_kernels(ctx):
    ctx.set_timing(True)
    try:
        ctx.eds_gfa_graph(b"{AC}{G,T}{A}")
        names = {n: c for n, _, c in ctx.get_timing()}
    finally:
        ctx.set_timing(False)
    for k in ("scan_segments", "k_gfa_closed", "scan_closed", "k_gfa_reach", "scan_links", "k_gfa_segments", "k_gfa_links"):
        assert names.get(k) == 1, names
    with ctx.paths_open(b"{AC}{G,T}{A}", b"{0}{1}{2}{0}") as s:
        s.gfa_walks()
        t = s.timing
        assert t["bytes_written"] == len(b"P\tpath1\t1+,2+,4+\t*\n") * 2 and t["copy_ms"] > 0


# ---- the tool -----------------------------------------------------------------------------------------------------------
def test_eds2gfa_cli(ctx, tmp_path):
    subprocess.run(["make", "-s", "-C", HOST], check=True)        # (libedsx.so itself comes from build())
    exe = os.path.join(BUILD, "eds2gfa")
    eds, seds, _ = ctx.genrandomeds(400_000, seed=23)
    (tmp_path / "g.eds").write_bytes(eds)
    (tmp_path / "g.seds").write_bytes(seds)
    run = lambda *a: subprocess.run([exe] + [str(x) for x in a], capture_output=True, text=True)
    g = tmp_path / "g.eds"
    whole, info = ctx.eds_gfa(eds, seds)
    graph = ctx.eds_gfa_graph(eds)[0]
    with ctx.paths_open(eds, seds) as s:
        assert s.info["num_paths"] == 4 and 12 * s.info["n_symbols"] + 256 > (1 << 19)     # two paths do not fit one MB
        # the sources beside the input, the default output name, the banner
        r = run("-i", g)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "g.gfa").read_bytes() == whole
        assert "Segments: %d, links: %d" % (info["n_segments"], info["n_links"]) in r.stdout and "Paths written: 4 of 4 in 1 batch" in r.stdout
        assert "Export complete!" in r.stdout and "[Performance] Runtime:" in r.stderr and "Warning" not in r.stderr
        # --no-paths, -o
        r = run("-i", g, "--no-paths", "-o", tmp_path / "n.gfa")
        assert r.returncode == 0 and (tmp_path / "n.gfa").read_bytes() == graph and "Paths written" not in r.stdout
        # -p, --names, -s; --prefix and batches
        (tmp_path / "names.txt").write_text("alpha\nbeta\ngamma\ndelta\n")
        r = run("-i", g, "-s", tmp_path / "g.seds", "-p", "3,1", "--names", tmp_path / "names.txt", "-o", tmp_path / "x.gfa")
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "x.gfa").read_bytes() == graph + s.gfa_walks([3, 1], names=["gamma", "alpha"])[0]
        r = run("-i", g, "-p", "2-4", "--prefix", "hap", "--batch-mb", "1", "-o", tmp_path / "y.gfa")
        assert r.returncode == 0 and "Paths written: 3 of 3 in 3 batches" in r.stdout, r.stdout + r.stderr
        assert (tmp_path / "y.gfa").read_bytes() == graph + s.gfa_walks([2, 3, 4], prefix="hap")[0]
    # no sources beside the input: the graph alone; a path that misses a symbol: one warning line
    (tmp_path / "h.eds").write_bytes(b"{A}{C}{G,T}")
    r = run("-i", tmp_path / "h.eds")
    assert r.returncode == 0 and (tmp_path / "h.gfa").read_bytes() == gs.graph(b"{A}{C}{G,T}")[0] and "Sources" not in r.stdout
    (tmp_path / "h.seds").write_bytes(b"{0}{1}{1}{2}")
    r = run("-i", tmp_path / "h.eds")
    assert r.returncode == 0 and (tmp_path / "h.gfa").read_bytes() == gs.gfa(b"{A}{C}{G,T}", b"{0}{1}{1}{2}")[0]
    assert r.stderr.count("Warning") == 1 and "Warning: 1 path has no string in some symbol" in r.stderr
    # errors
    r = run("-i", g, "--max-links", "3")
    assert r.returncode == 1 and "Error: Graph has %d links, above the limit of 3" % info["n_links"] in r.stderr
    assert "[Performance] Runtime:" in r.stderr
    r = run("-i", g, "-p", "9")
    assert r.returncode == 1 and "Error: Path id 9 out of range (1..4)" in r.stderr
    r = run("-i", g, "--prefix", "a b")
    assert r.returncode == 1 and "Error: Path name 0 is not a GFA name" in r.stderr
    r = run("-i", g, "--no-paths", "-p", "1")
    assert r.returncode == 1 and "--no-paths does not go with" in r.stderr
    r = run("-i", tmp_path / "none.eds")
    assert r.returncode == 1 and "Input file does not exist" in r.stderr
    r = run()
    assert r.returncode == 1 and "the option '--input' is required but missing" in r.stderr
    r = run("--help")
    assert r.returncode == 0 and "--no-paths" in r.stdout and "--max-links" in r.stdout


# ---- a P line that ends at the walk kernel's stretch -------------------------------------------------------------------
def _walk_of_token_bytes(T):
    """(eds, seds) whose path 1 has exactly T token bytes: one symbol of w strings, of which path 1 takes the first, then k
    one-string symbols; every unit of w moves one more id of the k symbols past 999, which adds one byte."""
    for k in range(2700, 2800):
        for w in range(2, 900):
            if 3 + gs.dsum(w + k) - gs.dsum(w) + 2 * k == T:         # "1+," and the ids w + 1 .. w + k
                syms = [[b"A"] + [b"C"] * (w - 1)] + [[b"G"]] * k
                sets = [{1}] + [{2}] * (w - 1) + [{0}] * k
                return _text(syms, sets)
    raise AssertionError(T)


@pytest.mark.parametrize("T", [WALK_TILE - 3, WALK_TILE - 2, WALK_TILE - 1, WALK_TILE, WALK_TILE + 1])
def test_walk_line_ends_at_the_stretch(ctx, T):
    """The body of a P line is its T token bytes and "*\\n": at T = WALK_TILE - 2 it fills one stretch exactly, at
    WALK_TILE - 1 and WALK_TILE the next stretch holds only the line feed, or "*" and the line feed."""
    eds, seds = _walk_of_token_bytes(T)
    text, lines, miss, steps = check(ctx, eds, seds)
    first = lines.split(b"\n")[0] + b"\n"
    assert len(first) == len(b"P\tpath1\t") + T + 2 and miss == [0, 0]
