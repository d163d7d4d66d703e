"""GPU: edsx_eds_subset (subset_device.hip) against the Python restatement of its specification (tests/subset_spec.py),
byte for byte in both texts and in info: hand-written cases, fixtures, bitset widths either side of a word, shapes at the
kernels' own boundaries, both tokenisers; and against independent machinery: path spelling of single paths, msa2eds of a
row subset, the statistics and the LINEAR merge downstream; errors; the edsparser-subset tool."""
import os
import random
import subprocess

import pytest

import path_spec as ps
import subset_spec as ss
from test_paths_cpu import BUILD, HOST, ROOT, merge_fixture_inputs, vcf_fixture_outputs
from test_subset_cpu import HAND, random_eds

pytestmark = pytest.mark.gpu

# read from subset_device.hip / dev_util.hpp: threads per block of the filter (strings per block when one lane owns a
# string), elements per scan tile, source characters per block step of the copy kernel
FILTER_BLOCK, SCAN_TILE, COPY_TILE = 256, 2048, 4096


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    return edsparser_amd.Context(0)


def _error(fn, *a, **kw):
    import edsparser_amd
    with pytest.raises(edsparser_amd.EdsxError) as ei:
        fn(*a, **kw)
    return ei.value.code, ei.value.message


def check(ctx, eds, seds, K, keep_ids=False):
    """The library against the specification; -> the specification's result."""
    want = ss.subset(eds, seds, K, keep_ids)
    got = ctx.eds_subset(eds, seds, K, keep_ids)
    assert got[0] == want[0], (eds[:200], seds[:200], K[:20], keep_ids)
    assert got[1] == want[1], (eds[:200], seds[:200], K[:20], keep_ids)
    assert got[2] == want[2], (eds[:200], seds[:200], K[:20], keep_ids)
    return want


def _text(syms, sets):
    return (b"".join(b"{" + b",".join(s) + b"}" for s in syms),
            b"".join(b"{" + b",".join(b"%d" % p for p in sorted(s)) + b"}" for s in sets))


# ---- hand-written cases and fixtures ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_written(ctx, case):
    _, eds, seds, K, keep, want_eds, want_seds = case
    got = ctx.eds_subset(eds, seds, K, keep)
    assert got[:2] == (want_eds, want_seds)
    assert got[2] == ss.subset(eds, seds, K, keep)[2]


def test_exclude_complement(ctx):
    eds, seds = b"{AC}{G,T,A}{TT}", b"{0}{1,4}{2}{3}{0}"
    assert ctx.eds_subset(eds, seds, ss.complement([2, 3], 4))[:2] == (b"{ACGTT}\n", b"{0}\n")
    assert ctx.eds_subset(eds, seds, ss.complement([1, 4], 4))[:2] == (b"{AC}{T,A}{TT}\n", b"{0}{1}{2}{0}\n")


def test_golden_ref_data_with_sources(ctx):
    g = os.path.join(ROOT, "tests", "golden", "ref_data", "vcf")
    seen = 0
    for stem in ("small", "test_overlaps"):
        eds, seds = open(os.path.join(g, stem + ".eds"), "rb").read(), open(os.path.join(g, stem + ".seds"), "rb").read()
        P = ps.parse(eds, seds)[2]
        for K in [[p] for p in range(1, P + 1)] + [list(range(1, P + 1)), list(range(1, P + 1, 2)), list(range(P, 0, -2))]:
            for keep in (False, True):
                check(ctx, eds, seds, K, keep)
                seen += 1
    assert seen >= 10


@pytest.mark.parametrize("which", ["merge", "vcf"])
def test_fixture_sets(ctx, which):
    rng = random.Random(7)
    inputs = merge_fixture_inputs() if which == "merge" else vcf_fixture_outputs()
    done = 0
    for eds, seds in inputs:
        try:
            P = ps.parse(eds, seds)[2]
        except ValueError:
            continue
        if P == 0:
            continue
        check(ctx, eds, seds, list(range(1, P + 1)))
        check(ctx, eds, seds, rng.sample(range(1, P + 1), rng.randint(1, P)), keep_ids=done % 2 == 1)
        done += 1
    assert done >= 100


# ---- bitset widths either side of a word ---------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [63, 64, 65, 127, 128, 130, 1100])
def test_bitset_widths(ctx, P):
    rng = random.Random(P)
    eds, seds = random_eds(rng, P=P, n=40)
    assert ps.parse(eds, seds)[2] == P
    last_word = [p for p in range(1, P + 1) if p // 64 == P // 64]
    for K in ([rng.randint(1, P)], list(range(1, P + 1)), list(range(1, P + 1, 2)), last_word):
        check(ctx, eds, seds, K)
        check(ctx, eds, seds, K, keep_ids=True)


# ---- shapes at the kernels' own boundaries -----------------------------------------------------------------------------
def _m_strings(rng, m, P=5):
    """m strings in symbols of 1..4 strings"""
    syms, sets = [], []
    left = m
    while left:
        k = min(left, rng.choice([1, 1, 2, 3, 4]))
        syms.append([("".join(rng.choice("ACGT") for _ in range(rng.randint(0, 3)))).encode() for _ in range(k)])
        for _ in range(k):
            sets.append({0} if k == 1 and rng.random() < 0.5 else set(rng.sample(range(1, P + 1), rng.randint(1, 3))))
        left -= k
    sets[0] = (sets[0] - {0}) | {P}
    return _text(syms, sets)


@pytest.mark.parametrize("m", [1, 63, 64, 65, FILTER_BLOCK - 1, FILTER_BLOCK, FILTER_BLOCK + 1,
                               SCAN_TILE - 2, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1])
def test_string_counts_at_the_tiles(ctx, m):
    rng = random.Random(m)
    eds, seds = _m_strings(rng, m)
    for K in ([5], [1, 2], [1, 2, 3, 4, 5]):
        check(ctx, eds, seds, K)


@pytest.mark.parametrize("n", [SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1])
def test_symbol_counts_at_the_scan_tile(ctx, n):
    """n one-string symbols: the symbol, survivor and run scans all sit at the tile."""
    rng = random.Random(n)
    syms = [[rng.choice("ACGT").encode()] for _ in range(n)]
    sets = [{rng.choice([1, 2, 3])} for _ in range(n)]          # K = {2, 3}: removed, explicit
    check(ctx, *_text(syms, sets), [2, 3])
    check(ctx, *_text(syms, sets), [1])                          # removed or common: one long run


@pytest.mark.parametrize("keep", [0, 1, 2, 3000])
def test_one_degenerate_symbol_of_3000_strings(ctx, keep):
    rng = random.Random(keep)
    strings = [("".join(rng.choice("ACGT") for _ in range(rng.randint(0, 6)))).encode() for _ in range(3000)]
    if keep == 3000:
        sets = [{1 + (j % 2)} for j in range(3000)]
    else:
        sets = [{3} for _ in range(3000)]
        for j in rng.sample(range(3000), keep):
            sets[j] = {1 + (j % 2), 3} if keep == 2 else {1, 2}
    eds, seds = _text([[b"ACGT"], strings, [b"TT"]], [{0}] + sets + [{0}])
    check(ctx, eds, seds, [1, 2])


def test_5000_one_character_commons_with_removed_symbols_between(ctx):
    rng = random.Random(50)
    syms, sets = [], []
    for k in range(5000):
        syms.append([rng.choice("ACGT").encode()])
        sets.append({0} if k % 3 else {1, 2})
        if rng.random() < 0.1:
            syms.append([b"GG", b"T"]); sets += [{3}, {4}]       # goes with K = {1, 2}
    want = check(ctx, *_text(syms, sets), [1, 2])
    assert want[2]["symbols_out"] == 1 and want[2]["chars_out"] == 5000 and want[2]["common_runs_merged"] == 1
    check(ctx, *_text(syms, sets), [1, 2, 3])                    # nothing is removed, {1,2} no longer covers K


def test_long_strings_cross_many_copy_tiles(ctx):
    rng = random.Random(9)
    long = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
    syms = [[b"ACG"], [long(100_000)], [long(70_000), long(70_000)], [b"T", long(COPY_TILE + 5), b""], [long(33)]]
    sets = [{0}, {0}, {1, 3}, {2}, {1}, {2}, {3}, {0}]
    eds, seds = _text(syms, sets)
    for K in ([1, 2, 3], [1], [2], [3]):
        check(ctx, eds, seds, K)


@pytest.mark.parametrize("lead", list(range(1, 17)))
def test_output_offsets_at_every_residue(ctx, lead):
    rng = random.Random(lead)
    body = bytes(rng.choice(b"ACGT") for _ in range(300))
    syms = [[b"A" * lead], [body[:100], body[100:150]], [body[150:]], [b"C" * lead, b"G"]]
    sets = [{0}, {1}, {2}, {0}, {1}, {2}]
    eds, seds = _text(syms, sets)
    check(ctx, eds, seds, [1, 2])
    check(ctx, eds, seds, [2])


def test_both_tokenisers_give_identical_output(ctx):
    plain = (b"{ACGT}{A,ACA,}{CGTTTTT}{,T}{GG}{C,G}{TTTTTTTTTT}", b"{0}{1,3}{2}{4}{0}{1,2}{3,4}{0}{1,2,3}{4}{0}")
    odd = (b"{AC GT}{A,A CA,}\n{CGTTTTT}{,T}{GG}\t{C,G}{TTTTT TTTTT}\n", b"{0}{1, 3}{2}{4}\n{0}{1,2}{3,4}{0}{1,2,3}{4}{0}\n")
    for K in ([1], [1, 3], [2, 4], [1, 2, 3, 4]):
        a = ctx.eds_subset(*plain, K)
        assert ctx.leds_tokenised_on_device()
        b = ctx.eds_subset(*odd, K)
        assert not ctx.leds_tokenised_on_device()
        assert a == b == ss.subset(*plain, K)


# ---- independent machinery -----------------------------------------------------------------------------------------------
def _spell_all(ctx, eds, seds):
    with ctx.paths_open(eds, seds) as s:
        fa, miss = s.spell(None, 0)
    lines = fa.split(b"\n")[:-1]
    out, k = [], 0
    while k < len(lines):                                        # an empty sequence has no line
        assert lines[k].startswith(b">")
        if k + 1 < len(lines) and not lines[k + 1].startswith(b">"):
            out.append(lines[k + 1]); k += 2
        else:
            out.append(b""); k += 1
    return out, list(miss)


def test_single_path_identity_through_path_spelling(ctx):
    """K = {p}: every kept string covers K, so where p has one string per symbol to choose from the whole subset is one
    common run - the sequence that path spelling, which shares no code with the subset kernels, spells for p."""
    rng = random.Random(40)
    eds, seds = random_eds(rng, P=40, n=120, disjoint=True)
    with ctx.paths_open(eds, seds) as s:
        assert s.info["num_paths"] == 40
        for p in range(1, 41):
            seq = s.spell([p], 0)[0].split(b"\n")[1] if s.lengths([p])[0][0] else b""
            got = ctx.eds_subset(eds, seds, [p])
            assert got[:2] == ((b"{" + seq + b"}\n", b"{0}\n") if seq else (b"\n", b"\n")), p


def _random_alignment(rng, S, L):
    base = [rng.choice("ACGT") for _ in range(L)]
    rows = []
    for _ in range(S):
        row = list(base)
        for c in rng.sample(range(L), L // 25):
            row[c] = rng.choice("ACGT-")
        a, g = rng.randrange(L - 40), rng.randint(1, 30)
        row[a:a + g] = "-" * g
        rows.append("".join(row))
    return rows


@pytest.mark.parametrize("l", [0, 8])
def test_msa_closure(ctx, l):
    """Subsetting msa2eds(A) to rows R spells rows R of A; so does msa2eds(A[R]) (the texts may differ)."""
    rng = random.Random(2400 + l)
    rows = _random_alignment(rng, 24, 20_000)
    msa = lambda rs: "".join(">s%d\n%s\n" % (i, r) for i, r in enumerate(rs)).encode()
    R = sorted(rng.sample(range(24), 9))
    want = [rows[r].replace("-", "").encode() for r in R]
    eds, seds = ctx.msa_transform(msa(rows), l)
    sub = check(ctx, eds, seds, [r + 1 for r in R])
    got, miss = _spell_all(ctx, sub[0], sub[1])
    assert got == want and not any(miss)
    direct = ctx.msa_transform(msa([rows[r] for r in R]), l)
    got2, miss2 = _spell_all(ctx, *direct)
    assert got2 == want and not any(miss2)


def test_downstream_stats_and_linear_merge(ctx):
    eds, seds, _ = ctx.genrandomeds(200_000, seed=17)
    P = ps.parse(eds, seds)[2]
    assert P >= 4
    for K in ([1, 3], [2], list(range(1, P + 1))):
        oe, os_, info = check(ctx, eds, seds, K)
        st = ctx.eds_stats(oe, os_)
        assert (st["n_strings"], st["n_symbols"], st["n_chars"]) == (info["strings_out"], info["symbols_out"], info["chars_out"])
        # the statistics count distinct ids, 0 among them; with one kept path everything is common and only 0 is left
        ids_out = set().union(*ps.parse(oe, os_)[1])
        assert ids_out == ({0} if len(K) == 1 else set(range(0, info["paths_out"] + 1)))
        assert st["num_paths"] == len(ids_out) and st["has_sources"] == 1
        # the LINEAR merge takes the pair and keeps every path; spelled from the parsed texts, since a subset that only
        # names 0 has no path id left to ask the device for (P = 0)
        leds, lseds = ctx.leds_merge(oe, os_, 4, compact=False)
        bsyms, bsets, BP = ps.parse(oe, os_)
        asyms, asets, AP = ps.parse(leds, lseds)
        assert AP == BP == max(ids_out)
        compared = 0
        for p in range(1, len(K) + 1):
            seq, miss = ps.spell(bsyms, bsets, p)
            if miss == 0:                                        # (a path without a string somewhere has no product there)
                assert ps.spell(asyms, asets, p) == (seq, 0)
                compared += 1
        assert compared or len(K) > 1
        if BP:                                                   # ... and the device spells the same from both
            before, after = _spell_all(ctx, oe, os_), _spell_all(ctx, leds, lseds)
            assert len(before[0]) == len(after[0]) == BP
            for p in range(BP):
                if before[1][p] == 0:
                    assert after[0][p] == before[0][p] and after[1][p] == 0


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_and_sessions_usable(ctx):
    eds, seds = b"{AC}{G,T}{A}", b"{0}{1}{2,3}{0}"
    with ctx.paths_open(eds, seds) as s:
        assert _error(ctx.eds_subset, eds, None, [1]) == (3, "Path subsetting needs sources (.seds)")
        assert _error(ctx.eds_subset, eds, seds, []) == (3, "No paths selected")
        assert _error(ctx.eds_subset, eds, seds, [0]) == (3, "Path id 0 out of range (1..3)")
        assert _error(ctx.eds_subset, eds, seds, [1, 4]) == (3, "Path id 4 out of range (1..3)")
        assert _error(ctx.eds_subset, eds, seds, [2**40]) == (3, "Path id %d out of range (1..3)" % 2**40)
        assert _error(ctx.eds_subset, eds, seds, [2, 1, 2]) == (3, "Path id 2 given twice")
        assert _error(ctx.eds_subset, eds, b"{0}{1}{2,3}", [1]) == _error(ctx.paths_open, eds, b"{0}{1}{2,3}")
        assert _error(ctx.eds_subset, b"{AC}{G", seds, [1]) == _error(ctx.paths_open, b"{AC}{G", seds)
        assert ctx.eds_subset(eds, seds, [3])[:2] == (b"{ACTA}\n", b"{0}\n")
        assert ctx.eds_subset(eds, seds, [1, 2])[:2] == (b"{AC}{G,T}{A}\n", b"{0}{1}{2}{0}\n")
        assert s.spell([3, 1], 0)[0] == b">path3\nACTA\n>path1\nACGA\n"     # the session opened before still answers


def test_timing_names_the_subset_kernels(ctx):
    ctx.set_timing(True)
    try:
        ctx.eds_subset(b"{AC}{G,T}{A}", b"{0}{1}{2,3}{0}", [1, 2])
        names = {n: c for n, _, c in ctx.get_timing()}
    finally:
        ctx.set_timing(False)
    for k in ("k_sub_filter", "k_sub_classify", "k_sub_place", "k_sub_copy", "k_sub_seds"):
        assert names.get(k) == 1, names


# ---- the tool -----------------------------------------------------------------------------------------------------------
def test_edsparser_subset_cli(ctx, tmp_path):
    subprocess.run(["make", "-s", "-C", HOST], check=True)        # (libedsx.so itself comes from build())
    exe, fasta_exe = os.path.join(BUILD, "edsparser-subset"), os.path.join(BUILD, "eds2fasta")
    eds, seds, _ = ctx.genrandomeds(300_000, seed=23)
    P = ps.parse(eds, seds)[2]
    assert P == 4
    (tmp_path / "g.eds").write_bytes(eds)
    (tmp_path / "g.seds").write_bytes(seds)
    run = lambda *a: subprocess.run([exe, "-i", str(tmp_path / "g.eds")] + [str(x) for x in a], capture_output=True, text=True)
    # -p, the default output names, the info line
    r = run("-p", "4,1-2")
    assert r.returncode == 0, r.stderr
    want = ctx.eds_subset(eds, seds, [4, 1, 2])
    assert (tmp_path / "g_subset.eds").read_bytes() == want[0] and (tmp_path / "g_subset.seds").read_bytes() == want[1]
    assert "Paths: 4 -> 3, symbols: %d -> %d" % (want[2]["symbols_in"], want[2]["symbols_out"]) in r.stdout
    assert "Subsetting complete!" in r.stdout and "[Performance] Runtime:" in r.stderr
    # --paths-file, -o, --keep-ids
    (tmp_path / "ids.txt").write_text("3\n1\n")
    r = run("-s", tmp_path / "g.seds", "--paths-file", tmp_path / "ids.txt", "--keep-ids", "-o", tmp_path / "k.eds")
    assert r.returncode == 0, r.stderr
    want = ctx.eds_subset(eds, seds, [3, 1], keep_ids=True)
    assert (tmp_path / "k.eds").read_bytes() == want[0] and (tmp_path / "k.seds").read_bytes() == want[1]
    # --exclude, --names / --names-out, and eds2fasta on the result
    (tmp_path / "names.txt").write_text("alpha\nbeta\ngamma one\ndelta\n")
    r = run("-p", "2", "--exclude", "-o", tmp_path / "x.eds", "--names", tmp_path / "names.txt", "--names-out", tmp_path / "kept.txt")
    assert r.returncode == 0, r.stderr
    want = ctx.eds_subset(eds, seds, [1, 3, 4])
    assert (tmp_path / "x.eds").read_bytes() == want[0] and (tmp_path / "x.seds").read_bytes() == want[1]
    assert (tmp_path / "kept.txt").read_text() == "alpha\ngamma one\ndelta\n"
    r = subprocess.run([fasta_exe, "-i", str(tmp_path / "x.eds"), "--names", str(tmp_path / "kept.txt"), "-o", str(tmp_path / "x.fa")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([fasta_exe, "-i", str(tmp_path / "g.eds"), "--names", str(tmp_path / "names.txt"), "-p", "1,3,4",
                        "-o", str(tmp_path / "g.fa")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "x.fa").read_bytes() == (tmp_path / "g.fa").read_bytes() and (tmp_path / "g.fa").stat().st_size > 800_000
    # errors
    r = run("-p", "5")
    assert r.returncode == 1 and "Error: Path id 5 out of range (1..4)" in r.stderr and "[Performance] Runtime:" in r.stderr
    r = run("-p", "1,1")
    assert r.returncode == 1 and "Error: Path id 1 given twice" in r.stderr
    r = run("-p", "1-4", "--exclude")
    assert r.returncode == 1 and "Error: No paths selected" in r.stderr
    r = run()
    assert r.returncode == 1 and "One of --paths and --paths-file is required" in r.stderr
    r = run("-p", "1,x")
    assert r.returncode == 1 and "for option '--paths' is invalid" in r.stderr
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--paths-file" in r.stdout and "--names-out" in r.stdout
