"""GPU: edsx_eds_locate (csrc/locate_device.hip) against the brute-force restatement of its contract
(tests/locate_oracle.py) - all six arrays, so order, totals and flags - then closed loops through edsx_eds_genpatterns'
witnesses and edsx_eds_check_positions, the edsparser-locate CLI, and the boundary contract of the new entry point."""
import ctypes
import glob
import os
import random
import re
import subprocess

import numpy as np
import pytest

import locate_oracle as lo
import query_oracle as qo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "edsparser_amd", "host", "build")       # the tools build() leaves there
GOLDEN = os.path.join(ROOT, "tests", "golden")
U64_MAX = 2 ** 64 - 1
SEED_LENGTHS = (1, 7, 8, 9, 16, 17)                        # around the 8-byte seed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    return edsparser_amd.Context(0)


def _as_arrays(r):
    from edsparser_amd._capi import LOCATE_HIT
    return (np.array(r["hit_off"], dtype=np.uint64), np.array(r["hits"], dtype=LOCATE_HIT).reshape(-1),
            np.array(r["choice_off"], dtype=np.uint64), np.array(r["choices"], dtype=np.int32),
            np.array(r["totals"], dtype=np.uint64), np.array(r["flags"], dtype=np.uint8))


NAMES = ("hit_off", "hits", "choice_off", "choices", "totals", "flags")


def _same(ctx, eds, seds, patterns, max_hits=1024, common_only=False):
    """The device's six arrays equal the restatement's; returns the device's."""
    got = ctx.eds_locate(eds.encode(), [p.encode() for p in patterns], seds=None if seds is None else seds.encode(),
                         max_hits=max_hits, common_only=common_only)
    want = _as_arrays(lo.locate(qo.Eds(eds, seds), patterns, max_hits=max_hits, common_only=common_only))
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all(), (name, eds[:200], seds and seds[:200], g[:20], w[:20])
    return dict(zip(NAMES, got))


def _walk_patterns(rng, e, lengths, per_length):
    """Patterns spelt by random walks from random characters (some run off the end and stay shorter), plus one mutated
    and one extended copy per length."""
    starts = [(s, j, o) for s in range(e.n) for j, t in enumerate(e.sets[s]) for o in range(len(t))]
    out = []
    if not starts:
        return ["A"]
    for L in lengths:
        for _ in range(per_length):
            s, j, o = rng.choice(starts)
            text = e.sets[s][j][o:]
            for sym in range(s + 1, e.n):
                if len(text) >= L:
                    break
                text += rng.choice(e.sets[sym])
            out.append(text[:L])
        out.append(out[-1][:-1] + ("G" if out[-1][-1] != "G" else "T"))
        out.append(out[-2] + "A")
    return out


def _golden_inputs():
    for f in sorted(glob.glob(os.path.join(GOLDEN, "ref_data", "eds", "*.eds")) + glob.glob(os.path.join(GOLDEN, "ref_data", "vcf", "*.eds"))):
        sf = f[:-4] + ".seds"
        yield os.path.relpath(f, GOLDEN), open(f).read(), open(sf).read() if os.path.exists(sf) else None


def test_golden_eds_files(ctx):
    rng = random.Random(1)
    hits = 0
    for name, eds, seds in _golden_inputs():
        e = qo.Eds(eds, seds)
        r = _same(ctx, eds, seds, _walk_patterns(rng, e, (1, 3, 8, 12), 3))
        hits += len(r["hits"])
        if seds is not None:
            _same(ctx, eds, None, _walk_patterns(rng, e, (2, 9), 3))
    assert hits > 100


HAND_MADE = ["ACGT{A,C}GG", "{A,C}{G,T}", "{,A}{,}{TTT}{G,GG,GGG}", "{AC}{A,,C}{G}{T,TT,}CCA{G,A}",
             "{AC,A}CGT{,T}ACG{T,G}",                                           # begins and ends with a degenerate symbol
             "ACGTACGTAACCGGTTACGT{A,C}GGTTGGTTGCTTGGATGG{T,TG,}ACGTTGCATGCATGCAACGT{ACGTACGTAA,CC}{}{G}"]


@pytest.mark.parametrize("eds", HAND_MADE)
def test_hand_made_cases(ctx, eds):
    rng = random.Random(2)
    e = qo.Eds(eds)
    pats = _walk_patterns(rng, e, SEED_LENGTHS, 4) + ["A", "C", "G", "T", "{", ",", "AC", "GG", "TTTG", "N"]
    r = _same(ctx, eds, None, pats)
    assert len(r["hits"]) > 0
    _same(ctx, eds, None, pats, common_only=True)


def test_named_edge_cases(ctx):
    eds = "{AC}{A,,C}{G}{T,TT,}CCA{G,A}"
    #       ends at a string end   starts on a last character   runs off the end   inside one alternative (of symbol 3)
    pats = ["AC",                  "CA",                        "CCAGA",           "TT", "CCAG", "CCAA", "GCC", "ACGCCAA"]
    r = _same(ctx, eds, None, pats)
    per = np.diff(r["hit_off"].astype(np.int64))
    assert per[0] >= 1 and per[1] >= 1 and per[2] == 0 and per[3] >= 1 and per[6] == 1 and per[7] == 1
    h = r["hits"][r["hit_off"][0]]
    assert (h["symbol"], h["offset"], r["choice_off"][1] - r["choice_off"][0]) == (0, 0, 0)   # the next symbol gets no choice
    # wholly inside one alternative; a symbol of one long string with the seed lengths
    long_eds = "{ACGTTGCAACGGTTCCAGTACGT,TT}{G,C}ACGTTGCAACGGTTCCAGTACGT"
    _same(ctx, long_eds, None, ["GTTG", "ACGTTGC", "ACGTTGCA", "ACGTTGCAA", "ACGTTGCAACGGTTCC", "ACGTTGCAACGGTTCCA", "T", "TG", "TC"])


@pytest.mark.parametrize("max_hits", [3, 8, 9])
def test_hit_cap(ctx, max_hits):
    r = _same(ctx, "{A,A}{A,A}{A,A}", None, ["AAA", "AA", "A"], max_hits=max_hits)
    assert r["flags"][0] == (1 if max_hits < 8 else 0) and r["hit_off"][1] == min(8, max_hits)
    assert r["totals"][0] == (6 if max_hits == 3 else 8)


def test_choice_cap(ctx):
    r = _same(ctx, "C" + "{A,}" * 64 + "G", None, ["CG", "CAG", "G"])
    assert r["hit_off"][1] == 1 and r["flags"][0] == 0 and r["choice_off"][1] == 64
    r = _same(ctx, "C" + "{A,}" * 65 + "G", None, ["CG", "CAG", "G"])
    assert r["hit_off"][1] == 0 and r["totals"][0] == 0 and r["flags"][0] == 2


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_pattern_counts(ctx, count):
    rng = random.Random(count)
    eds, _ = lo.random_eds(rng, 40, False)
    e = qo.Eds(eds)
    pats = (_walk_patterns(rng, e, (1, 2, 3, 5, 9), 60))[:count]
    assert len(pats) == count
    r = _same(ctx, eds, None, pats)
    assert len(r["hit_off"]) == count + 1 and (count == 0 or len(r["hits"]) > 0)


def test_degenerate_inputs(ctx):
    from edsparser_amd._capi import EdsxError
    for eds in ("", "{}", "{,}{}"):
        r = _same(ctx, eds, None, ["A", "AC"])
        assert len(r["hits"]) == 0 and list(r["hit_off"]) == [0, 0, 0]
    with pytest.raises(EdsxError, match="Pattern 1 is empty"):
        ctx.eds_locate(b"ACGT", [b"A", b""])
    with pytest.raises(EdsxError, match="max_hits must be at least 1"):
        ctx.eds_locate(b"ACGT", [b"A"], max_hits=0)
    r = ctx.eds_locate(b"ACGT{A,C}GG", [b"G"])
    info = ctx.query_last_info()
    assert (info["n_symbols"], info["n_strings"], info["n_chars"], info["num_common_chars"]) == (3, 4, 8, 6)
    assert info["kernel_ms"] > 0


@pytest.mark.parametrize("paths,max_ids", [(5, 3), (70, 45)])
def test_sources(ctx, paths, max_ids):
    rng = random.Random(paths)
    found = with_sources = 0
    for k in range(6):
        eds, seds = lo.random_eds(rng, 30, True, paths=paths, max_ids=max_ids)
        e = qo.Eds(eds, seds)
        assert "{0}" in seds and max(max(s) for s in e.sources) > (64 if paths > 64 else 3)
        pats = _walk_patterns(rng, e, (1, 2, 3, 5, 8), 5)
        a = _same(ctx, eds, seds, pats)
        b = _same(ctx, eds, None, pats)
        with_sources += len(a["hits"])
        found += len(b["hits"])
    assert 0 < with_sources < found


def test_sources_exclude_cartesian_hits(ctx):
    eds, seds = "{A,C}{G}{T,A}", "{1}{2}{0}{2}{1}"
    free = _same(ctx, eds, None, ["AGT", "AGA", "CGT"])
    tied = _same(ctx, eds, seds, ["AGT", "AGA", "CGT"])
    assert list(np.diff(free["hit_off"].astype(np.int64))) == [1, 1, 1]
    assert list(np.diff(tied["hit_off"].astype(np.int64))) == [0, 1, 1]


@pytest.mark.parametrize("sources", [False, True])
def test_random_parity_3000_characters(ctx, sources):
    rng = random.Random(33)
    eds, seds = lo.random_eds(rng, 900, True)
    # (the sampler's wrap-around takes a non-empty string of symbols 0..11: give it twelve that have one)
    eds, seds = "".join("{%s}" % c for c in "ACCAACACCAAC") + eds, "{0}" * 12 + seds
    assert 2500 < sum(len(t) for s in qo.Eds(eds).sets for t in s) < 3500
    pats = [p for L in (4, 12) for p in ctx.eds_genpatterns(eds.encode(), 100, L, 5 + L).decode().split("\n")[:-1]]
    assert len(pats) == 200
    r = _same(ctx, eds, seds if sources else None, pats)
    assert len(r["hits"]) > 1000


def _spell(sets, cum_deg, hit, choices, L):
    s = int(hit["symbol"])
    text = sets[s][int(hit["string"])][int(hit["offset"]):]
    k, sym = 0, s + 1
    while len(text) < L and sym < len(sets):
        if len(sets[sym]) > 1:
            text += sets[sym][int(choices[k]) - cum_deg[sym]]
            k += 1
        else:
            text += sets[sym][0]
        sym += 1
    return text[:L], k


def test_closed_loop_2mbp(ctx):
    L, NP = 12, 1000
    eds, _, _ = ctx.genrandomeds(2_000_000, seed=7)
    text, wpos, woff, wdeg = ctx.eds_genpatterns(eds, NP, L, 99, witness=True)
    pats = text.split(b"\n")[:-1]
    assert (wpos != U64_MAX).sum() >= 0.99 * NP
    hit_off, hits, choice_off, choices, totals, flags = ctx.eds_locate(eds, pats, max_hits=4096)
    assert (flags == 0).all()                                                        # (a)
    assert (totals == np.diff(hit_off)).all() and len(hits) == hit_off[-1] and len(choice_off) == len(hits) + 1
    keys = []
    for q in range(NP):
        keys.append({(int(hits["common_pos"][h]), tuple(choices[choice_off[h]:choice_off[h + 1]]))
                     for h in range(int(hit_off[q]), int(hit_off[q + 1]))})
    for q in range(NP):                                                              # (b)
        if wpos[q] != U64_MAX:
            assert (int(wpos[q]), tuple(wdeg[woff[q]:woff[q + 1]])) in keys[q], q
    common = np.flatnonzero(hits["common_pos"] != U64_MAX)                           # (c)
    owner = np.repeat(np.arange(NP), np.diff(hit_off).astype(np.int64))
    klen = np.diff(choice_off).astype(np.int64)
    coff = np.zeros(len(common) + 1, dtype=np.uint64)
    coff[1:] = np.cumsum(klen[common])
    ch = np.concatenate([choices[choice_off[h]:choice_off[h + 1]] for h in common]) if len(common) else np.zeros(0, np.int32)
    status = ctx.eds_check_positions(eds, hits["common_pos"][common], coff, ch, np.arange(len(common) + 1, dtype=np.uint64) * L,
                                     b"".join(pats[q] for q in owner[common]))
    assert len(common) >= 0.99 * NP and (status == 1).all()
    for q in range(NP):                                                              # (d)
        ks = [(int(hits["symbol"][h]), int(hits["string"][h]), int(hits["offset"][h]), tuple(choices[choice_off[h]:choice_off[h + 1]]))
              for h in range(int(hit_off[q]), int(hit_off[q + 1]))]
        assert all(a < b for a, b in zip(ks, ks[1:])), q
    sets = [m.group(1).split(",") if m.group(1) is not None else [m.group(2)]        # (e)
            for m in re.finditer(r"\{([^}]*)\}|([^{}]+)", eds.decode())]
    sizes = np.array([len(s) for s in sets])
    cum_deg = np.concatenate([[0], np.cumsum(np.where(sizes > 1, sizes, 0))])
    inside = np.flatnonzero(hits["common_pos"] == U64_MAX)
    assert len(inside) > 0
    for h in inside:
        spelt, k = _spell(sets, cum_deg, hits[h], choices[choice_off[h]:choice_off[h + 1]], L)
        assert spelt.encode() == pats[owner[h]] and k == klen[h] and sizes[int(hits["symbol"][h])] > 1, h


def test_locate_cli_round_trip(ctx, tmp_path):
    eds, _, _ = ctx.genrandomeds(20_000, seed=3)
    (tmp_path / "x.eds").write_bytes(eds)
    r = subprocess.run([os.path.join(BUILD, "edsparser-genpatterns"), "-i", str(tmp_path / "x.eds"), "-o", str(tmp_path / "p.txt"),
                        "-n", "300", "-l", "8", "--seed", "42", "--witness", str(tmp_path / "w.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exe = os.path.join(BUILD, "edsparser-locate")
    io = ["-i", str(tmp_path / "x.eds"), "-p", str(tmp_path / "p.txt")]
    r = subprocess.run([exe] + io + ["-o", str(tmp_path / "h.tsv")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "Patterns: 300, hits: " in r.stderr and "truncated patterns: 0" in r.stderr and "[Performance] Runtime:" in r.stderr
    rows = [line.split("\t") for line in (tmp_path / "h.tsv").read_text().split("\n")[:-1]]
    assert all(len(x) == 6 for x in rows)
    seen = {(int(x[0]), x[1], x[5]) for x in rows}
    wl = (tmp_path / "w.txt").read_text().split("\n")[:-1]
    assert len(wl) == 300 and sum(w != "-" for w in wl) > 290
    for q, w in enumerate(wl):
        if w != "-":
            pos, ch = w.split("\t")
            assert (q, pos, ch) in seen, (q, w)
    pats = (tmp_path / "p.txt").read_bytes().split(b"\n")[:-1]
    hit_off = ctx.eds_locate(eds, pats)[0]
    assert [int(x[0]) for x in rows] == list(np.repeat(np.arange(300), np.diff(hit_off).astype(np.int64)))
    r = subprocess.run([exe] + io + ["-o", str(tmp_path / "c.tsv"), "--count-only"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    counts = [line.split("\t") for line in (tmp_path / "c.tsv").read_text().split("\n")[:-1]]
    assert counts == [[str(q), str(int(hit_off[q + 1] - hit_off[q])), "0"] for q in range(300)]
    r = subprocess.run([exe] + io + ["-o", str(tmp_path / "o.tsv"), "--common-only"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "o.tsv").read_text().split("\n")[:-1] == ["\t".join(x) for x in rows if x[1] != "-"]


# ---- the boundary contract of edsx_eds_locate, through raw ctypes (tests/test_capi_contract_gpu.py does the other calls)
def _raw_call(lib, handle, n, poff, pats, max_hits, null=None):
    from edsparser_amd._capi import _Buf
    bufs = [_Buf(0xdead0000, 7) for _ in range(6)]
    eds = b"{ACGT}{A,C}{GT}"
    args = [ctypes.byref(b) for b in bufs]
    if null is not None:
        args[null] = None
    rc = lib.edsx_eds_locate(handle, eds, len(eds), None, 0, n, poff.ctypes.data, pats, max_hits, 0, *args)
    return rc, [b for i, b in enumerate(bufs) if i != null]


def test_boundary_contract():
    import edsparser_amd
    lib = edsparser_amd.load_library()
    h = ctypes.c_void_p()
    assert lib.edsx_ctx_create(0, ctypes.byref(h)) == 0
    try:
        poff = np.array([0, 2, 3], dtype=np.uint64)
        rc, bufs = _raw_call(lib, None, 2, poff, b"ACG", 10)
        assert rc == 3 and all((b.data, b.size) == (None, 0) for b in bufs)
        for null in range(6):
            rc, bufs = _raw_call(lib, h, 2, poff, b"ACG", 10, null)
            assert rc == 3 and lib.edsx_last_error(h) == b"null argument"
            assert all((b.data, b.size) == (None, 0) for b in bufs)
        rc, bufs = _raw_call(lib, h, 2, np.array([0, 2, 2], dtype=np.uint64), b"AC", 10)
        assert rc == 3 and lib.edsx_last_error(h) == b"Pattern 1 is empty"
        assert all((b.data, b.size) == (None, 0) for b in bufs)
        rc, bufs = _raw_call(lib, h, 2, np.array([0, 2, 1], dtype=np.uint64), b"AC", 10)
        assert rc == 3 and lib.edsx_last_error(h) == b"pattern_off decreases at pattern 1"
        rc, bufs = _raw_call(lib, h, 2, poff, b"ACG", 0)
        assert rc == 3 and lib.edsx_last_error(h) == b"max_hits must be at least 1"
        assert all((b.data, b.size) == (None, 0) for b in bufs)
        rc, bufs = _raw_call(lib, h, 2, poff, b"ACG", 10)
        assert rc == 0 and lib.edsx_last_error(h) == b""
        assert [b.size for b in bufs] == [24, 32 * 3, 8 * 4, 0, 16, 2]     # AC at 0; G in ACGT and in GT: no choices
        for b in bufs:
            lib.edsx_buf_free(ctypes.byref(b))
            assert (b.data, b.size) == (None, 0)
    finally:
        lib.edsx_ctx_destroy(h)
