"""CPU: the host code of the column-slab partition of msa2eds (edsparser_amd/csrc/msa_slabs.hpp: image geometry, slab
cuts, edge and anchor descriptors, the stitch of both context lengths, mini alignments, piece offsets) as host code under
the address and undefined-behaviour sanitizers (tests/cpp/test_msa_slabs.cpp, a program of its own).  What the numbers
should be comes from the Python restatement of the same logic (edsparser_amd/multigpu.py) and from the oracle: the kept
ranges and jobs the program reports are those of the restatement, and the oracle's slab texts cut to those ranges plus
the oracle's text of every job's mini alignment are the oracle's text of the whole alignment."""
import os
import random
import struct
import subprocess
import sys

import pytest

import oracle_lib as o
from msa_cases import random_msa
from test_multigpu_cpu import anchors_of, edges_of, rows_of, slab_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edsparser_amd import multigpu as mg  # noqa: E402

LAYOUT, EDGES, ANCHORS, MINI, OFFSETS = 1, 2, 3, 4, 5
ANCHOR_KEYS = ("n_segments", "found", "first_seg", "last_seg", "last_col", "last_eds_bytes", "last_seds_bytes", "first_end",
               "first_eds_end", "first_seds_end")


class Cases:
    """The case file: words (u64) and blobs (byte count, bytes, zeros up to a multiple of eight)"""

    def __init__(self):
        self.parts = []

    def words(self, *vals):
        self.parts.append(struct.pack("<%dQ" % len(vals), *vals))

    def blob(self, data):
        self.words(len(data))
        self.parts.append(bytes(data) + b"\0" * (-len(data) % 8))

    def mini(self, S, blocks):
        self.words(MINI, S, len(blocks))
        for data, ncols in blocks:
            self.words(ncols)
            self.blob(data)


class Results:
    def __init__(self, data):
        self.data, self.at = data, 0

    def words(self, n):
        v = struct.unpack_from("<%dQ" % n, self.data, self.at)
        self.at += 8 * n
        return list(v)

    def one(self):
        return self.words(1)[0]

    def blob(self):
        n = self.one()
        b = self.data[self.at:self.at + n]
        self.at += (n + 7) // 8 * 8
        return b

    def stitch(self, N):
        """-> (chains, max_cols, keep [(elo, ehi, slo, shi)], jobs [(owner, [(slab, col0, ncols)])]); the payload offsets of
        the parts are checked here against the parts themselves"""
        chains, max_cols = self.words(2)
        keep = [tuple(self.words(4)) for _ in range(N)]
        jobs, cols = [], [0] * N
        for _ in range(self.one()):
            owner, np_ = self.words(2)
            parts = []
            for _p in range(np_):
                slab, col0, ncols, before = self.words(4)
                assert before == cols[slab]
                cols[slab] += ncols
                parts.append((slab, col0, ncols))
            jobs.append((owner, parts))
        assert max_cols == max(cols)
        return chains, max_cols, keep, jobs

    def done(self):
        return self.at == len(self.data)


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    d = tmp_path_factory.mktemp("msa_slabs")
    exe = str(d / "test_msa_slabs")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-I", os.path.join(ROOT, "edsparser_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_msa_slabs.cpp"), "-o", exe], check=True)
    return exe, d


def run_twin(twin, name, cases):
    exe, d = twin
    cf, rf = str(d / (name + ".bin")), str(d / (name + ".out"))
    open(cf, "wb").write(b"".join(cases.parts))
    r = subprocess.run([exe, cf, rf], capture_output=True, text=True, env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert r.returncode == 0, r.stderr[-6000:]
    return Results(open(rf, "rb").read())


# ---------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------
def _column_queries(rng, L, lw, first=None):
    qs = [first] if first else []
    c0 = rng.randint(0, L - 1)
    qs += [(c0, rng.randint(c0 + 1, L)), (c0, c0 + 1), (0, L), (L - 1, L)]
    if lw and lw < L:                                            # cuts on, in front of and behind the line edges
        k = rng.randint(1, (L - 1) // lw)
        qs += [(k * lw, min(L, k * lw + lw)), (k * lw - 1, k * lw), (k * lw - 1, k * lw + 1), (0, k * lw), (k * lw, L)]
    return qs


def test_layout_and_row_columns(twin):
    """msa_layout, slabs_fit, slab_cut and row_columns on the alignments of test_shard_cli_cpu's layout test, on 200 more
    with blank lines at the end, and on files that are not cut"""
    inputs = []
    rng = random.Random(77)                                      # test_shard_cli_cpu.py::test_msa_layout_and_slab_images
    for _ in range(200):
        S, L = rng.randint(2, 6), rng.randint(2, 90)
        lw = rng.choice([10 ** 6, 1, 3, 7, 60])
        msa = random_msa(rng, S=S, L=L, lw=lw, trailing_newline=rng.random() < 0.5)
        c0 = rng.randint(0, L - 1)
        inputs.append((msa, L, lw, (c0, rng.randint(c0 + 1, L))))
    rng = random.Random(78)
    for _ in range(200):
        S, L = rng.randint(2, 6), rng.randint(1, 80)
        lw = rng.choice([None, 1, 7, 60])
        msa = random_msa(rng, S=S, L=L, lw=lw or 10 ** 6, trailing_newline=rng.random() < 0.5)
        blank = rng.randint(0, 3)
        if blank:
            msa = msa.rstrip(b"\n") + b"\n" * (1 + blank)
        inputs.append((msa, L, lw, None))
    rejects = [b"", b"ACGT\n", b">a\nACGT\n", b">a\nACGT\n>b\nAC\n",           # empty, no header, a single row, ragged rows
               b">a\nACGT\nACGT\nAC\n>b\nACG\nACGT\nAC\n>c\nACGT\nACGT\nAC\n",     # a wrapped row with a short middle line
               b">a\nACGT\n>b\nACGT\n\nxx\n"]                                      # text behind the last row
    cases, want = Cases(), []
    for msa, L, lw, first in inputs:
        lay = mg.msa_layout(msa)
        assert lay is not None and lay[3] == L
        N, l = rng.randint(1, 6), rng.choice([0, 0, 1, 3, 6])
        qs = _column_queries(rng, L, lw if lw and lw < L else 0, first)
        cases.words(LAYOUT)
        cases.blob(msa)
        cases.words(N, l, len(qs), *[c for q in qs for c in q])
        cols = [b"".join(mg.msa_slab_image(msa, lay, c0, c1).split(b"\n")[1::2]) for c0, c1 in qs]
        assert cols[0] == b"".join(r[qs[0][0]:qs[0][1]] for r in rows_of(msa))
        fit = N >= 2 and L >= 2 * N and L // N >= 4 * l
        want.append((lay, int(fit), [L * k // N for k in range(N + 1)], cols))
    for msa in rejects:
        assert mg.msa_layout(msa) is None
        cases.words(LAYOUT)
        cases.blob(msa)
        cases.words(2, 0, 1, 0, 1)
    res = run_twin(twin, "layout", cases)
    for i, ((starts, draw, lw, L), fit, cuts, cols) in enumerate(want):
        assert res.one() == 1, i
        S = res.one()
        assert S == len(starts) and res.words(S) == list(starts), i
        assert res.words(3) == [draw, lw, L], i
        assert res.one() == fit, i
        assert res.words(len(cuts)) == cuts, i
        for c in cols:
            assert res.blob() == c, i
    for _ in rejects:
        assert res.one() == 0
    assert res.done()


# ---------------------------------------------------------------------------------------------------------------
# the stitch
# ---------------------------------------------------------------------------------------------------------------
def _assemble(texts, keep, jobs, mini_text):
    """slab texts [(eds, seds)] cut to the kept ranges, each followed by the texts of the jobs its slab owns"""
    eds, seds = b"", b""
    for r, (e, s) in enumerate(texts):
        elo, ehi, slo, shi = keep[r]
        eds += e[elo:ehi]
        seds += s[slo:shi]
        for j, (owner, _parts) in enumerate(jobs):
            if owner == r:
                eds += mini_text[j][0]
                seds += mini_text[j][1]
    return eds, seds


def test_stitch_from_edges(twin):
    """l = 0 on the generator of test_multigpu_cpu.py::test_plan_on_simulated_slabs: 300 alignments in 2-6 slabs, the cuts
    anywhere"""
    rng = random.Random(4242)
    cases, todo = Cases(), []
    for it in range(300):
        msa = random_msa(rng, S=rng.randint(2, 6), L=rng.randint(6, 60), lw=10 ** 6, p_var=rng.choice([0.08, 0.3, 0.6]))
        rows = rows_of(msa)
        L, S = len(rows[0]), len(rows)
        nslab = rng.randint(2, min(6, L))
        bounds = [0] + sorted(rng.sample(range(1, L), nslab - 1)) + [L]
        texts = [o.msa(slab_image(rows, bounds[i], bounds[i + 1]), 0) for i in range(nslab)]
        edges = [edges_of(rows, bounds[i], bounds[i + 1], *texts[i]) for i in range(nslab)]
        plan = mg.plan_stitch(edges)
        keep = [mg.piece_bounds(edges[r], plan.actions[r]) for r in range(nslab)]
        jobs, minis = [], []
        for r in range(nslab):
            for ci in plan.actions[r].owns:
                ch = plan.chains[ci]
                parts = [(q,) + tuple(mg.chain_columns(ch, q, edges)) for q in range(ch.first, ch.last + 1)]
                jobs.append((r, parts))
                minis.append([(b"".join(row[bounds[q] + a:bounds[q] + a + n] for row in rows), n) for q, a, n in parts])
        cases.words(EDGES, nslab, *[getattr(e, f) for e in edges for f in mg.EDGE_FIELDS])
        for blocks in minis:
            cases.mini(S, blocks)
        todo.append((msa, S, texts, len(plan.chains), keep, jobs, minis))
    res = run_twin(twin, "edges", cases)
    with_jobs = 0
    for it, (msa, S, texts, nchains, keep, jobs, minis) in enumerate(todo):
        chains, _max_cols, got_keep, got_jobs = res.stitch(len(texts))
        assert chains == nchains and got_keep == keep and got_jobs == jobs, it
        mini_text = []
        for blocks in minis:
            image = mg.mini_alignment(blocks, S)
            assert res.blob() == image, it
            mini_text.append(o.msa(image, 0))
        assert _assemble(texts, got_keep, got_jobs, mini_text) == o.msa(msa, 0), it
        with_jobs += bool(jobs)
    assert res.done()
    assert with_jobs >= 30 and len(todo) - with_jobs >= 30       # both kinds: a variant run over a cut, and none


def test_stitch_from_anchors(twin):
    """l > 0: slab_anchors against leds_anchor_fields on the oracle's slab texts, and where every slab has its anchors the
    stitch between them; 2, 3 and 5 slabs at L * r // K"""
    cases, todo = Cases(), []
    for K in (2, 3, 5):
        rng = random.Random(7000 + K)
        for it in range(60):
            l = rng.choice([1, 2, 3, 5, 8, 16])
            S, L = rng.randint(2, 6), rng.randint(60 * K, 120 * K)
            lw = rng.choice([None, 7, 60])                       # None: random_msa draws one (one line, 3, 7 or 60)
            msa = random_msa(rng, S=S, L=L, lw=lw, p_var=rng.choice([0.01, 0.03, 0.1]))
            lay = mg.msa_layout(msa)
            fit = L >= 2 * K and L // K >= 4 * l
            cases.words(LAYOUT)
            cases.blob(msa)
            cases.words(K, l, 0)
            if not fit:
                todo.append((K, it, l, msa, lay, None))
                continue
            rows = rows_of(msa)
            bounds = [L * r // K for r in range(K + 1)]
            texts, fields, slab_rows = [], [], []
            cases.words(ANCHORS, K)
            for r in range(K):
                image = mg.msa_slab_image(msa, lay, bounds[r], bounds[r + 1])
                assert image == slab_image(rows, bounds[r], bounds[r + 1])
                e, s = o.msa(image, l)
                a = anchors_of(rows_of(image), l, e, s)
                ncols = bounds[r + 1] - bounds[r]
                cases.words(*[a[k] for k in ANCHOR_KEYS], ncols, len(e), len(s))
                texts.append((e, s))
                fields.append(mg.leds_anchor_fields(a, r, K, ncols, len(e), len(s)))
                slab_rows.append(rows_of(image))
            minis = []
            if all(f[0] for f in fields):
                for r in range(K - 1):
                    tail, head = fields[r][1], fields[r + 1][4]
                    minis.append([(b"".join(row[tail:] for row in slab_rows[r]), fields[r][7] - tail),
                                  (b"".join(row[:head] for row in slab_rows[r + 1]), head)])
                    cases.mini(S, minis[-1])
            todo.append((K, it, l, msa, lay, (S, texts, fields, minis)))
    res = run_twin(twin, "anchors", cases)
    stitched, unstitched, narrow = {2: 0, 3: 0, 5: 0}, 0, 0
    for K, it, l, msa, lay, slabs in todo:
        assert res.one() == 1
        S = res.one()
        assert res.words(S) == list(lay[0]) and res.words(3) == list(lay[1:])
        assert res.one() == (slabs is not None), (K, it)             # slabs_fit
        res.words(K + 1)
        if slabs is None:
            narrow += 1
            continue
        S, texts, fields, minis = slabs
        for r, (ok, tail_col, tail_eds, tail_seds, head_end, head_eds, head_seds, ncols) in enumerate(fields):
            assert res.words(12) == [ncols, len(texts[r][0]), len(texts[r][1]), ok, tail_col, tail_eds, tail_seds, head_end, head_eds,
                                     head_seds, 0, 0], (K, it, r)
        all_ok = all(f[0] for f in fields)
        assert res.one() == all_ok, (K, it)
        if not all_ok:
            unstitched += 1
            continue
        stitched[K] += 1
        chains, _max_cols, keep, jobs = res.stitch(K)
        assert chains == K - 1
        assert keep == [(f[5], f[2], f[6], f[3]) for f in fields], (K, it)
        assert jobs == [(r, [(r, fields[r][1], fields[r][7] - fields[r][1]), (r + 1, 0, fields[r + 1][4])]) for r in range(K - 1)], (K, it)
        mini_text = []
        for blocks in minis:
            image = mg.mini_alignment(blocks, S)
            assert res.blob() == image, (K, it)
            mini_text.append(o.msa(image, l))
        assert _assemble(texts, keep, jobs, mini_text) == o.msa(msa, l), (K, it, l)
    assert res.done()
    print("stitched", stitched, "unstitched", unstitched, "too narrow", narrow)
    assert all(n >= 25 for n in stitched.values()) and unstitched >= 10 and narrow >= 1
    assert (stitched, unstitched, narrow) == ({2: 60, 3: 47, 5: 32}, 40, 1)      # what the restatement gives for this draw order


def test_piece_offsets(twin):
    """piece_offsets against a prefix sum: the strides of the MSA stitch (2), the merge (3) and the VCF partition (5)"""
    rng = random.Random(5)
    cases, want = Cases(), []
    for stride in (2, 3, 5):
        for N in (1, 2, 3, 8):
            sizes = [rng.choice([0, 1, rng.randint(0, 2 ** 40)]) for _ in range(stride * N)]
            for r in range(N):
                cases.words(OFFSETS, stride, r, len(sizes), *sizes)
                e, s = sizes[0::stride], sizes[1::stride]
                want += [sum(e[:r]), sum(s[:r]), sum(e), sum(s)]
    res = run_twin(twin, "offsets", cases)
    assert res.words(len(want)) == want and res.done()
