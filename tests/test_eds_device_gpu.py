"""GPU: one Context, many features, inputs that differ in size, in the width of the path sets and in tokeniser path.  The
context keeps one DeviceEds (csrc/eds_device.hip) that the merge, the statistics, the queries and the pattern search load
in turn, inside buffers that only grow: every call must see its own text and nothing of the one before.  Expected values
come from the per-feature oracles (oracle_lib, query_oracle, locate_oracle, path_spec), never from a second context."""
import random

import numpy as np
import pytest

import locate_oracle as lo
import oracle_lib as o
import path_spec as ps
import query_oracle as qo

# A: five symbols, ids <= 3 (W = 1), plain text: tokenised on the device
A = ("{ACGT}{A,C}{GG}{T,}{ACGTACGT}", "{0}{1,2}{3}{0}{1}{2,3}{0}")
# C: inner whitespace sends it to the host tokenisers; no sources
C = "{A,C} GG{T}"
# D: a format error
D = "{A{C}}"
KIND = {True: 1, False: 0, "out_of_range": -1, "invalid_argument": -2}


def make_b():
    """About 40 symbols from a fixed seed, common and degenerate ones mixed; the first string of every symbol is on path 0
    (no merge comes out empty), the others on one to three of the paths 1..70, one of them on path 69: W = 2."""
    rng = random.Random(4242)
    sets, srcs = [], []
    for i in range(40):
        k = 1 if i % 2 == 0 and rng.random() < 0.7 else rng.choice([2, 2, 3])
        alts = ["".join(rng.choice("ACGT") for _ in range(rng.choice([1, 2, 3, 4, 6]) if j == 0 else rng.choice([0, 1, 2, 3])))
                for j in range(k)]
        sets.append(alts)
        for j in range(k):
            srcs.append({0} if j == 0 else set(rng.sample(range(1, 71), rng.randint(1, 3))))
    srcs[-1] = {0}
    next(s for s in srcs if 0 not in s).add(69)
    return ("".join("{" + ",".join(s) + "}" for s in sets), "".join("{" + ",".join(str(i) for i in sorted(s)) + "}" for s in srcs))


B = make_b()


def test_inputs_are_what_the_sequence_needs():
    """CPU side of the premises: the oracles accept A, B and C and reject D; B is larger than A in every dimension and
    needs two words per path set."""
    a, b = qo.Eds(*A), qo.Eds(*B)
    assert max(max(s) for s in a.sources) <= 3 and max(max(s) for s in b.sources) >= 64
    size = lambda e: (e.n, sum(len(s) for s in e.sets), sum(len(t) for s in e.sets for t in s))
    assert all(x > y for x, y in zip(size(b), size(a))) and b.n >= 35
    assert all(0 in b.sources[k] for k in b.first_sid)
    for eds, seds, l in ((A[0], None, 2), (A[0], A[1], 2), (B[0], B[1], 3), (C, None, 1)):
        out, _ = o.merge(eds.encode(), None if seds is None else seds.encode(), l, True)
        assert out.endswith(b"\n") and len(out) > 1
        o.eds_stats(eds.encode(), None if seds is None else seds.encode(), l)
    assert [len(s) for s in qo.Eds(C).sets] == [2, 1, 1]
    ps.parse(B[0].encode(), B[1].encode())
    with pytest.raises(o.OracleError):
        o.merge(D.encode(), None, 1, True)


def _locate_same(ctx, eds, seds, patterns):
    from edsparser_amd._capi import LOCATE_HIT
    got = ctx.eds_locate(eds.encode(), [p.encode() for p in patterns], seds=seds.encode())
    r = lo.locate(qo.Eds(eds, seds), patterns)
    want = (np.array(r["hit_off"], dtype=np.uint64), np.array(r["hits"], dtype=LOCATE_HIT).reshape(-1),
            np.array(r["choice_off"], dtype=np.uint64), np.array(r["choices"], dtype=np.int32),
            np.array(r["totals"], dtype=np.uint64), np.array(r["flags"], dtype=np.uint8))
    for name, g, w in zip(("hit_off", "hits", "choice_off", "choices", "totals", "flags"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all(), (name, eds, g[:20], w[:20])
    return len(got[1])


def _patterns(e, rng, lengths, per_length):
    """walks from random characters, so most patterns occur"""
    starts = [(s, j, k) for s in range(e.n) for j, t in enumerate(e.sets[s]) for k in range(len(t))]
    out = []
    for L in lengths:
        for _ in range(per_length):
            s, j, k = rng.choice(starts)
            text = e.sets[s][j][k:]
            for sym in range(s + 1, e.n):
                if len(text) >= L:
                    break
                text += rng.choice(e.sets[sym])
            out.append(text[:L])
    return out + ["TTTTTTTTT"]


@pytest.mark.gpu
def test_calls_on_one_context_do_not_leak_into_each_other():
    import edsparser_amd
    ctx = edsparser_amd.Context(0)
    (a_eds, a_seds), (b_eds, b_seds), c = (x.encode() for x in A), (x.encode() for x in B), C.encode()
    rng = random.Random(7)

    # 1. stats of B with sources
    assert ctx.eds_stats(b_eds, b_seds, 3) == o.eds_stats(b_eds, b_seds, 3)
    session = ctx.paths_open(b_eds, b_seds)                  # a DeviceEds of its own: spelt after everything else
    # 2. locate of A with sources
    assert _locate_same(ctx, A[0], A[1], _patterns(qo.Eds(*A), rng, (1, 2, 5, 9), 4)) > 0
    # 3. merge of B with sources, l = 3
    assert ctx.leds_merge(b_eds, b_seds, 3, True) == o.merge(b_eds, b_seds, 3, True)
    assert ctx.leds_tokenised_on_device() == 1
    # 4. position checks on A without sources: every start, right and wrong choices, patterns that match and do not
    e = qo.Eds(A[0])
    queries = [(pos, ch, pat) for pos in range(e.C + 1) for ch in ([], [0], [1, 2], [1, 3], [0, 3], [2], [9], [-1])
               for pat in ("A", "GTCG", "CGGT", "TAGGACG", "GGTACGTACGT", "")]
    pos = [q[0] for q in queries]
    coff = np.zeros(len(queries) + 1, dtype=np.uint64)
    coff[1:] = np.cumsum([len(q[1]) for q in queries])
    poff = np.zeros(len(queries) + 1, dtype=np.uint64)
    poff[1:] = np.cumsum([len(q[2]) for q in queries])
    st = ctx.eds_check_positions(a_eds, pos, coff, np.array([x for q in queries for x in q[1]], dtype=np.int32), poff,
                                 "".join(q[2] for q in queries).encode())
    want = [KIND[qo.check(e, *q)] for q in queries]
    assert list(st) == want and {1, 0, -1, -2} <= set(want)
    # 5. sampling on C (host tokenisers), with witnesses
    text, wpos, woff, wdeg = ctx.eds_genpatterns(c, 50, 3, 11, witness=True)
    wtext, wit = qo.generate(qo.Eds(C), 50, 3, 11)
    assert text == wtext
    for k, (wp, wc) in enumerate(wit):
        assert int(wpos[k]) == (2**64 - 1 if wp is None else wp)
        assert list(wdeg[int(woff[k]):int(woff[k + 1])]) == wc
    info = ctx.query_last_info()
    assert (info["n_symbols"], info["n_strings"], info["n_chars"]) == (3, 4, 5)
    # 6. merge of D: the oracle's text
    with pytest.raises(o.OracleError) as want_err:
        o.merge(D.encode(), None, 1, True)
    with pytest.raises(edsparser_amd.EdsxError) as got_err:
        ctx.leds_merge(D.encode(), None, 1, True)
    assert got_err.value.message == str(want_err.value)
    assert ctx.leds_tokenised_on_device() == 0
    # 7. stats of A without sources
    st7 = ctx.eds_stats(a_eds, None, 2)
    assert st7 == o.eds_stats(a_eds, None, 2)
    assert (st7["has_sources"], st7["num_paths"], st7["total_paths"], st7["max_paths_per_string"]) == (0, 0, 0, 0)
    # 8. locate of B with sources
    assert _locate_same(ctx, B[0], B[1], _patterns(qo.Eds(*B), rng, (1, 3, 8, 12), 6)) > 0
    # 9. CARTESIAN merge of A, l = 2
    assert ctx.leds_merge(a_eds, None, 2, True) == o.merge(a_eds, None, 2, True)
    assert ctx.leds_tokenised_on_device() == 1
    # 10. stats of C
    assert ctx.eds_stats(c, None, 1) == o.eds_stats(c, None, 1)

    with session as s:
        for lw in (0, 7):
            want, miss = ps.fasta(b_eds, b_seds, None, lw)
            got, gm = s.spell(None, lw)
            assert got == want and list(gm) == miss
        assert s.info["num_paths"] == ps.parse(b_eds, b_seds)[2] >= 64 and s.info["tokenised_on_device"] == 1
