"""Premises of the constructed alignments of tests/msa_resident_cases.py, checked with numpy and the oracle alone (no
GPU): every case really begins and ends with the kind of segment it is named after, every emitter route has a case,
and the counts are the ones tests/test_msa_resident_gpu.py asserts too - no case is dropped silently."""
import hashlib

import numpy as np

import msa_resident_cases as mc
import oracle_lib as o


def _runs(rows):
    """-> [(variant, first column, columns)] of the alignment's runs (msa_transforms.cpp: a column is variant when a row
    differs from row 0 or row 0 has a gap)."""
    V = (rows != rows[0]).any(axis=0) | (rows[0] == ord("-"))
    cut = np.flatnonzero(np.diff(V.astype(np.int8))) + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut, [len(V)]])
    return [(bool(V[a]), int(a), int(b - a)) for a, b in zip(starts, ends)]


def _groups(eds):
    assert eds[:1] == b"{" and eds[-1:] == b"}"
    return eds[1:-1].split(b"}{")


def test_constructed_cases_begin_and_end_as_named():
    cases, impossible = mc.constructed_cases()
    assert len(cases) == mc.N_CONSTRUCTED == 376
    assert len([c for c in cases if c.l == 0 and c.kind != "huge"]) == mc.N_L0
    assert len([c for c in cases if c.kind == "huge"]) == mc.N_HUGE
    assert len([c for c in cases if c.l]) == mc.N_MIXED
    assert len({c.id for c in cases}) == len(cases)
    # what cannot exist: more strings than rows (either layout), a single column wrapped; nothing else
    assert all((S == 2 and mc.min_rows(kind) > 2) or (kind == "a1" and wrapped) for kind, S, wrapped in impossible)
    assert len(impossible) == 2 * mc.N_IMPOSSIBLE_L0 + len(mc.ROWS) + 2 * len(mc.MIXED_L) * mc.N_IMPOSSIBLE_MIXED == 30
    assert len([c for c in cases if c.lw]) == 157 and len([c for c in cases if not c.lw]) == 219
    reached, texts = set(), set()
    for c in cases:
        text, rows = c.build()
        assert rows.shape == (c.S, c.width()), c.id
        assert text.count(b">") == c.S
        # a wrapped case has more than one line per row, a one-line case the whole row on its first line
        assert c.lw is None or 0 < c.lw < rows.shape[1], c.id
        assert len(text.split(b"\n", 2)[1]) == (c.lw or rows.shape[1]), c.id
        assert text.count(b"\n") == c.S * (1 + (-(-rows.shape[1] // c.lw) if c.lw else 1)), c.id
        texts.add(hashlib.sha256(b"%d " % c.l + text).digest())
        runs = _runs(rows)
        e0, s0 = o.msa(text, 0)
        g0 = _groups(e0)
        assert len(g0) == len(runs), c.id
        # .seds: "{0}" per common segment, one id list per string of a variant segment
        assert len(_groups(s0)) == sum(len(g.split(b",")) if r[0] else 1 for r, g in zip(runs, g0)), c.id
        for (variant, strings, cols), run, grp in ((c.first, runs[0], g0[0]), (c.last, runs[-1], g0[-1])):
            assert run[0] == variant and run[2] == cols, (c.id, run)
            seg = rows[:, run[1]:run[1] + run[2]]
            if strings is None:                                  # the NUL kind: the oracle says how many strings
                assert c.kind == "nul" and (seg == 0).any(), c.id
            else:
                assert len(grp.split(b",")) == strings, (c.id, grp[:80])
            if not variant:
                assert grp == rows[0, run[1]:run[1] + run[2]].tobytes(), c.id
        k = c.kind
        if k[0] == "c":
            assert c.first[2] == c.last[2] == int(k[1:]) and len(runs) == (5 if c.l else 3)
        elif k[0] == "a":
            assert runs == [(False, 0, int(k[1:]))] and s0 == b"{0}"
        elif k == "huge":
            big = c.last if c.where == "last" else c.first
            assert big[2] > mc.HUGE_COMMON and c.S == 2 and not big[0]
            assert (c.first if c.where == "last" else c.last)[0]          # the other end is a variant site
        elif k == "gstrings":
            assert c.first[1] == c.last[1] > 64
        elif k == "gcols":
            assert c.first[2] == c.last[2] > 64
        elif k != "nul":
            n = int(k[1:])
            assert c.first[1] == c.last[1] == n
            assert {"v": 1 <= n <= 4, "w": 5 <= n <= 64}[k[0]] and c.first[2] <= 3
        # the generic kernels' share at l = 0 (k_seg_meta: more than 64 columns - 16 beyond 1024 rows; k_seg_group /
        # k_rl_count: more than 64 strings, a NUL byte)
        slow = 0
        for (variant, a, w), grp in zip(runs, g0):
            if variant and (w > (64 if c.S <= 1024 else 16) or len(grp.split(b",")) > 64 or (rows[:, a:a + w] == 0).any()):
                slow += 1
        assert slow == c.slow, (c.id, slow)
        if c.l:
            el, sl = o.msa(text, c.l)
            gl = _groups(el)
            assert len(gl) < len(g0), c.id
            if c.first[0]:
                assert gl[0] != g0[0] and gl[-1] != g0[-1], c.id         # both ends absorbed their neighbours: mixed
            else:
                assert gl[0] == g0[0] and gl[-1] == g0[-1] and len(gl) == 3, c.id       # common ends stand alone, the middle merged
        else:
            assert c.routes(), c.id
            reached |= c.routes()
    assert len(texts) == len(cases)                                  # no case repeats another's text and context length
    assert reached == mc.ALL_ROUTES, mc.ALL_ROUTES ^ reached
    sub = mc.one_per_route()
    assert len(sub) == 22
    assert set().union(*[c.routes() for c in sub]) == mc.ALL_ROUTES - {"common_huge"}


def test_input_cases_end_as_named():
    cases = mc.input_cases()
    assert len(cases) == mc.N_INPUT >= 200
    assert len({c.id for c in cases}) == len(cases)
    for name, values in (("L", mc.IN_L), ("S", mc.IN_S), ("lw", mc.IN_LW), ("ending", list(mc.ENDINGS)), ("l", [0, 5])):
        assert {getattr(c, name) for c in cases} == set(values), name
    for e in mc.ENDINGS:                                             # every ending with one-line and with wrapped rows
        assert {bool(c.lw and c.lw < c.L) for c in cases if c.ending == e} == ({True} if e == "partial" else {True, False})
    for c in cases:
        text = c.build()
        lines = text.split(b"\n")
        assert sum(ln.startswith(b">") for ln in lines) == c.S, c.id
        wrapped = bool(c.lw) and c.lw < c.L
        assert len(lines[1]) == (c.lw if wrapped else c.L), c.id
        if c.ending == "newline":
            assert text.endswith(b"\n") and not text.endswith(b"\n\n")
        elif c.ending == "blank":
            assert text.endswith(b"\n\n\n")
        else:
            assert not text.endswith(b"\n")
        if c.ending == "partial":
            assert wrapped and 0 < len(lines[-1]) == c.L % c.lw < c.lw, c.id
        eds, seds = o.msa(text, c.l)                                 # the oracle takes it as S rows of L columns
        assert len(_groups(seds)) >= len(_groups(eds)), c.id
        ids = [int(t) for t in seds.replace(b"}{", b",").strip(b"{}").split(b",")]
        if max(ids) > 0:                                             # every variant segment lists every row once
            assert max(ids) == c.S and ids.count(c.S) == ids.count(1), c.id
