"""Python restatement of the MSA -> EDS / l-EDS specification (edsx_msa_transform / msa2eds), column-wise, written
from what msa_transforms.cpp means (:30-35 the common columns, :121-131 and :153 the l-EDS rule, :245-317 the two
kinds of symbol) and not from how it reads its stream: an alignment is a matrix of bytes here, with no file
position, no line width and no buffer.  TEST INFRASTRUCTURE: the comparator of tests/test_msa_spec_*.py, never
imported by edsparser_amd/ and independent of oracle/msa_oracle.cpp.

Domain: the inputs the library accepts, at least two rows of one non-zero length.  Anything else is a ValueError."""
import re

import numpy as np


def rows(msa):
    """-> the rows of the alignment.  A line that starts with '>' opens a row, every other non-empty line is
    appended to the current row."""
    out = []
    for line in bytes(msa).split(b"\n"):
        if not line:
            continue
        if line[:1] == b">":
            out.append([])
        elif not out:
            raise ValueError("sequence data before the first header")
        else:
            out[-1].append(line)
    out = [b"".join(r) for r in out]
    if len(out) < 2:
        raise ValueError("an alignment has at least two rows")
    if not out[0] or any(len(r) != len(out[0]) for r in out):
        raise ValueError("the rows of an alignment have one length, and it is not zero")
    return out


def common_columns(rws):
    """-> bool[L]: a column is common iff every row has the same byte there and that byte is not '-' (bytes are
    compared as they are, 'a' is not 'A')."""
    A = np.frombuffer(b"".join(rws), dtype=np.uint8).reshape(len(rws), len(rws[0]))
    return (A == A[0]).all(axis=0) & (A[0] != 0x2D)


def runs(common):
    """-> [(a, b, is_common)]: the maximal runs of common or of variant columns, in order."""
    L = len(common)
    edges = [0] + (np.flatnonzero(common[1:] != common[:-1]) + 1).tolist() + [L]
    first = bool(common[0])
    return [(edges[i], edges[i + 1], first == (i % 2 == 0)) for i in range(len(edges) - 1)]


def segments(common, l):
    """-> [(a, b, is_common)]: the columns of each symbol.  l == 0: every run.  l > 0: a common run stands alone iff
    it has at least l columns, or starts at column 0, or ends at the last column; every other common run and the
    variant runs around it are one segment."""
    L = len(common)
    out = []
    for a, b, c in runs(common):
        alone = c and (l == 0 or b - a >= l or a == 0 or b == L)
        if alone or not out or out[-1][2]:
            out.append((a, b, alone))
        else:
            out[-1] = (out[-1][0], b, False)
    return out


class Alignment:
    """The rows of an alignment with what does not depend on l: the common columns, and one of each distinct row
    with the ids of the rows that have its bytes (they spell the same strings), in order of first appearance."""

    def __init__(self, rws):
        self.rows = rws
        self.common = common_columns(rws)
        self.same = {}
        for i, r in enumerate(rws):
            self.same.setdefault(r, []).append(i + 1)
        self.id_text = [b"%d" % i for i in range(len(rws) + 1)]

    def transform(self, l=0):
        """-> (eds, seds).  A common symbol is the reference row's bytes with the source set {0}.  A variant segment
        has, per row, the bytes of the segment cut at the first NUL (:282) with the gaps removed; the distinct strings
        in order of first appearance, each with the ascending 1-based ids of its rows - also when all rows spell one
        string."""
        eds, seds, id_text = [], [], self.id_text
        for a, b, is_common in segments(self.common, l):
            if is_common:
                eds.append(b"{" + self.rows[0][a:b] + b"}")
                seds.append(b"{0}")
                continue
            strings = {}
            for r, ids in self.same.items():
                s = r[a:b]
                if 0 in s:
                    s = s[:s.index(0)]
                strings.setdefault(s.replace(b"-", b""), []).extend(ids)
            eds.append(b"{" + b",".join(strings) + b"}")
            seds.extend(b"{" + b",".join([id_text[i] for i in sorted(ids)]) + b"}" for ids in strings.values())
        return b"".join(eds), b"".join(seds)


def transform(msa, l=0):
    """-> (eds, seds) of the text of an alignment."""
    return Alignment(rows(msa)).transform(l)


# ---- checkers on a pair of output texts: they know nothing of how the texts were made ----

def _symbols(eds, seds):
    """-> [(strings, id lists in the order of the text)] per symbol."""
    syms = [g.split(b",") for g in re.findall(rb"\{([^{}]*)\}", bytes(eds))]
    sets = [list(map(int, g.split(b","))) for g in re.findall(rb"\{([^{}]*)\}", bytes(seds))]
    if len(sets) != sum(len(s) for s in syms):
        raise ValueError("source count does not match cardinality")
    out, k = [], 0
    for s in syms:
        out.append((s, sets[k:k + len(s)]))
        k += len(s)
    return out


def spell_all(eds, seds, S):
    """-> [path_spec.spell(..., p)[0] for p in 1..S], in one walk over the texts instead of one per path: per symbol
    the first string whose set holds p or 0 (test_spell_all_is_path_spec_spell holds the two together).  A path that
    no string of a symbol holds is an AssertionError."""
    out = [[] for _ in range(S)]
    everyone = list(range(1, S + 1))
    shared = []                                  # the strings of {0} symbols since the last symbol that tells paths apart
    for strings, sets in _symbols(eds, seds):
        if sets == [[0]]:
            shared.append(strings[0])
            continue
        head = b"".join(shared)
        shared = []
        if sorted(p for ids in sets for p in ids) == everyone:          # a partition: one string per path
            for s, ids in zip(strings, sets):
                piece = head + s
                for p in ids:
                    out[p - 1].append(piece)
            continue
        taken = {}
        for s, ids in zip(strings, sets):
            for p in (everyone if 0 in ids else ids):
                taken.setdefault(p, s)
        for p in everyone:
            assert p in taken, "path %d has no string in a symbol" % p
            out[p - 1].append(head + taken[p])
    tail = b"".join(shared)
    return [b"".join(x) + tail for x in out]


def closure(msa, eds, seds):
    """Every row comes back: for every row r, the sequence of path r is the row without its gaps.  Only for inputs
    without NUL bytes (a NUL ends a row's string inside a segment, so the row does not come back)."""
    closure_rows(rows(msa), eds, seds)


def closure_rows(rws, eds, seds):
    assert not any(b"\0" in r for r in rws)
    spelled = spell_all(eds, seds, len(rws))
    for r, row in enumerate(rws):
        assert spelled[r] == row.replace(b"-", b""), "row %d is not the sequence of path %d" % (r + 1, r + 1)


def partition(eds, seds, S):
    """In every symbol that is not {0}: the sets partition 1..S, each is ascending, the strings are pairwise distinct
    and the sets are ordered by their smallest id (the order of first appearance)."""
    for strings, sets in _symbols(eds, seds):
        if sets == [[0]]:
            continue
        assert len(set(strings)) == len(strings), strings
        assert all(ids == sorted(set(ids)) for ids in sets), sets
        assert sorted(i for ids in sets for i in ids) == list(range(1, S + 1)), sets
        firsts = [ids[0] for ids in sets]
        assert firsts == sorted(firsts), sets


def every_segment_has_two_strings(eds):
    """The premise under which an l-EDS made from an alignment passes the reference's is_leds(l): that check takes a
    symbol of one string for a common block, so a variant segment whose rows all spell one string (rows that differ
    in the placing of their gaps only) looks like a common block of any length, down to zero.  Common and variant
    segments alternate, so from the .eds alone: no two neighbouring symbols have one string each."""
    n = [g.count(b",") + 1 for g in re.findall(rb"\{([^{}]*)\}", bytes(eds))]
    return not any(x == 1 and y == 1 for x, y in zip(n, n[1:]))
