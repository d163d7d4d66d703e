"""Python restatement of the GFA export specification (edsx_eds_gfa_graph / edsx_paths_gfa_walks / eds2gfa), by brute
force: loops over all (i, j, u, v), path_spec for the chosen strings, str() for the numbers.  Also the closed forms of the
byte counts as the device uses them (restated here, checked against len() of the text in tests/test_gfa_cpu.py) and a
GFA reader.  TEST INFRASTRUCTURE: the comparator of tests/test_gfa_*.py, never imported by edsparser_amd/."""
import itertools
import re

import path_spec as ps

HEADER = b"H\tVN:Z:1.0\n"
INFO_KEYS = ("n_symbols", "n_strings", "n_segments", "n_empty_strings", "n_open_symbols", "n_links", "header_bytes",
             "segment_bytes", "link_bytes")


def parse_eds(eds):
    """-> symbols (lists of bytes) of an .eds text, as path_spec.parse reads it."""
    eds = re.sub(rb"\s", b"", bytes(eds))
    return [([m.group(1)] if m.group(1) is not None else m.group(2).split(b","))
            for m in re.finditer(rb"([^{}]+)|\{([^{}]*)\}", eds)]


def segment_ids(syms):
    """-> per symbol the list of (id or None) of its strings: 1-based rank among the non-empty strings."""
    out, nxt = [], 1
    for strings in syms:
        row = []
        for s in strings:
            row.append(nxt if s else None)
            nxt += 1 if s else 0
        out.append(row)
    return out


def links(syms):
    """Every (u, v), sorted: u of symbol i, v of symbol j > i, all symbols between them open (holding an empty string)."""
    ids = segment_ids(syms)
    is_open = [any(not s for s in strings) for strings in syms]
    out = []
    for i in range(len(syms)):
        for j in range(i + 1, len(syms)):
            if not all(is_open[k] for k in range(i + 1, j)):
                break                                             # (nor is any later j reached: the same k lies between)
            for u in ids[i]:
                for v in ids[j]:
                    if u is not None and v is not None:
                        out.append((u, v))
    return sorted(out)


def graph(eds):
    """-> (H + S + L text, info dict)"""
    syms = parse_eds(eds)
    ids = segment_ids(syms)
    seg = b"".join(b"S\t" + str(k).encode() + b"\t" + s + b"\n"
                   for strings, row in zip(syms, ids) for s, k in zip(strings, row) if k is not None)
    ls = links(syms)
    lk = b"".join(b"L\t" + str(u).encode() + b"\t+\t" + str(v).encode() + b"\t+\t0M\n" for u, v in ls)
    m = sum(len(s) for s in syms)
    nseg = sum(1 for row in ids for k in row if k is not None)
    info = {"n_symbols": len(syms), "n_strings": m, "n_segments": nseg, "n_empty_strings": m - nseg,
            "n_open_symbols": sum(1 for strings in syms if any(not s for s in strings)), "n_links": len(ls),
            "header_bytes": len(HEADER), "segment_bytes": len(seg), "link_bytes": len(lk)}
    return HEADER + seg + lk, info


def chosen(syms, sets, p):
    """-> (list of (symbol, string index) of the chosen strings of path p, missing), as path_spec.spell chooses."""
    out, missing, sid = [], 0, 0
    for i, strings in enumerate(syms):
        for j in range(len(strings)):
            if p in sets[sid + j] or 0 in sets[sid + j]:
                out.append((i, j))
                break
        else:
            missing += 1
        sid += len(strings)
    return out, missing


def bad_name(name):
    return name == b"" or any(c in name for c in b"\t\n ")


def walks(eds, seds, paths=None, names=None, prefix=b"path"):
    """-> (P lines, [missing], [steps]); paths None or empty: all paths 1..P.  ValueError as the library's ParamError."""
    syms, sets, P = ps.parse(eds, seds)
    ids = segment_ids(syms)
    paths = list(paths) if paths else list(range(1, P + 1))
    out, miss, steps = [], [], []
    for k, p in enumerate(paths):
        if p < 1 or p > P:
            raise ValueError("Path id %d out of range (1..%d)" % (p, P))
    for k, p in enumerate(paths):
        name = names[k] if names else prefix + str(p).encode()
        if bad_name(name):
            raise ValueError("Path name %d is not a GFA name" % k)
    for k, p in enumerate(paths):
        name = names[k] if names else prefix + str(p).encode()
        ch, m = chosen(syms, sets, p)
        walk = [ids[i][j] for i, j in ch if ids[i][j] is not None]
        if walk:
            out.append(b"P\t" + name + b"\t" + b",".join(str(x).encode() + b"+" for x in walk) + b"\t*\n")
        miss.append(m)
        steps.append(len(walk))
    return b"".join(out), miss, steps


def gfa(eds, seds=None, prefix=b"path"):
    """-> (whole text, info): the graph, then the walks of all paths when there are sources."""
    text, info = graph(eds)
    if seds is not None:
        text += walks(eds, seds, None, None, prefix)[0]
    return text, info


# ---- the closed forms (what the device computes instead of looking at every line) -------------------------------------
def digits(k):
    return len(str(k))


def dsum(x):
    """sum of digits(k) over 1 <= k <= x, as a ten-step function"""
    return sum(x - 10 ** p + 1 for p in range(20) if x >= 10 ** p)


def closed_form_counts(syms):
    """-> (segment_bytes, n_links, link_bytes) from ranks and ranges only."""
    seg_rank, r = [], 0                                           # non-empty strings before every string, + the total
    for strings in syms:
        for s in strings:
            seg_rank.append(r)
            r += 1 if s else 0
    seg_rank.append(r)
    M, N = r, sum(len(s) for strings in syms for s in strings)
    segment_bytes = 4 * M + dsum(M) + N
    ent, e = [], 0
    for strings in syms:
        ent.append(e)
        e += len(strings)
    n = len(syms)
    closed = [i for i in range(n) if seg_rank[ent[i] + len(syms[i])] - seg_rank[ent[i]] == len(syms[i])]
    n_links = link_bytes = 0
    for i in range(n):
        later = [c for c in closed if c > i]
        R = later[0] if later else n - 1
        a, b = seg_rank[ent[i]] + 1, seg_rank[ent[i] + len(syms[i])] + 1
        c, d = b, seg_rank[ent[R] + len(syms[R])] + 1
        n_links += (b - a) * (d - c)
        if b > a and d > c:
            link_bytes += (d - c) * (dsum(b - 1) - dsum(a - 1)) + (b - a) * (dsum(d - 1) - dsum(c - 1)) + 11 * (b - a) * (d - c)
    return segment_bytes, n_links, link_bytes


# ---- a GFA reader ---------------------------------------------------------------------------------------------------
def read(text):
    """-> (segments: dict id -> sequence, links: list of (u, v), paths: list of (name, [ids])); asserts the layout: one
    header, then S, L, P lines in this order, tab separated, every line ended by a line feed."""
    assert text.endswith(b"\n")
    lines = text[:-1].split(b"\n")
    assert lines[0] + b"\n" == HEADER
    segs, lks, paths, order = {}, [], [], []
    for line in lines[1:]:
        f = line.split(b"\t")
        order.append(f[0])
        if f[0] == b"S":
            assert len(f) == 3 and f[2] and int(f[1]) == len(segs) + 1 and str(int(f[1])).encode() == f[1]
            segs[int(f[1])] = f[2]
        elif f[0] == b"L":
            assert len(f) == 6 and f[2] == f[4] == b"+" and f[5] == b"0M"
            lks.append((int(f[1]), int(f[3])))
        else:
            assert f[0] == b"P" and len(f) == 4 and f[3] == b"*" and f[1]
            steps = f[2].split(b",")
            assert all(s.endswith(b"+") for s in steps)
            paths.append((f[1], [int(s[:-1]) for s in steps]))
    assert order == sorted(order, key=b"SLP".index)
    return segs, lks, paths


def language(syms):
    """All words of a (small) EDS."""
    return {b"".join(w) for w in itertools.product(*syms)}


def complete_walk_words(syms, segs, lks):
    """The sequences of all walks that start at a segment with only open symbols in front of it and end at one with only
    open symbols behind it."""
    ids = segment_ids(syms)
    is_open = [any(not s for s in strings) for strings in syms]
    starts = [k for i, row in enumerate(ids) if all(is_open[:i]) for k in row if k is not None]
    ends = {k for i, row in enumerate(ids) if all(is_open[i + 1:]) for k in row if k is not None}
    nxt = {}
    for u, v in lks:
        nxt.setdefault(u, []).append(v)
    words = set()

    def go(u, word):
        word = word + segs[u]
        if u in ends:
            words.add(word)
        for v in nxt.get(u, ()):
            go(v, word)
    for s in starts:
        go(s, b"")
    return words
