"""Python restatement of the alignment export specification (edsx_paths_align / eds2msa), for well formed texts, built on
tests/path_spec.py.  TEST INFRASTRUCTURE: the comparator of tests/test_msa_export_*.py, never imported by edsparser_amd/."""
import path_spec as ps

BAD_GAPS = b">\n\r {},"


def widths(syms):
    """w[i]: the length of the longest string of symbol i, over ALL its strings."""
    return [max(len(s) for s in strings) for strings in syms]


def row(syms, sets, p, gap=b"-"):
    """-> (row of path p: per symbol the chosen string left-justified in w[i] columns, missing)"""
    out, missing, sid = [], 0, 0
    for strings, w in zip(syms, widths(syms)):
        for j, s in enumerate(strings):
            if p in sets[sid + j] or 0 in sets[sid + j]:
                out.append(s + gap * (w - len(s)))
                break
        else:
            out.append(gap * w)
            missing += 1
        sid += len(strings)
    return b"".join(out), missing


def info(eds, seds):
    syms, sets, P = ps.parse(eds, seds)
    w = widths(syms)
    return {"n_symbols": len(syms), "n_columns": sum(w), "n_zero_width_symbols": w.count(0), "widest_symbol": max(w + [0]),
            "num_paths": P}


def size(eds, seds, paths=None, line_width=60, names=None, prefix=b"path"):
    """The exact size of the text, from the counts alone."""
    syms, sets, P = ps.parse(eds, seds)
    paths = list(paths) if paths else list(range(1, P + 1))
    W = sum(widths(syms))
    lw = line_width if line_width else max(W, 1)
    heads = sum(len(names[k] if names else prefix + str(p).encode()) + 2 for k, p in enumerate(paths))
    return heads + len(paths) * (W + (W + lw - 1) // lw)


def align(eds, seds, paths=None, line_width=60, names=None, prefix=b"path", gap=b"-", max_bytes=0):
    """-> (FASTA bytes, [missing per record]); paths None or empty: all paths 1..P.  ValueError with the library's text for
    an id outside 1..P, an unusable gap byte and a text above max_bytes."""
    syms, sets, P = ps.parse(eds, seds)
    paths = list(paths) if paths else list(range(1, P + 1))
    for p in paths:
        if p < 1 or p > P:
            raise ValueError("Path id %d out of range (1..%d)" % (p, P))
    gap = gap or b"-"
    if len(gap) != 1 or gap in BAD_GAPS or gap == b"\0":
        raise ValueError("Gap character is not usable in an alignment")
    n = size(eds, seds, paths, line_width, names, prefix)
    if max_bytes and n > max_bytes:
        raise ValueError("Alignment has %d bytes, above the limit of %d" % (n, max_bytes))
    out, miss = [], []
    for k, p in enumerate(paths):
        r, m = row(syms, sets, p, gap)
        out.append(ps.record(names[k] if names else prefix + str(p).encode(), r, line_width))
        miss.append(m)
    text = b"".join(out)
    assert len(text) == n
    return text, miss


def rows_of(fasta):
    """[(name, row without line feeds)] of an aligned FASTA."""
    out = []
    for rec in fasta.split(b">")[1:]:
        name, _, body = rec.partition(b"\n")
        out.append((name, body.replace(b"\n", b"")))
    return out
