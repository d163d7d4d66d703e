"""Python restatement of the path distance specification (edsx_paths_distances / edsparser-dist), for well formed texts:
brute force over tests/path_spec.py's parse.  TEST INFRASTRUCTURE: the comparator of tests/test_dist_*.py, never imported
by edsparser_amd/."""
import path_spec as ps

NOCHAR = 256                                                     # "no character": equals itself, differs from every byte
METRICS = ("columns", "strings")


def chosen(syms, sets, p):
    """per symbol the index, within the symbol, of the first string whose set holds p or 0; None where there is none"""
    out, sid = [], 0
    for strings in syms:
        out.append(next((j for j in range(len(strings)) if p in sets[sid + j] or 0 in sets[sid + j]), None))
        sid += len(strings)
    return out


def shown(syms, sets, p):
    """the row of path p in the alignment view, one value per column: the bytes of its chosen strings left-justified in
    w[i] columns, NOCHAR elsewhere -> (values, missing)"""
    row, ch = [], chosen(syms, sets, p)
    for strings, j in zip(syms, ch):
        w = max(len(s) for s in strings)
        s = strings[j] if j is not None else b""
        row += list(s) + [NOCHAR] * (w - len(s))
    return row, ch.count(None)


def units(syms, metric):
    """the denominator of a normalised distance: W for columns, the number of symbols for strings"""
    return sum(max(len(s) for s in strings) for strings in syms) if metric == "columns" else len(syms)


def matrix(eds, seds, paths=None, metric="columns"):
    """-> (K x K list of lists, [missing per path], units); paths None or empty: all paths 1..P; ValueError with the
    library's text for an id outside 1..P and for an unknown metric."""
    if metric not in METRICS:
        raise ValueError("unknown metric")
    syms, sets, P = ps.parse(eds, seds)
    paths = list(paths) if paths else list(range(1, P + 1))
    for p in paths:
        if p < 1 or p > P:
            raise ValueError("Path id %d out of range (1..%d)" % (p, P))
    rows, miss = {}, {}
    for p in set(paths):
        if metric == "columns":
            rows[p], miss[p] = shown(syms, sets, p)
        else:
            rows[p] = chosen(syms, sets, p)
            miss[p] = rows[p].count(None)
    D = [[sum(1 for x, y in zip(rows[a], rows[b]) if x != y) for b in paths] for a in paths]
    return D, [miss[p] for p in paths], units(syms, metric)


def default_names(paths, prefix=b"s"):
    return [prefix + str(p - 1).encode() for p in paths]


def text(eds, seds, paths=None, metric="columns", fmt="tsv", normalize=False, names=None, prefix=b"s"):
    """what edsparser-dist writes: tsv - "path\\t<names>" and per row "<name>\\t<values>"; phylip - "K" and per row the
    name and the K values separated by single blanks; values decimal, or %.6f of D / units with normalize (units 0:
    0.000000); names: one per requested path, else <prefix><id - 1>"""
    D, _, u = matrix(eds, seds, paths, metric)
    _, _, P = ps.parse(eds, seds)
    paths = list(paths) if paths else list(range(1, P + 1))
    names = list(names) if names else default_names(paths, prefix)
    cell = (lambda d: b"%.6f" % (d / u if u else 0.0)) if normalize else (lambda d: b"%d" % d)
    sep = b"\t" if fmt == "tsv" else b" "
    head = b"path\t" + b"\t".join(names) + b"\n" if fmt == "tsv" else b"%d\n" % len(paths)
    if fmt == "tsv" and not paths:
        head = b"path\n"
    return head + b"".join(n + sep + sep.join(cell(d) for d in row) + b"\n" for n, row in zip(names, D))
