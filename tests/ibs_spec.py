"""Python restatement of the shared-segment specification (edsx_paths_ibs / edsparser-ibs), for well formed texts: brute
force over tests/path_spec.py's parse and tests/dist_spec.py's chosen.  It walks all symbols of every pair: no class list,
no bit rows, no chunks.  TEST INFRASTRUCTURE: the comparator of tests/test_ibs_*.py, never imported by edsparser_amd/.

Two paths agree at a symbol iff they take the same string index there (two paths without a string agree; equal texts are
not merged; a fixed symbol - a single universal string - is taken by everybody).  A segment of a pair is a maximal non-empty
run of symbols at all of which the two agree.  Its record is (x, y, symbol_first, symbol_last, sites, column_first,
column_end): x < y request positions, sites the choice symbols inside (every symbol that is not fixed), the columns those of
the alignment view, col[symbol_first] and col[symbol_last + 1].  It is reported iff sites >= min_sites and column_end -
column_first >= min_columns.  Records come in (x, y, symbol_first) order; pair_off is the CSR over the pairs in row-major
upper-triangle order."""
import dist_spec as ds
import path_spec as ps

FIELDS = ("x", "y", "symbol_first", "symbol_last", "sites", "column_first", "column_end")


def layout(syms, sets):
    """-> (choice flag per symbol, col with n + 1 entries)"""
    choice, col, sid = [], [0], 0
    for strings in syms:
        choice.append(not (len(strings) == 1 and 0 in sets[sid]))
        col.append(col[-1] + max(len(s) for s in strings))
        sid += len(strings)
    return choice, col


def ibs(eds, seds, paths=None, min_sites=1, min_columns=0):
    """-> dict(segments=[7-tuples], pair_off=[...], info={paths, choice_symbols, pairs, candidate_segments, segments});
    paths None or empty: all paths 1..P; ValueError with the library's text for an id outside 1..P"""
    syms, sets, P = ps.parse(eds, seds)
    paths = list(paths) if paths else list(range(1, P + 1))
    for p in paths:
        if p < 1 or p > P:
            raise ValueError("Path id %d out of range (1..%d)" % (p, P))
    choice, col = layout(syms, sets)
    n, K = len(syms), len(paths)
    ch = {p: ds.chosen(syms, sets, p) for p in set(paths)}
    nchoice = [0]
    for c in choice:
        nchoice.append(nchoice[-1] + int(c))
    recs, pair_off, cand = [], [0], 0
    for x in range(K):
        for y in range(x + 1, K):
            a, b = ch[paths[x]], ch[paths[y]]
            i = 0
            while i < n:
                if a[i] != b[i]:
                    i += 1
                    continue
                j = i
                while j + 1 < n and a[j + 1] == b[j + 1]:
                    j += 1
                sites = nchoice[j + 1] - nchoice[i]
                cand += 1
                if sites >= min_sites and col[j + 1] - col[i] >= min_columns:
                    recs.append((x, y, i, j, sites, col[i], col[j + 1]))
                i = j + 1
            pair_off.append(len(recs))
    info = {"paths": K, "choice_symbols": nchoice[-1], "pairs": K * (K - 1) // 2, "candidate_segments": cand, "segments": len(recs)}
    return {"segments": recs, "pair_off": pair_off, "info": info}


def default_names(paths, prefix=b"s"):
    return [prefix + str(p - 1).encode() for p in paths]


HEADER = b"path_a\tpath_b\tsymbol_first\tsymbol_last\tsites\tcolumn_first\tcolumn_end\tcolumns\n"


def text(eds, seds, paths=None, min_sites=1, min_columns=0, names=None, prefix=b"s"):
    """what edsparser-ibs writes: the header, then one line per record in record order: the names of the two paths -
    one per requested path, else <prefix><id - 1> -, the five numbers of the record and column_end - column_first"""
    _, _, P = ps.parse(eds, seds)
    req = list(paths) if paths else list(range(1, P + 1))
    names = list(names) if names else default_names(req, prefix)
    out = [HEADER]
    for x, y, sf, sl, sites, cf, ce in ibs(eds, seds, paths, min_sites, min_columns)["segments"]:
        out.append(names[x] + b"\t" + names[y] + b"\t%d\t%d\t%d\t%d\t%d\t%d\n" % (sf, sl, sites, cf, ce, ce - cf))
    return b"".join(out)
