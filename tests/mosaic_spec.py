"""Python restatement of the mosaic specification (edsx_paths_mosaic / edsparser-mosaic), for well formed texts: brute
force over tests/path_spec.py's parse and tests/dist_spec.py's chosen.  It walks all symbols of every (target, donor): no
class list, no bit rows, no words.  TEST INFRASTRUCTURE: the comparator of tests/test_mosaic_*.py, never imported by
edsparser_amd/.

Two paths agree at a symbol iff they take the same string index there (tests/ibs_spec.py).  For the target position x with
path t a donor position y is eligible iff donors[y] != t.  From s = 0, while s < n: e(y) is the first symbol >= s at which t
and donors[y] differ (n without one), best the largest e(y) over the eligible y.  With an eligible donor and best > s the
record is a copy of [s, best - 1] from the smallest eligible y with e(y) = best, and s = best; else it is private (donor
NONE): [s, j - 1], j the first symbol > s at which some eligible donor agrees with t, or n, and s = j.  The record is
(target, donor, symbol_first, symbol_last, sites, column_first, column_end), sites and columns as in tests/ibs_spec.py.
Records come in (target, symbol_first) order; target_off is the CSR over the targets."""
import dist_spec as ds
import ibs_spec as isp
import path_spec as ps

NONE = 2 ** 64 - 1
FIELDS = ("target", "donor", "symbol_first", "symbol_last", "sites", "column_first", "column_end")


def requested(eds, seds, targets, donors):
    """-> (targets, donors) as id lists; None or empty: all paths; ValueError with the library's text for an id outside 1..P"""
    P = ps.parse(eds, seds)[2]
    targets = list(targets) if targets else list(range(1, P + 1))
    donors = list(donors) if donors else list(range(1, P + 1))
    for p in targets + donors:
        if p < 1 or p > P:
            raise ValueError("Path id %d out of range (1..%d)" % (p, P))
    return targets, donors


def mosaic(eds, seds, targets=None, donors=None):
    """-> dict(segments=[7-tuples], target_off=[...], info={targets, donors, choice_symbols, segments, private_segments,
    private_symbols, switches})"""
    syms, sets, P = ps.parse(eds, seds)
    targets, donors = requested(eds, seds, targets, donors)
    choice, col = isp.layout(syms, sets)
    n = len(syms)
    ch = {p: ds.chosen(syms, sets, p) for p in set(targets) | set(donors)}
    nchoice = [0]
    for c in choice:
        nchoice.append(nchoice[-1] + int(c))
    recs, off = [], [0]
    for x, t in enumerate(targets):
        eligible = [y for y, d in enumerate(donors) if d != t]
        a, s = ch[t], 0
        while s < n:
            best, who = s, NONE
            for y in eligible:
                b, e = ch[donors[y]], s
                while e < n and a[e] == b[e]:
                    e += 1
                if e > best:
                    best, who = e, y
            if who == NONE:
                best = s + 1
                while best < n and not any(ch[donors[y]][best] == a[best] for y in eligible):
                    best += 1
            recs.append((x, who, s, best - 1, nchoice[best] - nchoice[s], col[s], col[best]))
            s = best
        off.append(len(recs))
    private = [r for r in recs if r[1] == NONE]
    info = {"targets": len(targets), "donors": len(donors), "choice_symbols": nchoice[-1], "segments": len(recs),
            "private_segments": len(private), "private_symbols": sum(r[3] - r[2] + 1 for r in private),
            "switches": len(recs) - len(targets) if n else 0}
    return {"segments": recs, "target_off": off, "info": info}


def default_names(paths, prefix=b"s"):
    return [prefix + str(p - 1).encode() for p in paths]


HEADER = b"target\tdonor\tsymbol_first\tsymbol_last\tsites\tcolumn_first\tcolumn_end\tcolumns\n"
BREAKPOINT_HEADER = b"target\tdonor_before\tdonor_after\tsymbol\tcolumn\n"


def _names(eds, seds, targets, donors, names, prefix):
    """the names of the target and of the donor positions: line id of `names` (a list with one name per path 1..P), else
    <prefix><id - 1>"""
    targets, donors = requested(eds, seds, targets, donors)
    if names:
        return [names[p - 1] for p in targets], [names[p - 1] for p in donors]
    return default_names(targets, prefix), default_names(donors, prefix)


def text(eds, seds, targets=None, donors=None, names=None, prefix=b"s"):
    """what edsparser-mosaic writes: the header, then one line per record in record order: the names of the target and of
    the donor ("." for a private segment), the five numbers of the record and column_end - column_first"""
    tn, dn = _names(eds, seds, targets, donors, names, prefix)
    out = [HEADER]
    for x, y, sf, sl, sites, cf, ce in mosaic(eds, seds, targets, donors)["segments"]:
        out.append(tn[x] + b"\t" + (b"." if y == NONE else dn[y]) + b"\t%d\t%d\t%d\t%d\t%d\t%d\n" % (sf, sl, sites, cf, ce, ce - cf))
    return b"".join(out)


def breakpoints(eds, seds, targets=None, donors=None, names=None, prefix=b"s"):
    """what edsparser-mosaic --breakpoints writes: one line per place where the donor of a target changes, that is per
    segment of a target but its first: the target, the donor before and the donor after ("." for private), and the symbol
    and the column at which the new segment starts"""
    tn, dn = _names(eds, seds, targets, donors, names, prefix)
    got = mosaic(eds, seds, targets, donors)
    out = [BREAKPOINT_HEADER]
    who = lambda y: b"." if y == NONE else dn[y]
    for x in range(len(tn)):
        mine = got["segments"][got["target_off"][x]:got["target_off"][x + 1]]
        for a, b in zip(mine, mine[1:]):
            out.append(tn[x] + b"\t" + who(a[1]) + b"\t" + who(b[1]) + b"\t%d\t%d\n" % (b[2], b[5]))
    return b"".join(out)
