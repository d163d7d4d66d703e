"""Inputs of the path distance tests (tests/test_dist_cpu.py, test_dist_gpu.py, dist_guard_child.py): random EDSs with
overlapping sets, missing paths, universal strings inside multi-string symbols, empty strings and equal texts; the
boundary shapes of the kernels; and the class list of tests/dist_spec.py's units restated in Python, so that a test can
say how many class columns a shape has.  TEST INFRASTRUCTURE, never imported by edsparser_amd/."""
import random

import path_spec as ps

NOCHAR, NOSTRING = 256, (1 << 24) - 1
CHUNK_COLUMNS = 4096                                             # of the pair kernel, while there are few workgroups


def set_text(q):
    return b"{" + b",".join(b"%d" % x for x in sorted(q)) + b"}"


def render(syms, sets):
    return b"".join(b"{" + b",".join(s) + b"}" for s in syms), b"".join(set_text(q) for q in sets)


def random_eds(rng, n_symbols, P, alphabet=b"ACGT"):
    syms, sets = [], []
    for _ in range(n_symbols):
        k = rng.choice([1, 1, 2, 2, 3, 4])
        strings = [bytes(rng.choice(alphabet) for _ in range(rng.choice([0, 0, 1, 1, 2, 3, 5]))) for _ in range(k)]
        if k > 1 and rng.random() < 0.2:
            strings[rng.randrange(k)] = strings[0]              # equal texts
        syms.append(strings)
        for j in range(k):
            r = rng.random()
            if (k == 1 and r < 0.5) or (k > 1 and r < 0.12):
                sets.append({0})                                 # universal, also inside a multi-string symbol
            else:
                sets.append(set(rng.sample(range(1, P + 1), rng.randint(1, min(3, P)))))   # overlapping, with paths left out
    return render(syms, sets)


def wide_eds(rng, P=130, n_symbols=40):
    """P paths, every symbol splits them into 2..4 strings and leaves about a tenth out; fixed symbols in between"""
    syms, sets = [], []
    for i in range(n_symbols):
        if i % 5 == 4:
            syms.append([b"ACGT"]); sets.append({0})
            continue
        k = rng.choice([2, 3, 4])
        strings = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 4))) for _ in range(k)]
        part = [set() for _ in range(k)]
        for p in range(1, P + 1):
            if rng.random() < 0.9:
                part[rng.randrange(k)].add(p)
        for q in part:
            if not q:
                q.add(rng.randint(1, P))
        syms.append(strings); sets += part
    syms.append([b"A", b"C"]); sets += [{P}, {1}]               # P is the largest id
    return render(syms, sets)


def snp_eds(pairs, triples=0):
    """`pairs` symbols {A,C} and `triples` symbols {A,C,G} over the paths 1 and 2, fixed symbols in between: 2 * pairs + 3 *
    triples class columns under both metrics (the third string of a triple is a class that no path takes)"""
    eds = (b"{A,C}" + b"{TT}") * pairs + b"{A,C,G}" * triples
    seds = (b"{1}{2}" + b"{0}") * pairs + b"{1}{2}{1}" * triples
    return eds, seds


def with_columns(c):
    """an EDS with exactly c class columns, c >= 2"""
    return snp_eds((c - 3) // 2, 1) if c % 2 else snp_eds(c // 2)


def long_string_eds(rng, length=3000):
    """{X,}: every column of X is a byte or no character, 2 * length class columns from one symbol"""
    x = bytes(rng.choice(b"ACGT") for _ in range(length))
    return b"{GA}{" + x + b",}{T}", b"{0}{1,3}{2}{0}"


# a symbol with 65 strings; a universal string second; a path in two sets of one symbol; paths missing in some symbols and
# path 66 missing everywhere (P = 67); empty strings; a zero-width symbol that is not universal; bytes from 0x80 on; '-' in a string
EDGE = (b"{" + b",".join(b"%c%c" % (65 + k % 26, 97 + k // 26) for k in range(65)) + b"}" +
        b"{A,C,G}{A,C}{AC}{,T}{}{\x80\xff,\xc3\xa9,A\x80}{A-C,---,AC}{G,GG,GGG}{T}{C,C}",
        b"".join(b"{%d}" % (k + 1) for k in range(65)) +
        b"{1}{0}{2}" b"{1,2}{2,3}" b"{0}" b"{1,5}{2,6}" b"{3}" b"{1}{2,3}{5,6,7}" b"{1,2}{3}{5}" b"{1}{2}{3,5}" b"{0}" b"{1,3}{2,67}")


def boundary_shapes():
    """name -> (eds, seds, requests): the smallest shapes at which the kernels can go wrong; a request is a list of path ids
    or None for all paths"""
    rng = random.Random(8)
    wide = wide_eds(rng)
    alone_twice = [[p] for p in (63, 64, 65, 127, 128)] + [[p, p] for p in (63, 64, 65, 127, 128)]
    shapes = {
        "wide": wide + ([list(range(1, K + 1)) for K in (1, 2, 63, 64, 65, 129)] + alone_twice +
                        [list(range(130, 0, -1)), [130, 1, 64, 64, 65, 1]],),
        "fixed": (b"{ACGT}{GG}{}", b"{0,3}{0}{0,1}", [None, [3, 3, 1]]),      # no choice symbol, three paths
        "edge": EDGE + ([None, [66, 66, 1], [67, 65, 66, 2, 1]],),
        "long": long_string_eds(rng) + ([None],),
    }
    for c in (63, 64, 65, CHUNK_COLUMNS - 1, CHUNK_COLUMNS, CHUNK_COLUMNS + 1):
        shapes["columns%d" % c] = with_columns(c) + ([None],)
    return shapes


def classes(eds, seds, metric):
    """-> (descriptors, V): the class columns of the specification's units in order, as (unit, value) for columns - unit
    counts the columns of the choice symbols, value a byte or NOCHAR - and (rank, index) for strings - the rank of the
    symbol among the choice symbols, index within the symbol or NOSTRING.  A choice symbol is one that is not a single
    universal string; it may leave a path out when no set is universal and their union lacks an id of 1..P; a unit with
    fewer than two classes is not listed."""
    syms, sets, P = ps.parse(eds, seds)
    desc, V, sid, rank, unit = [], 0, 0, 0, 0
    for strings in syms:
        q = sets[sid:sid + len(strings)]
        sid += len(strings)
        if len(strings) == 1 and 0 in q[0]:
            continue
        miss = not any(0 in s for s in q) and bool(set(range(1, P + 1)) - set().union(*q))
        if metric == "strings":
            c = [(rank, j) for j in range(len(strings))] + ([(rank, NOSTRING)] if miss else [])
            if len(c) >= 2:
                desc += c
                V += 1
        else:
            for off in range(max(len(s) for s in strings)):
                vals = sorted(set(s[off] for s in strings if len(s) > off))
                if miss or any(len(s) <= off for s in strings):
                    vals.append(NOCHAR)
                if len(vals) >= 2:
                    desc += [(unit + off, v) for v in vals]
                    V += 1
            unit += max(len(s) for s in strings)
        rank += 1
    return desc, V
