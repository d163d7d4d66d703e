"""Python restatement of the region slice specification (edsx_paths_slice / edsparser-slice), by brute force,
for well formed texts: lists of strings, Python slicing and a renderer over tests/path_spec.py.  TEST INFRASTRUCTURE: the
comparator of tests/test_slice_*.py, never imported by edsparser_amd/."""
import path_spec as ps

U64_MAX = 2 ** 64 - 1
OK, RANGE = 0, 4
FIELDS = ("symbol_first", "symbol_last", "cut_first", "cut_end", "column_first", "column_end", "strings", "chars", "eds_off", "eds_len",
          "seds_off", "seds_len")


def render(syms, sets):
    """FULL-form texts: braces around every symbol, one {ids} per string, a set that holds 0 as {0}, a line feed each."""
    eds = b"".join(b"{" + b",".join(s) + b"}" for s in syms) + b"\n"
    seds = b"".join(b"{0}" if 0 in q else b"{" + b",".join(str(x).encode() for x in sorted(q)) + b"}" for q in sets) + b"\n"
    return eds, seds


class Model:
    def __init__(self, eds, seds):
        self.syms, self.sets, self.P = ps.parse(eds, seds)
        self.n = len(self.syms)
        self.first, self.col = [0], [0]                          # first string / first alignment column of every symbol
        for s in self.syms:
            self.first.append(self.first[-1] + len(s))
            self.col.append(self.col[-1] + max(len(t) for t in s))
        self.W = self.col[-1]

    def offsets(self, p):
        """at[i]: characters of path p in front of symbol i (n + 1 entries); p == 0: the columns."""
        if p == 0:
            return self.col
        at = [0]
        for s, f in zip(self.syms, self.first):
            at.append(at[-1] + next((len(t) for j, t in enumerate(s) if {p, 0} & self.sets[f + j]), 0))
        return at

    def length(self, p):
        return self.offsets(p)[-1]

    def ends(self, p, start, end):
        """-> (i0, i1, o0, o1e, c0, c1e), or None for a region that is empty or leaves the path (the columns)."""
        if p > self.P:
            raise ValueError("Path id %d out of range (1..%d)" % (p, self.P))
        at = self.offsets(p)
        if start >= end or end > at[-1]:
            return None
        i0 = max(i for i in range(self.n) if at[i] <= start)     # the LARGEST symbol that begins at or in front of it
        i1 = max(i for i in range(self.n) if at[i] <= end - 1)
        o0, o1 = start - at[i0], end - 1 - at[i1]
        return i0, i1, o0, o1 + 1, self.col[i0] + o0, self.col[i1] + o1 + 1

    def cut(self, p, start, end):
        """-> (symbols, sets, ends) of the slice, or None"""
        e = self.ends(p, start, end)
        if e is None:
            return None
        i0, i1, o0, o1e = e[:4]
        syms = [list(s) for s in self.syms[i0:i1 + 1]]
        syms[-1] = [t[:o1e] for t in syms[-1]]                   # (first the end: both offsets count from the string's start)
        syms[0] = [t[o0:] for t in syms[0]]
        return syms, self.sets[self.first[i0]:self.first[i1 + 1]], e

    def slice(self, path, start, end, max_bytes=0):
        """-> (eds, seds, {field: list}, status list) of the regions laid end to end, as edsx_paths_slice gives them"""
        eds, seds, status = [], [], []
        reg = {f: [] for f in FIELDS}
        eo = so = 0
        for p, s, e in zip(path, start, end):
            c = self.cut(p, s, e)
            if c is None:
                status.append(RANGE)
                for f in FIELDS:
                    reg[f].append(0 if f in ("eds_len", "seds_len") else U64_MAX)
                continue
            te, ts = render(c[0], c[1])
            vals = c[2] + (len(c[1]), sum(len(t) for x in c[0] for t in x), eo, len(te), so, len(ts))
            for f, v in zip(FIELDS, vals):
                reg[f].append(v)
            status.append(OK)
            eds.append(te)
            seds.append(ts)
            eo += len(te)
            so += len(ts)
        if max_bytes and eo + so > max_bytes:
            raise ValueError("Slices have %d bytes, above the limit of %d" % (eo + so, max_bytes))
        return b"".join(eds), b"".join(seds), reg, status
