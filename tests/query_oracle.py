"""Python restatement of the EDS query side: EDS::check_position and the seeded pattern sampler.

Our own code, written from the reference's src/cpp/lib/formats/eds.cpp (line numbers below), with the pins of
edsparser's container where the reference reads past its tables: a common position >= num_common_chars is False, a
degenerate string number >= the number of degenerate strings is 'out_of_range', a wrap-around symbol without a
non-empty string is an error instead of an endless loop.  Results: True / False / 'out_of_range' / 'invalid_argument'.
"""

M64 = (1 << 64) - 1


def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def hash3(seed, a, b):
    return mix64((seed ^ mix64((a ^ mix64((b + 0x632BE59BD9B4E019) & M64)) & M64)) & M64)


def draw(seed, i, k, bound):
    """Draw k of pattern i in [0, bound): the high 64 bits of hash3(seed, i, k) * bound."""
    return (hash3(seed, i, k) * bound) >> 64


def parse(text):
    """eds.cpp:39-155 on well-formed text: whitespace dropped, a bare run is a symbol of one string."""
    s = "".join(ch for ch in text if not ch.isspace())
    sets, i = [], 0
    while i < len(s):
        if s[i] == "{":
            j = s.index("}", i)
            sets.append(s[i + 1:j].split(","))
            i = j + 1
        else:
            j = s.find("{", i)
            j = len(s) if j < 0 else j
            sets.append([s[i:j]])
            i = j
    return sets


def parse_sources(text):
    return [set(int(x) for x in grp.split(",") if x) for grp in "".join(text.split()).strip("{}").split("}{")]


class Eds:
    def __init__(self, text, seds=None):
        self.sets = parse(text)
        self.n = len(self.sets)
        self.sources = parse_sources(seds) if seds is not None else None
        self.deg = [len(s) > 1 for s in self.sets]
        self.cum_common, self.cum_deg = [0], [0]        # eds.cpp:438-469
        for s, d in zip(self.sets, self.deg):
            self.cum_common.append(self.cum_common[-1] + (0 if d else len(s[0])))
            self.cum_deg.append(self.cum_deg[-1] + (len(s) if d else 0))
        self.C = self.cum_common[-1]
        self.first_sid = []
        k = 0
        for s in self.sets:
            self.first_sid.append(k)
            k += len(s)


def _start(e, pos):
    """find_symbol_at_common_position (:1098-1138) for pos < C: the last symbol with cum_common <= pos."""
    lo, hi = 0, e.n
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if e.cum_common[mid] <= pos:
            lo = mid
        else:
            hi = mid
    return lo, pos - e.cum_common[lo]


class _Err(Exception):
    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


def _decode(e, num, sym):
    """decode_degenerate_string_number (:1051-1095) + the symbol test of :1171 / :1334 -> local index"""
    if num < 0:
        raise _Err("invalid_argument")
    if num >= e.cum_deg[-1]:
        raise _Err("out_of_range")
    if not (e.cum_deg[sym] <= num < e.cum_deg[sym + 1]):
        raise _Err("invalid_argument")
    return num - e.cum_deg[sym]


def _walk(e, s, off, choices, L):
    """The symbols visited by reconstruct_from_memory (:1141-1209) and calculate_path_intersection (:1300-1418):
    yields (string id, text taken) per step; raises _Err at a bad or missing choice."""
    got, d = 0, 0
    sym = s
    while sym < e.n and got < L:
        if e.deg[sym]:
            if d >= len(choices):
                raise _Err("invalid_argument")
            j = _decode(e, choices[d], sym)
            d += 1
            text = e.sets[sym][j]
        else:
            j = 0
            text = e.sets[sym][0][off if sym == s else 0:]
        take = text[:L - got]
        got += len(take)
        yield e.first_sid[sym] + j, take
        sym += 1


def check(e, pos, choices, pattern):
    """EDS::check_position (:953-1047)."""
    if e.n == 0:
        return False
    if not pattern:
        return True
    if pos >= e.C:
        return False
    s, off = _start(e, pos)
    L = len(pattern)
    try:
        if e.sources is not None:                     # :1001-1018, the intersection walk first
            acc = None
            for sid, _ in _walk(e, s, off, choices, L):
                cur = e.sources[sid]
                if acc is None:
                    acc = set(cur)
                elif 0 in cur and 0 in acc:
                    acc = {0}
                elif 0 in cur:
                    pass
                elif 0 in acc:
                    acc = set(cur)
                else:
                    acc &= cur
                if not acc:
                    return False
        rec = "".join(t for _, t in _walk(e, s, off, choices, L))
    except _Err as x:
        return x.kind
    return len(rec) >= L and rec == pattern


def extract(e, pos, length, changes):
    if e.n == 0:
        return ("runtime_error", "Cannot extract from empty EDS")
    if pos >= e.n:
        return ("out_of_range", "Start position exceeds EDS length")
    if length == 0:
        return ""
    end = min(pos + length, e.n)
    if len(changes) != end - pos:
        return ("invalid_argument", "changes vector size")
    out = []
    for i, c in enumerate(changes):
        st = e.sets[pos + i]
        if c < 0 or c >= len(st):
            return ("out_of_range", "Change index")
        out.append(st[c])
    return "".join(out)


def generate(e, count, L, seed):
    """The seeded sampler (:673-769 with the shared draw sequence).  Returns (text bytes, witnesses) with one
    (start common position or None, [degenerate string numbers]) per pattern, None for wrapped patterns and EDSs
    without common characters; raises RuntimeError naming the symbol when a wrap reaches one without a non-empty
    string."""
    if e.n == 0:
        raise RuntimeError("Cannot generate patterns from empty EDS")
    if L == 0:
        raise ValueError("Pattern length must be greater than 0")
    out, wit = [], []
    for i in range(count):
        pat, cur, off, p = "", 0, 0, None
        if e.C > 0:
            p = draw(seed, i, 0, e.C)
            cur, off = _start(e, p)
        k, first, chosen = 1, True, []
        while len(pat) < L and cur < e.n:
            st = e.sets[cur]
            j = draw(seed, i, k, len(st))
            k += 1
            frm = off if first else 0
            if frm < len(st[j]):
                pat += st[j][frm:frm + L - len(pat)]
            if len(st) > 1:
                chosen.append(e.cum_deg[cur] + j)
            first = False
            if len(pat) < L:
                cur += 1
        wrapped = len(pat) < L
        while len(pat) < L:
            w = len(pat) % e.n
            ne = [x for x in e.sets[w] if x]
            if not ne:
                raise RuntimeError("Cannot generate pattern %d: the wrap-around reaches symbol %d, which has no "
                                   "non-empty string" % (i, w))
            pat += ne[draw(seed, i, k, len(ne))][:L - len(pat)]
            k += 1
        out.append(pat)
        wit.append((None, []) if wrapped or e.C == 0 else (p, chosen))
    return "".join(x + "\n" for x in out).encode(), wit
