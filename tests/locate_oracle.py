"""Brute-force restatement of edsx_eds_locate's contract (include/edsx.h), on query_oracle.Eds.

An occurrence of a pattern P (length L >= 1) is (symbol s, string j of s, offset o < len(string), choices): the walk takes
string[o:], then per following symbol its only string (common) or the string the next choice names (degenerate; a choice is
cum_deg[symbol] + index), each cut to what is still needed, while fewer than L characters are taken and symbols remain.  It
spells P; the choices are exactly the degenerate symbols visited after s; with sources the strings used share a path by the
rule of query_oracle.check.  Order: per pattern, ascending (s, j, o), then depth-first over the alternatives in file order.
Caps: a start stops at max_hits of its own (bit 0 when it had one more); totals sum min(occurrences of the start,
max_hits); a pattern keeps its first max_hits hits (bit 0 when the total is larger); bit 1 when a walk whose characters
match so far needs choice number MAX_CHOICES + 1 (it is cut there).
"""
import query_oracle as qo

U64_MAX = 2 ** 64 - 1
MAX_CHOICES = 64


def share_path(e, sids):
    """The accumulation of query_oracle.check over the strings of a walk."""
    acc = None
    for sid in sids:
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
    return True


def occurrences(e, s, j, o, P, flags):
    """The choice lists of the occurrences that start at (s, j, o), in order (a generator); flags[0] collects bit 1."""
    L = len(P)
    first = e.sets[s][j][o:o + L]
    if not P.startswith(first):
        return

    def rec(sym, got, choices, sids):
        while got < L and sym < e.n and not e.deg[sym]:
            t = e.sets[sym][0][:L - got]
            if P[got:got + len(t)] != t:
                return
            got += len(t)
            sids = sids + [e.first_sid[sym]]
            sym += 1
        if got == L:
            if e.sources is None or share_path(e, sids):
                yield list(choices)
            return
        if sym >= e.n:
            return
        if len(choices) == MAX_CHOICES:
            flags[0] |= 2
            return
        for a, t in enumerate(e.sets[sym]):
            t = t[:L - got]
            if P[got:got + len(t)] == t:
                yield from rec(sym + 1, got + len(t), choices + [e.cum_deg[sym] + a], sids + [e.first_sid[sym] + a])

    yield from rec(s + 1, len(first), [], [e.first_sid[s] + j])


def locate(e, patterns, max_hits=1024, common_only=False):
    """-> dict of lists: hit_off, hits [(common_pos, symbol, string, offset)], choice_off, choices, totals, flags"""
    r = {"hit_off": [0], "hits": [], "choice_off": [0], "choices": [], "totals": [], "flags": []}
    for P in patterns:
        P = P.decode("latin-1") if isinstance(P, bytes) else P
        assert P
        fl, total, kept = [0], 0, []
        for s in range(e.n):
            if common_only and e.deg[s]:
                continue
            for j, text in enumerate(e.sets[s]):
                for o in range(len(text)):
                    if text[o] != P[0]:
                        continue
                    cnt = 0
                    for ch in occurrences(e, s, j, o, P, fl):
                        if cnt == max_hits:
                            fl[0] |= 1
                            break
                        cnt += 1
                        if len(kept) < max_hits:
                            kept.append(((U64_MAX if e.deg[s] else e.cum_common[s] + o, s, j, o), ch))
                    total += cnt
        if total > max_hits:
            fl[0] |= 1
        for hit, ch in kept:
            r["hits"].append(hit)
            r["choices"].extend(ch)
            r["choice_off"].append(len(r["choices"]))
        r["hit_off"].append(len(r["hits"]))
        r["totals"].append(total)
        r["flags"].append(fl[0])
    return r


def random_eds(rng, n_symbols, sources, paths=5, alphabet="AC", max_ids=3):
    """n_symbols sets of 1-3 strings of 0-4 characters (empty alternatives and duplicates included); with sources every
    string gets {0} or 1..max_ids of the paths 1..paths, sometimes with 0 added.  -> (eds text, seds text or None)"""
    sets = []
    for _ in range(n_symbols):
        k = rng.choice([1, 1, 2, 2, 3])
        alts = ["".join(rng.choice(alphabet) for _ in range(rng.choice([0, 1, 1, 2, 3, 4]))) for _ in range(k)]
        if k > 1 and rng.random() < 0.2:
            alts[-1] = alts[0]
        sets.append(alts)
    eds = "".join("{" + ",".join(s) + "}" for s in sets)
    if not sources:
        return eds, None
    groups = []
    for _ in range(sum(len(s) for s in sets)):
        x = rng.random()
        ids = {0} if x < 0.2 else set(rng.sample(range(1, paths + 1), rng.randint(1, min(max_ids, paths))))
        if x > 0.9:
            ids.add(0)
        groups.append("{" + ",".join(str(i) for i in sorted(ids)) + "}")
    return eds, "".join(groups)


def walks(e, pos, L):
    """Every choice list without an unused tail for a walk of L characters from common position pos < e.C."""
    s, off = qo._start(e, pos)

    def rec(sym, got, choices):
        while got < L and sym < e.n and not e.deg[sym]:
            got += len(e.sets[sym][0][off if sym == s else 0:])
            sym += 1
        if got >= L or sym >= e.n:
            yield list(choices)
            return
        for a, t in enumerate(e.sets[sym]):
            yield from rec(sym + 1, got + len(t), choices + [e.cum_deg[sym] + a])

    yield from rec(s, 0, [])
