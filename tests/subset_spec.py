"""Python restatement of the path subsetting specification (edsx_eds_subset / edsparser-subset), by brute force on parsed
lists.  TEST INFRASTRUCTURE: the comparator of tests/test_subset_*.py, never imported by edsparser_amd/.  The texts are
parsed by path_spec.parse; nothing of the parsing is restated here."""
import path_spec as ps

INFO_FIELDS = ("symbols_in", "symbols_out", "strings_in", "strings_out", "chars_in", "chars_out", "paths_in", "paths_out",
               "symbols_removed", "common_runs_merged")


def check_ids(ids, P):
    """The keep set as the sorted list of its ids; ValueError with the library's text otherwise."""
    ids = list(ids)
    if not ids:
        raise ValueError("No paths selected")
    seen = set()
    for p in ids:
        if p < 1 or p > P:
            raise ValueError("Path id %d out of range (1..%d)" % (p, P))
        if p in seen:
            raise ValueError("Path id %d given twice" % p)
        seen.add(p)
    return sorted(seen)


def subset_parsed(syms, sets, P, ids, keep_ids=False):
    """-> (symbols: list of lists of bytes, sources: one sorted list of ints per string, info) of the subset to `ids`."""
    K = check_ids(ids, P)
    new_id = {p: (p if keep_ids else r + 1) for r, p in enumerate(K)}
    Kset = set(K)
    # steps 1 and 2: per symbol the kept strings with their new sets; None marks a common symbol's set
    survivors, removed, sid = [], 0, 0
    for strings in syms:
        kept = []
        for j, text in enumerate(strings):
            S = sets[sid + j]
            if 0 in S:
                kept.append((text, [0], True))
            elif S & Kset:
                kept.append((text, sorted(new_id[p] for p in S & Kset), Kset <= S))
        sid += len(strings)
        if not kept:
            removed += 1
        elif len(kept) == 1 and kept[0][2]:
            survivors.append(("common", kept[0][0]))
        else:
            survivors.append(("other", kept))
    # step 3: runs of adjacent common symbols become one symbol; an empty run is dropped
    out_syms, out_sets, merged = [], [], 0
    k = 0
    while k < len(survivors):
        if survivors[k][0] == "common":
            e = k
            while e < len(survivors) and survivors[e][0] == "common":
                e += 1
            text = b"".join(s[1] for s in survivors[k:e])
            merged += e - k >= 2
            if text:
                out_syms.append([text])
                out_sets.append([0])
            k = e
        else:
            out_syms.append([t for t, _, _ in survivors[k][1]])
            out_sets.extend(s for _, s, _ in survivors[k][1])
            k += 1
    info = {"symbols_in": len(syms), "symbols_out": len(out_syms), "strings_in": len(sets), "strings_out": len(out_sets),
            "chars_in": sum(len(t) for s in syms for t in s), "chars_out": sum(len(t) for s in out_syms for t in s),
            "paths_in": P, "paths_out": len(K), "symbols_removed": removed, "common_runs_merged": merged}
    return out_syms, out_sets, info


def render(out_syms, out_sets):
    """The FULL .eds text and the .seds text, each with its trailing line feed."""
    eds = b"".join(b"{" + b",".join(s) + b"}" for s in out_syms) + b"\n"
    seds = b"".join(b"{" + b",".join(b"%d" % p for p in s) + b"}" for s in out_sets) + b"\n"
    return eds, seds


def subset(eds, seds, ids, keep_ids=False):
    """-> (eds bytes, seds bytes, info dict); ValueError with the library's text for a bad keep set."""
    syms, sets, P = ps.parse(eds, seds)
    out_syms, out_sets, info = subset_parsed(syms, sets, P, ids, keep_ids)
    return render(out_syms, out_sets) + (info,)


def complement(ids, P):
    """--exclude: the ids of 1..P that are not listed (the list itself is checked like a keep set, but may be empty)."""
    drop = set(check_ids(ids, P)) if list(ids) else set()
    return [p for p in range(1, P + 1) if p not in drop]
