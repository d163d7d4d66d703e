"""What the directed inputs of tests/contig_walk_cases.py must give, from tests/contig_spec.py and the oracle alone: every
field of every FASTA record, the key of every record line, the regrouped line starts, the counts, the verdict "the host
classifies this file", and the texts of the picked contigs.  Shared by tests/test_contig_walk_cpu.py (the host program)
and tests/test_contig_walk_gpu.py (the library)."""
import numpy as np

import contig_spec as cs
import oracle_lib as o

NONE = 2 ** 64 - 1
_RECORDS, _EXPECT = {}, {}


def records_of(case):
    key = case["name"].replace("weak/", "")
    if key not in _RECORDS:
        _RECORDS[key] = cs.fasta_records(case["F"])
    return _RECORDS[key]


def host_bound(V):
    """the device hands the classification to the host: some record line's first tab field is empty or holds one of ' ',
    '\\r', '\\v', '\\f', or the file holds '\\r' anywhere"""
    if b"\r" in V:
        return True
    for ln in V.split(b"\n"):
        if cs.is_record_line(ln):
            f = ln.split(b"\t")[0]
            if f == b"" or any(ch in f for ch in b" \r\v\f"):
                return True
    return False


def radix_passes(K):
    """8-bit passes that sort the keys 0..K (K: no such contig)"""
    return max(1, min(4, (K.bit_length() + 7) // 8))


def expected(case):
    """dict: recs (K x 7 array: name_off, name_len, rec_start, rec_end, seq_start, line_width, seq_size), names, duplicate,
    host (the verdict), nr, counts (by first token), without_token, unknown, unknown_text; and where the device classifies:
    keys, lsorted, first"""
    key = case["name"].replace("weak/", "")
    if key in _EXPECT:
        return _EXPECT[key]
    V, F = case["V"], case["F"]
    records = records_of(case)
    K = len(records)
    recs = np.zeros((K, 7), dtype=np.uint64)
    index, dup = {}, np.zeros(K, dtype=np.uint64)
    for i, (nm, s, e) in enumerate(records):
        ss, lw, size = cs.fasta_metadata(F, s, e)
        recs[i] = (s + 1, len(nm), s, e, ss, lw, size)
        dup[i] = nm in index
        index.setdefault(nm, i)
    starts, tokens, at = [], [], 0
    for ln in V.split(b"\n"):
        if cs.is_record_line(ln):
            starts.append(at)
            tokens.append(cs.first_token(ln))
        at += len(ln) + 1
    counts = np.zeros(K, dtype=np.uint64)
    unknown, without = {}, 0
    for t in tokens:
        if t is None:
            without += 1
        elif t in index:
            counts[index[t]] += 1
        else:
            unknown[t] = unknown.get(t, 0) + 1                       # (dicts keep the order of first appearance)
    x = {"K": K, "recs": recs, "names": [r[0] for r in records], "duplicate": dup, "index": index, "host": host_bound(V), "nr": len(starts),
         "counts": counts, "without_token": without, "unknown": sum(unknown.values()), "unknown_names": list(unknown.items()),
         "unknown_text": b"".join(b"%s\t%d\n" % kv for kv in unknown.items()), "passes": radix_passes(K)}
    if not x["host"]:
        keys = np.array([index.get(t, K) for t in tokens], dtype=np.uint64)
        order = np.argsort(keys, kind="stable")
        first = np.full(K + 1, NONE, dtype=np.uint64)
        sk = keys[order]
        for j in range(len(sk) - 1, -1, -1):
            first[int(sk[j])] = j
        x.update(keys=keys, lsorted=np.array(starts, dtype=np.uint64)[order], first=first)
    _EXPECT[key] = x
    return x


_TEXTS = {}


def expected_texts(case, name):
    """{"eds", "seds", "stats"} of oracle(split(V, F, name)), or {"error": text}"""
    key = (case["name"].replace("weak/", ""), name)
    if key not in _TEXTS:
        try:
            e, s, st = o.vcf(*cs.split(case["V"], case["F"], name), 0)
            _TEXTS[key] = {"eds": e, "seds": s, "stats": st}
        except o.OracleError as ex:
            _TEXTS[key] = {"error": str(ex)}
    return _TEXTS[key]


def contig_lines(case, name):
    """the lines of V_name (contig_spec.split), without the empty piece behind a final newline"""
    lines = cs.split(case["V"], case["F"], name)[0].split(b"\n")
    return lines[:-1] if lines and lines[-1] == b"" else lines
