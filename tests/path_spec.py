"""Python restatement of the path spelling specification (edsx_paths_spell / EDS::path_sequence / eds2fasta), for well
formed texts.  TEST INFRASTRUCTURE: the comparator of tests/test_paths_*.py, never imported by edsparser_amd/."""
import re


def parse(eds, seds):
    """-> (symbols: list of lists of bytes, sources: one set of ints per string, P).  Whitespace is dropped; text
    outside braces is a single-string symbol (the compact form).  ValueError when the texts do not go together."""
    eds = re.sub(rb"\s", b"", bytes(eds))
    syms = [([m.group(1)] if m.group(1) is not None else m.group(2).split(b","))
            for m in re.finditer(rb"([^{}]+)|\{([^{}]*)\}", eds)]
    sets = [set(int(x) for x in g.split(b",")) for g in re.findall(rb"\{([^{}]*)\}", re.sub(rb"\s", b"", bytes(seds)))]
    if len(sets) != sum(len(s) for s in syms):
        raise ValueError("source count does not match cardinality")
    return syms, sets, (max(max(s) for s in sets) if syms else 0)


def spell(syms, sets, p):
    """-> (sequence, missing) of path p: per symbol the first string whose source set holds p or 0."""
    out, missing, sid = [], 0, 0
    for strings in syms:
        for j, s in enumerate(strings):
            if p in sets[sid + j] or 0 in sets[sid + j]:
                out.append(s)
                break
        else:
            missing += 1
        sid += len(strings)
    return b"".join(out), missing


def record(name, seq, line_width):
    """One FASTA record: header, then lines of line_width characters (0: one line); an empty sequence has no line."""
    w = line_width if line_width else max(len(seq), 1)
    return b">" + name + b"\n" + b"".join(seq[i:i + w] + b"\n" for i in range(0, len(seq), w))


def fasta(eds, seds, paths=None, line_width=60, names=None, prefix=b"path"):
    """-> (FASTA bytes, [missing per record]); paths None or empty: all paths 1..P; ValueError for an id outside 1..P."""
    syms, sets, P = parse(eds, seds)
    paths = list(paths) if paths else list(range(1, P + 1))
    out, miss = [], []
    for k, p in enumerate(paths):
        if p < 1 or p > P:
            raise ValueError("Path id %d out of range (1..%d)" % (p, P))
        seq, m = spell(syms, sets, p)
        out.append(record(names[k] if names else prefix + str(p).encode(), seq, line_width))
        miss.append(m)
    return b"".join(out), miss
