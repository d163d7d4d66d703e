"""The specification of contig selection (edsx_vcf_session_*, vcf2eds --chrom / --all-chroms), by reduction to the
transform that exists: split(V, F, c) -> (V_c, F_c), and the result for contig c is edsx_vcf_transform(V_c, F_c, l).

compose() builds multi-contig inputs out of single-contig fixtures whose expected results came from the reference, so
the fixtures are the answer key: contig k of the combined input must give fixture k's `expect`."""
import random

NAMES = [b"chr1", b"chr10", b"chr1_alt", b"21", b"X", b"HLA-A*01:01", b"chr2", b"c"]      # prefix relations on purpose


def first_token(line):
    t = line.split()          # bytes.split(): ASCII whitespace, what operator>> skips
    return t[0] if t else None


def is_record_line(line):
    return line != b"" and line[:1] != b"#"


def fasta_records(f):
    """[(name, start, end)]: a record starts at a '>' that is byte 0 or follows '\\n'"""
    starts = [0] if f[:1] == b">" else []
    i = f.find(b"\n>")
    while i >= 0:
        starts.append(i + 1)
        i = f.find(b"\n>", i + 1)
    recs = []
    for k, s in enumerate(starts):
        e = starts[k + 1] if k + 1 < len(starts) else len(f)
        nl = f.find(b"\n", s, e)
        hdr = f[s:nl if nl >= 0 else e]
        sp = hdr.find(b" ")
        recs.append((hdr[1:sp] if sp >= 0 else hdr[1:], s, e))
    return recs


def fasta_metadata(f, s, e):
    """(seq_start, line_width, seq_size) of the record f[s:e] as parse_fasta_metadata (vcf_transforms.cpp:51-86) finds them,
    as offsets into f; a record without a sequence line: (e, 0, 0)"""
    nl = f.find(b"\n", s, e)
    if nl < 0:
        return e, 0, 0
    ss = nl + 1
    nl2 = f.find(b"\n", ss, e)
    lw = (nl2 if nl2 >= 0 else e) - ss
    return ss, lw, (e - ss) - f.count(b"\n", ss, e)


def split(vcf, fasta, name):
    recs = [r for r in fasta_records(fasta) if r[0] == name]
    if not recs:
        raise KeyError(name)
    fc = fasta[recs[0][1]:recs[0][2]]
    out = []
    for ln in vcf.split(b"\n"):
        if not is_record_line(ln) or first_token(ln) == name:
            out.append(ln)
    return b"\n".join(out), fc


def rename(vcf, fasta, name):
    """the single-contig input (vcf, fasta) with its contig called `name`; None: it cannot be renamed"""
    lines = []
    for ln in vcf.split(b"\n"):
        if not is_record_line(ln):
            lines.append(ln)
            continue
        t = first_token(ln)
        if t is None:
            return None
        i = ln.find(t)
        lines.append(ln[:i] + name + ln[i + len(t):])
    recs = fasta_records(fasta)
    if not recs or recs[0][1] != 0:
        return None
    fo = b""
    for k, (nm, s, e) in enumerate(recs):
        body = fasta[s:e]
        nn = name if k == 0 else name + b"_x%d" % k
        fo += b">" + nn + body[1 + len(nm):]
    if not fo.endswith(b"\n"):
        fo += b"\n"
    return b"\n".join(lines), fo


def compose(cases, seed, names=NAMES):
    """Fixtures combined len(names) at a time.  Yields (V, F, [(name, case)], left_out): one VCF with the '#' lines of all
    parts in front and their record lines interleaved at random (order kept inside a contig), one FASTA with the records
    in another order."""
    rng = random.Random(seed)
    idx = list(range(len(cases)))
    rng.shuffle(idx)
    for g in range(0, len(idx), len(names)):
        parts, left = [], []
        for j, ci in enumerate(idx[g:g + len(names)]):
            c = cases[ci]
            r = rename(c["vcf"].encode(), c["fasta"].encode(), names[j])
            if r is None:
                left.append(c)
            else:
                parts.append((names[j], c, r))
        heads, per = [], {}
        for nm, c, (v, f) in parts:
            per[nm] = []
            for ln in v.split(b"\n"):
                if ln == b"":
                    continue
                (heads if ln[:1] == b"#" else per[nm]).append(ln)
        merged = []
        live = [nm for nm in per if per[nm]]
        while live:
            nm = rng.choice(live)
            merged.append(per[nm].pop(0))
            if not per[nm]:
                live.remove(nm)
        V = b"".join(ln + b"\n" for ln in heads) + b"\n".join(merged) + b"\n"
        order = parts[:]
        rng.shuffle(order)
        F = b"".join(f for _, _, (v, f) in order)
        yield V, F, [(nm, c) for nm, c, _ in parts], left


def load_fixtures(golden_dir):
    import json
    import os
    cases = []
    for fn in ("gen_vcf.json", "gen2_vcf.json"):
        cases += json.load(open(os.path.join(golden_dir, fn)))["cases"]
    return cases
