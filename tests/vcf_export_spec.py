"""Python restatement of the VCF export specification (edsx_eds_vcf / eds2vcf, include/edsx.h), by brute force, for well
formed texts.  TEST INFRASTRUCTURE: the comparator of tests/test_vcf_export_*.py, never imported by edsparser_amd/.

The documented example, {AGCT}{T,C}{AG}{G,}{TA} with the sets {0}{1,2}{3}{0}{1}{2,3}{0}:
    reference (first strings)  AGCT T AG G TA  =  AGCTTAGGTA, refpos = 0 4 5 7 8
    symbol 1 {T,C}: no empty string, POS = refpos + 1 = 5, alleles verbatim;   paths 1, 2 take T (0), path 3 takes C (1)
    symbol 3 {G,}:  anchored, base at refpos - 1 = 6 is 'G', POS = 7, GG / G;  path 1 takes G (0), paths 2, 3 the empty one
    eds  5  .  T   C  .  .  .  GT  0  0  1
    eds  7  .  GG  G  .  .  .  GT  0  1  1
"""
import re

import path_spec as ps

TILE_PATHS = 256          # path ids [256 t, 256 t + 256) share a workgroup of the cell kernels (csrc/vcf_text.hpp)
STAGE = 4096              # bytes of cell text a workgroup stages in LDS; more is written by bytes


def parse(eds, seds=None):
    """-> (symbols, sets or None, P)"""
    if seds is not None:
        return ps.parse(eds, seds)
    eds = re.sub(rb"\s", b"", bytes(eds))
    syms = [([m.group(1)] if m.group(1) is not None else m.group(2).split(b","))
            for m in re.finditer(rb"([^{}]+)|\{([^{}]*)\}", eds)]
    return syms, None, 0


def export(eds, seds=None, chrom=b"eds", ref_path=0, names=None, prefix=b"path", line_width=60, max_bytes=0):
    """-> (vcf, fasta, info).  ValueError with the library's text for what it refuses."""
    if not chrom or re.search(rb"\s", chrom):
        raise ValueError("Chromosome name is empty or holds whitespace")
    if ref_path and seds is None:
        raise ValueError("A reference path needs sources (.seds)")
    syms, sets, P = parse(eds, seds)
    if ref_path > P:
        raise ValueError("Path id %d out of range (1..%d)" % (ref_path, P))
    # reference strings
    first, sid = [], 0
    for strings in syms:
        first.append(sid)
        sid += len(strings)
    takes = lambda j, p: p in sets[j] or 0 in sets[j]
    ridx = []
    for i, strings in enumerate(syms):
        r = 0
        if ref_path:
            r = next((j for j in range(len(strings)) if takes(first[i] + j, ref_path)), None)
            if r is None:
                raise ValueError("Path %d takes no string of symbol %d" % (ref_path, i))
        ridx.append(r)
    refs = [strings[r] for strings, r in zip(syms, ridx)]
    ref = b"".join(refs)
    L = len(ref)
    refpos = [0]
    for s in refs:
        refpos.append(refpos[-1] + len(s))
    # records
    lines, anchored, overlapping, prev_end = [], 0, 0, 0
    for i, strings in enumerate(syms):
        if len(strings) < 2:
            continue
        r = ridx[i]
        order = [r] + [j for j in range(len(strings)) if j != r]
        alleles = [strings[j] for j in order]
        if any(len(s) == 0 for s in strings):
            if refpos[i] > 0:
                base = ref[refpos[i] - 1:refpos[i]]
                alleles, pos = [base + a for a in alleles], refpos[i]
            else:
                q = refpos[i + 1]
                if q >= L:
                    raise ValueError("Symbol %d has an empty string and no reference base to anchor it" % i)
                alleles, pos = [a + ref[q:q + 1] for a in alleles], 1
            anchored += 1
        else:
            pos = refpos[i] + 1
        if lines and pos <= prev_end:
            overlapping += 1
        prev_end = pos + len(alleles[0]) - 1
        line = b"\t".join([chrom, b"%d" % pos, b".", alleles[0], b",".join(alleles[1:]), b".", b".", b"."])
        if sets is not None:
            line += b"\tGT"
            for p in range(1, P + 1):
                got = [b"%d" % a for a, j in enumerate(order) if takes(first[i] + j, p)]
                line += b"\t" + (b"/".join(got) if got else b".")
        lines.append(line + b"\n")
    body = b"".join(lines)
    # header
    if names is not None and len(names) != P:
        raise ValueError("Expected %d sample names, got %d" % (P, len(names)))
    head = b"##fileformat=VCFv4.2\n##source=eds2vcf\n##contig=<ID=%s,length=%d>\n" % (chrom, L)
    cols = [b"#CHROM", b"POS", b"ID", b"REF", b"ALT", b"QUAL", b"FILTER", b"INFO"]
    if sets is not None:
        head += b"##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
        cols.append(b"FORMAT")
        for p in range(1, P + 1):
            name = names[p - 1] if names is not None else prefix + b"%d" % p
            if not name or b"\t" in name or b"\n" in name:
                raise ValueError("Sample name %d is not a VCF sample name" % (p - 1))
            cols.append(name)
    head += b"\t".join(cols) + b"\n"
    info = dict(symbols=len(syms), strings=sum(len(s) for s in syms), paths=P, records=len(lines), anchored=anchored,
                overlapping=overlapping, ref_length=L, header_bytes=len(head), body_bytes=len(body))
    if max_bytes and len(body) > max_bytes:
        raise ValueError("VCF body of %d bytes is above the limit of %d" % (len(body), max_bytes))
    return head + body, ps.record(chrom, ref, line_width), info


# ---- reading it back (what a consumer does) --------------------------------------------------------------------------------
def read(vcf):
    """-> (sample names, [(pos, ref, [alts], [cell per sample])]); cells as lists of allele numbers, [] for '.'"""
    names, recs = [], []
    for line in bytes(vcf).split(b"\n"):
        if not line or line.startswith(b"##"):
            continue
        f = line.split(b"\t")
        if line.startswith(b"#"):
            names = f[9:]
            continue
        cells = [[] if c == b"." else [int(x) for x in re.split(rb"[/|]", c)] for c in f[9:]]
        recs.append((int(f[1]), f[3], f[4].split(b","), cells))
    return names, recs


def fasta_sequence(fasta):
    return b"".join(bytes(fasta).split(b"\n")[1:])


def apply_sample(ref, recs, s):
    """The sequence of haploid sample s (0-based): every record's REF - the anchor base is part of it - replaced by the one
    allele of the sample's cell.  The records must not overlap."""
    out, at = [], 0
    for pos, r, alts, cells in recs:
        assert len(cells[s]) == 1, (pos, cells[s])
        assert pos - 1 >= at and ref[pos - 1:pos - 1 + len(r)] == r, pos
        out.append(ref[at:pos - 1])
        out.append(([r] + alts)[cells[s][0]])
        at = pos - 1 + len(r)
    out.append(ref[at:])
    return b"".join(out)
