"""Seeded synthetic VCF + FASTA inputs of the VCF tests (no oracle imports: also used by profiles/): BASELINE configs[3]'s
shape, the random files of the parity tests, and the constructed files of the device tokeniser's edge tests."""
import random


def gen_vcf(Lf, nrec, ns, seed):
    import random
    rng = random.Random(seed)
    seq = "".join(rng.choices("ACGT", k=Lf))
    fasta = ">chr1 synthetic\n" + "\n".join(seq[i:i + 60] for i in range(0, Lf, 60)) + "\n"
    pos = sorted(rng.sample(range(1, Lf - 12), nrec))
    out = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("s%d" % i for i in range(ns))]
    for p in pos:
        r = rng.random()
        base = seq[p - 1]
        if r < 0.7:
            ref, alt = base, rng.choice([b for b in "ACGT" if b != base])
        elif r < 0.85:
            ref, alt = base, base + "".join(rng.choices("ACGT", k=rng.randint(1, 10)))
        else:
            d = rng.randint(1, 10)
            ref, alt = seq[p - 1:p + d], base
        gts = "\t".join("%d|%d" % (rng.random() < 0.3, rng.random() < 0.3) for _ in range(ns))
        out.append("chr1\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT\t%s" % (p, ref, alt, gts))
    return ("\n".join(out) + "\n").encode(), fasta.encode()


def random_vcf(rng, L, nvar, ns, lw):
    ref = "".join(rng.choice("ACGT") for _ in range(L))
    fasta = ">chr1 synthetic\n" + "\n".join(ref[i:i + lw] for i in range(0, L, lw)) + "\n"
    pos = sorted(rng.sample(range(1, L + 1), nvar))
    lines = ["##fileformat=VCFv4.2", "\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] +
                                                ["S%d" % i for i in range(ns)])]
    for p in pos:
        x = rng.random()
        if x < 0.7:
            r = ref[p - 1]
            alts = [rng.choice([b for b in "ACGT" if b != r])]
            if rng.random() < 0.1:
                alts.append(rng.choice("ACGT"))
        elif x < 0.85:
            r = ref[p - 1]
            alts = [r + "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 10)))]
        else:
            r = ref[p - 1:p + rng.randint(1, 10)]
            alts = [r[0]]
        gts = ["|".join(str(rng.randint(0, len(alts)) if rng.random() < 0.3 else 0) for _ in range(2)) for _ in range(ns)]
        lines.append("\t".join(["chr1", str(p), ".", r, ",".join(alts), ".", "PASS", ".", "GT"] + gts))
    return ("\n".join(lines) + "\n").encode(), fasta.encode()


def records_vcf(ref, recs, ns, lw=60, shuffle=None):
    fasta = ">chr1 synthetic\n" + "\n".join(ref[i:i + lw] for i in range(0, len(ref), lw)) + "\n"
    lines = ["##fileformat=VCFv4.2", "\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] +
                                                ["S%d" % i for i in range(ns)])]
    body = ["\t".join(["chr1", str(p), ".", r, a, ".", "PASS", ".", "GT"] + g) for p, r, a, g in recs]
    if shuffle is not None:
        shuffle.shuffle(body)
    return ("\n".join(lines + body) + "\n").encode(), fasta.encode()


def random_records(rng, ref, n, ns, dup_frac=0.0):
    L = len(ref)
    pos = sorted(rng.sample(range(1, L + 1), n))
    if dup_frac:
        pos = sorted(p if rng.random() > dup_frac else rng.choice(pos) for p in pos)
    recs = []
    for p in pos:
        x = rng.random()
        if x < 0.6:
            r, alts = ref[p - 1], rng.choice("ACGT")
        elif x < 0.8:
            r = ref[p - 1]
            alts = r + "".join(rng.choice("ACGT") for _ in range(rng.randint(1, 6)))
        else:
            r = ref[p - 1:p + rng.randint(1, 12)]
            alts = r[0] + "," + "<DEL>"
        na = alts.count(",") + 1
        recs.append((p, r, alts, ["|".join(str(rng.randint(0, na)) for _ in range(2)) for _ in range(ns)]))
    return recs


def shuffled(rng, vcf, dup=False):
    """the same file with its record lines in random order; dup: half of them a second time"""
    lines = vcf.decode().split("\n")
    head, body = lines[:2], [x for x in lines[2:] if x]
    if dup:
        body += [rng.choice(body) for _ in range(len(body) // 2)]
    rng.shuffle(body)
    return ("\n".join(head + body) + "\n").encode()


def single_damage_files(rng):
    """One oddity per small file (tests/test_vcf_gpu.py::test_device_tokeniser_single_damage_per_file): yields
    (kind, choice, samples, tail, damaged line, vcf, fasta)."""
    gts = ["./.", ".", "1", "0/1/2", "x|1", "1|", "|", "0|1:9:x", ":", "99999999999|0", "0|1\r", "+1|0", " 1|0", "01|1", "1x|0", "|1", "0||1", "0/1|1"]
    alts = ["<DEL>", "<INS>", "<INV>", "A,<DEL>", "<DUP>,C", ",", "A,,C", "C,", "<>", "<", ".", "*", "<DEL>,<INS>", "ACGTACGT", "<DELX>", "<del>"]
    poss = ["0", "-5", "+7", " 12", "12abc", "abc", "99999999999999999999999", "18446744073709551615", "0012", "1", "3000"]
    wholes = ["", "#junk", "chr1", "\t\t\t", "chr1\t12\t.\tA", "chr1 14 . A G . PASS . GT 0|1 1|1", "chr1\t15\t.\tA\tG", "chr1\t16\t.\tA\tG\t.\tPASS\t.\tGT",
              "\tchr1\t17\t.\tA\tG\t.\tPASS\t.\tGT\t0|1\t0|0", "chr1\t18\t.\tA\tG\t.\tPASS\t.\tGT\t0|1\t", "chr1\t19\t.\tA\tG\t\t.\tPASS\t.\tGT\t0|1"]
    for kind, choices in (("gt", gts), ("alt", alts), ("pos", poss), ("line", wholes), ("cr", ["\r"]), ("tabs", ["x"])):
        for ch in choices:
            for ns in (0, 2):
                vcf, fasta = random_vcf(rng, 3000, 25, ns, 60)
                lines = vcf.decode().split("\n")
                i = rng.randrange(2, len(lines) - 1)
                f = lines[i].split("\t")
                if kind == "gt":
                    if ns == 0:
                        continue
                    f[9 + rng.randrange(ns)] = ch
                    lines[i] = "\t".join(f)
                elif kind == "alt":
                    f[4] = ch
                    lines[i] = "\t".join(f)
                elif kind == "pos":
                    f[1] = ch
                    lines[i] = "\t".join(f)
                elif kind == "line":
                    lines.insert(i, ch)
                elif kind == "cr":
                    lines[i] += "\r"
                else:
                    lines[i] = lines[i].replace("\t", "\t\t", 1)
                for tail in ("\n", ""):
                    yield kind, ch, ns, tail, lines[i], ("\n".join(lines[:-1]) + tail).encode(), fasta


def text_length_files(rng):
    """The texts of tests/test_vcf_gpu.py::test_text_length_every_remainder_mod_8_with_and_without_final_newline: a comment
    line of adjustable length in front, last record with a long ALT, an <INS> and a <DEL>.  Returns (fasta, mod8, sized):
    mod8 = [(tail, pad, nl, vcf)] with every text length modulo 8 with and without the final newline; sized = [(target, vcf)]
    with lengths just below / at / above multiples of 256."""
    base_vcf, fasta = random_vcf(rng, 2000, 60, 4, 60)
    lines = base_vcf.decode().split("\n")
    head, body = lines[:2], [x for x in lines[2:] if x]
    ref = "".join(fasta.decode().split("\n")[1:])
    last_pos = 1990
    tails = [
        "chr1\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT\t0|1\t1|1\t0|0\t1|0" % (last_pos, ref[last_pos - 1], ref[last_pos - 1] + "ACGTACGTAC"),
        "chr1\t%d\t.\t%s\t<INS>\t.\tPASS\t.\tGT\t0|1\t1|1\t0|0\t1|0" % (last_pos, ref[last_pos - 1:last_pos + 4]),
        "chr1\t%d\t.\t%s\t<DEL>\t.\tPASS\t.\tGT\t0|1\t1|1\t0|0\t1|0" % (last_pos, ref[last_pos - 1:last_pos + 2]),
    ]
    body = [b for b in body if int(b.split("\t")[1]) < last_pos - 12]
    mod8 = []
    for tail in tails:
        for pad in range(0, 8):
            for nl in ("\n", ""):
                mod8.append((tail, pad, nl, ("\n".join([head[0], "##pad=" + "x" * pad, head[1]] + body + [tail]) + nl).encode()))
    sized = []
    for target in (255, 256, 257, 511, 512, 513, 4095, 4096, 4097):
        for k in (3, 0):                                          # (the shortest lengths have room for the last record only)
            stem = "\n".join([head[0], head[1]] + body[:k] + [tails[0]])
            padn = target - len(stem) - len("##pad=\n")
            if padn >= 0:
                break
        vcf = ("\n".join([head[0], "##pad=" + "x" * padn, head[1]] + body[:k] + [tails[0]])).encode()
        assert len(vcf) == target
        sized.append((target, vcf))
    return fasta, mod8, sized


def large_key_vcf(rng, n, ns=2):
    """n records with pairwise distinct POS in random order; a quarter of them carry positions of 8 to 19 digits (at most
    9 * 10^18, far beyond the reference: accepted input), so that every byte of a 64-bit sort key is non-zero somewhere."""
    ref = "".join(rng.choices("ACGT", k=max(3000, 4 * n)))
    recs = random_records(rng, ref, n, ns)
    used = set()
    for i in range(0, n, 4):
        while True:
            d = rng.randint(8, 19)
            p = rng.randrange(10 ** (d - 1), min(10 ** d, 9 * 10 ** 18 + 1))
            if p not in used:
                break
        used.add(p)
        recs[i] = (p, "A", "C" + "".join(rng.choices("ACGT", k=rng.randint(0, 5))), recs[i][3])     # (distinct texts: their order shows)
    return records_vcf(ref, recs, ns, shuffle=rng)
