"""Alignments built from a mask of variant columns, for tests/test_msa_spec_*.py: masks that hold every window of
common and variant columns at every phase of the device's 64-column words, rows that copy k haplotypes, and chains of
variant columns and short common runs that an l-EDS merges into one segment."""
import numpy as np

DNA = b"ACGT"
A65 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789*+."     # no byte the .eds / .seds texts use


# ---- masks: 1 = a variant column ----

def de_bruijn(n):
    """The binary de Bruijn sequence B(2, n) as the concatenation of the Lyndon words whose length divides n: 2**n bits,
    every n-bit word once as a cyclic window; it starts with n zeros and ends with n ones."""
    a, seq = [0] * (n + 1), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            if a[t - p] == 0:
                a[t] = 1
                db(t + 1, t)
    db(1, 1)
    return np.array(seq, dtype=np.uint8)


def phased_mask(n):
    """B(2, n) and one spacer column, 64 times, and the first n - 1 columns once more.  The period 2**n + 1 is odd, so
    a window that starts at column p of the period starts at p + j (mod 64) in repetition j: at every phase of the
    64-column words.  The spacer is a variant column like the n columns before it, so the windows 1..10..0 that wrap
    around the end of B(2, n) are there as well (the spacer is one of their ones).  The n - 1 columns at the end let
    the last repetition finish its windows: 64 repetitions alone have n - 1 window starts too few in their last period
    to hold every window at every phase."""
    b = de_bruijn(n)
    period = np.concatenate([b, [1]]).astype(np.uint8)
    return b, np.concatenate([np.tile(period, 64), period[:n - 1]])


def windows_and_phases(mask, n):
    """-> the set of (value of the n-column window, start column mod 64) over every window of the mask."""
    v = np.zeros(len(mask) - n + 1, dtype=np.int64)
    for i in range(n):
        v |= mask[i:len(mask) - n + 1 + i].astype(np.int64) << i
    return set((v * 64 + np.arange(len(v)) % 64).tolist())


def check_mask(n):
    """Both properties of phased_mask(n), computed from the mask itself."""
    b, mask = phased_mask(n)
    assert len(b) == 2 ** n and len(mask) == (2 ** n + 1) * 64 + n - 1
    cyc = np.concatenate([b, b[:n - 1]])
    assert len({cyc[i:i + n].tobytes() for i in range(2 ** n)}) == 2 ** n           # de Bruijn: every word once
    assert len(windows_and_phases(mask, n)) == 2 ** n * 64                           # ... at each of the 64 phases
    return mask


# ---- alignments from a mask ----

def alignment(mask, S, k, alph, seed, gaps=True):
    """-> the S rows (bytes) of an alignment whose variant columns are exactly those of `mask`.  Row r copies one of k
    haplotypes (rows 0..k-1 are the haplotypes themselves, haplotype 0 is the reference row); every other haplotype
    differs from the reference on every variant column.  k <= len(alph): the haplotypes differ from EACH OTHER on
    every variant column too, so every segment has exactly k strings; else their letters are drawn.  With `gaps` the
    last haplotype has a gap on every third column where that column is variant."""
    rng = np.random.default_rng(seed)
    mask = np.asarray(mask, dtype=np.int64)
    L, A = len(mask), len(alph)
    base = rng.integers(0, A, L)
    if k <= A:
        off = np.arange(k)[:, None] * np.ones(L, dtype=np.int64)[None, :]
    else:
        off = 1 + rng.integers(0, A - 1, (k, L))
        off[0] = 0
    cells = np.frombuffer(alph, dtype=np.uint8)[(base[None, :] + off * mask[None, :]) % A]
    if gaps:
        cells[k - 1, (mask == 1) & (np.arange(L) % 3 == 0)] = 0x2D
    haps = [cells[h].tobytes() for h in range(k)]
    pick = list(range(k)) + rng.integers(0, k, S - k).tolist()
    return [haps[h] for h in pick]


def fasta(rows, lw=None):
    out = []
    for i, r in enumerate(rows):
        out.append(b">row%d" % i)
        w = lw or len(r)
        out.extend(r[j:j + w] for j in range(0, len(r), w))
    return b"\n".join(out) + b"\n"


def alphabet(k):
    return DNA if k <= 4 else b"ACGTN" if k == 5 else A65


# ---- merged segments at the kernels' limits ----

def chain(width, nvar, l):
    """A mask of `width` columns that an l-EDS makes ONE segment: nvar variant columns, the first and the last column
    among them, and between them common runs of fewer than l columns (filled from the left)."""
    spare = width - nvar
    assert nvar >= 2 and 0 <= spare <= (nvar - 1) * (l - 1), (width, nvar, l)
    m = []
    for _ in range(nvar - 1):
        g = min(l - 1, spare)
        spare -= g
        m += [1] + [0] * g
    return m + [1]


def chain_of(nvar, l):
    """... with nvar variant columns and common runs of l - 1, 1, 0, l - 1, 1, 0, ... columns between them."""
    m = []
    for i in range(nvar - 1):
        m += [1] + [0] * (l - 1, 1, 0)[i % 3]
    return m + [1]


def chains(l):
    """The chains at the limits: 511 / 512 / 513 columns wide (STAGE_WMAX) with the fewest variant columns that can
    hold them together and with 300; 63 / 64 / 65 (STAGE_COLS) and 15 / 16 / 17 (RL_MAXCOLS) variant columns."""
    out = []
    for w in (511, 512, 513):
        out.append(chain(w, -(-(w - 1) // l) + 1, l))
        out.append(chain(w, 300, l))
    for v in (63, 64, 65, 15, 16, 17):
        out.append(chain_of(v, l))
        out.append(chain(2 * v - 1 if l == 2 else 4 * v - 3, v, l))
    return out
