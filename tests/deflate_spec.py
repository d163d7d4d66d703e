"""DEFLATE test vectors that no real encoder writes: a pure-Python assembler of raw DEFLATE streams (RFC 1951) from token
lists and explicit code lengths, and the corpora built with it - directed valid streams, seeded random valid streams and
hand-made streams that must be refused.  The reference is zlib / gzip of the Python that runs the test, nothing else:
every accepted stream inflates through zlib to the text its token lists spell, every refused member makes
gzip.decompress raise (asserted where the corpora are generated).

A stream is a list of blocks:
    ("stored", data[, {"nlen": n}])
    ("fixed", tokens[, {"eob": False}])
    ("dynamic", tokens, {"ll": [...], "dl": [...]  [, "cl": 19 lengths, "rle": [...], "hclen": n, "hlit": n, "hdist": n, "eob": False]})
    ("bits", [(value, nbits), ...])                        anything at all, after the BFINAL bit
A token is a literal byte (int), a match (length, distance), or a bare symbol ("L", symbol, extra) / ("D", symbol, extra).
"rle" is the code-length sequence: a length 0..15, or (16 | 17 | 18, repeat count).
"""
import bisect
import functools
import gzip
import random
import struct
import zlib

import bgzf_spec as bz

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
         12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 32
WINDOW = 32768
FAR = WINDOW - 262                    # zlib's encoder never reaches further back than this
BATCH_EDGE = WINDOW - 4096            # distances above this can end a device batch early


def length_code(length):
    """(symbol, extra value) of a match length; 258 is symbol 285."""
    if length == 258:
        return 285, 0
    i = bisect.bisect_right(LBASE, length) - 1
    return 257 + i, length - LBASE[i]


def dist_code(dist):
    i = bisect.bisect_right(DBASE, dist) - 1
    return i, dist - DBASE[i]


# ---- bits and codes ---------------------------------------------------------------------------------------------
class BitWriter:
    """LSB first; Huffman codes go in most significant bit first, that is bit-reversed."""

    def __init__(self):
        self.out, self.acc, self.n, self.nbits = bytearray(), 0, 0, 0

    def bits(self, value, k):
        assert 0 <= value < (1 << k) or k == 0 and value == 0
        self.acc |= value << self.n
        self.n += k
        self.nbits += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        self.bits(int(format(code & ((1 << length) - 1), "0%db" % length)[::-1], 2), length)

    def align(self):
        pad = -self.n % 8
        self.bits(0, pad)
        return pad

    def raw(self, data):
        assert self.n == 0
        self.out += data
        self.nbits += 8 * len(data)

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lens):
    """The canonical code of every symbol (RFC 1951 3.2.2), None where the length is 0.  An over-subscribed set gets
    codes that overflow their length; BitWriter.code masks them."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    codes = []
    for l in lens:
        codes.append(nxt[l] if l else None)
        nxt[l] += 1 if l else 0
    return codes


def kraft(lens):
    """Sum of 2^-l in units of 2^-15: 32768 is a complete code."""
    return sum(1 << (15 - l) for l in lens if l)


def complete_lengths(k, limit, rng=None):
    """k code lengths (k >= 2) of a complete code: a leaf is split until there are k - the shallowest without rng, a random
    one below the limit with it."""
    assert 2 <= k <= (1 << limit)
    leaves = [1, 1]
    while len(leaves) < k:
        if rng is None:
            i = leaves.index(min(leaves))
        else:
            i = rng.choice([j for j, d in enumerate(leaves) if d < limit])
        d = leaves.pop(i)
        leaves += [d + 1, d + 1]
    return leaves


def lengths_for(symbols, size, limit=15, rng=None):
    """`size` code lengths, complete over `symbols` (one symbol: length 1; none: all zero)."""
    symbols = sorted(set(symbols))
    lens = [0] * size
    if len(symbols) == 1:
        lens[symbols[0]] = 1
    elif symbols:
        ls = complete_lengths(len(symbols), limit, rng)
        if rng:
            rng.shuffle(ls)
        for s, l in zip(symbols, ls):
            lens[s] = l
    return lens


def used_symbols(tokens):
    ll, dd = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            ll.add(t)
        elif t[0] == "L":
            ll.add(t[1])
        elif t[0] == "D":
            dd.add(t[1])
        else:
            ll.add(length_code(t[0])[0])
            dd.add(dist_code(t[1])[0])
    return ll, dd


def auto_codes(tokens, nlen=None, ndist=None):
    """{"ll", "dl"} of a balanced complete code over exactly the symbols the tokens use."""
    ll, dd = used_symbols(tokens)
    return {"ll": lengths_for(ll, nlen or max(257, max(ll) + 1)), "dl": lengths_for(dd, ndist or max(1, max(dd, default=0) + 1))}


def rle_plain(seq):
    return list(seq)


def rle_greedy(seq):
    """The longest repeat code at every position."""
    out, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        if v == 0 and run >= 3:
            rep = min(run, 138)
            out.append((18 if rep >= 11 else 17, rep))
        elif v and i and seq[i - 1] == v and run >= 3:
            rep = min(run, 6)
            out.append((16, rep))
        else:
            rep = 1
            out.append(v)
        i += rep
    return out


def rle_symbols(rle):
    return [t if isinstance(t, int) else t[0] for t in rle]


def rle_total(rle):
    return sum(1 if isinstance(t, int) else t[1] for t in rle)


def default_cl(rle):
    used = set(rle_symbols(rle))
    if len(used) == 1:
        used.add(0 if 0 not in used else 1)            # zlib wants the code-length code complete
    return lengths_for(used, 19, 7)


# ---- block writers ----------------------------------------------------------------------------------------------
def put_symbol(w, codes, lens, s):
    assert s < len(lens) and lens[s], "symbol %d has no code" % s
    w.code(codes[s], lens[s])


def put_tokens(w, tokens, ll, dl, eob=True):
    lc, dc = canonical(ll), canonical(dl)
    for t in tokens:
        if isinstance(t, int):
            put_symbol(w, lc, ll, t)
        elif t[0] == "L":
            put_symbol(w, lc, ll, t[1])
            w.bits(t[2], LEXT[t[1] - 257] if 257 <= t[1] <= 285 else 0)
        elif t[0] == "D":
            put_symbol(w, dc, dl, t[1])
            w.bits(t[2], DEXT[t[1]] if t[1] < 30 else 0)
        else:
            s, e = length_code(t[0])
            put_symbol(w, lc, ll, s)
            w.bits(e, LEXT[s - 257])
            s, e = dist_code(t[1])
            put_symbol(w, dc, dl, s)
            w.bits(e, DEXT[s])
    if eob:
        put_symbol(w, lc, ll, 256)


def put_stored(w, data, final, nlen=None):
    w.bits(final, 1)
    w.bits(0, 2)
    w.align()
    w.bits(len(data), 16)
    w.bits((len(data) ^ 0xffff) if nlen is None else nlen, 16)
    w.raw(data)


def put_fixed(w, tokens, final, eob=True):
    w.bits(final, 1)
    w.bits(1, 2)
    put_tokens(w, tokens, FIXED_LL, FIXED_DL, eob)


def put_dynamic(w, tokens, final, ll, dl, cl=None, rle=None, hclen=None, hlit=None, hdist=None, eob=True):
    rle = rle_greedy(ll + dl) if rle is None else rle
    cl = default_cl(rle) if cl is None else cl
    if hclen is None:
        hclen = max(4, 1 + max(i for i in range(19) if cl[CL_ORDER[i]]))
    assert all(cl[CL_ORDER[i]] == 0 for i in range(hclen, 19))
    w.bits(final, 1)
    w.bits(2, 2)
    w.bits(len(ll) - 257 if hlit is None else hlit, 5)
    w.bits(len(dl) - 1 if hdist is None else hdist, 5)
    w.bits(hclen - 4, 4)
    for i in range(hclen):
        w.bits(cl[CL_ORDER[i]], 3)
    cc = canonical(cl)
    for t in rle:
        s = t if isinstance(t, int) else t[0]
        put_symbol(w, cc, cl, s)
        if s == 16:
            w.bits(t[1] - 3, 2)
        elif s == 17:
            w.bits(t[1] - 3, 3)
        elif s == 18:
            w.bits(t[1] - 11, 7)
    put_tokens(w, tokens, ll, dl, eob)


def assemble(blocks, info=None):
    """The raw stream of a block list; BFINAL on the last block.  info (a dict) receives "bits" and "pad"."""
    w = BitWriter()
    for i, b in enumerate(blocks):
        final = 1 if i == len(blocks) - 1 else 0
        opts = dict(b[2]) if len(b) > 2 else {}
        if b[0] == "stored":
            put_stored(w, b[1], final, **opts)
        elif b[0] == "fixed":
            put_fixed(w, b[1], final, **opts)
        elif b[0] == "dynamic":
            put_dynamic(w, b[1], final, **opts)
        else:
            w.bits(final, 1)
            for v, k in b[1]:
                w.bits(v, k)
    if info is not None:
        info["bits"] = w.nbits
        info["pad"] = -w.nbits % 8
    return w.getvalue()


def walk(blocks):
    """(position, token) of every literal and match, stored bytes as literals; positions count from the stream's start."""
    pos = 0
    for b in blocks:
        if b[0] == "stored":
            yield pos, b[1]
            pos += len(b[1])
            continue
        for t in b[1]:
            yield pos, t
            pos += 1 if isinstance(t, int) else t[0]


def expand(blocks):
    """The text a block list spells, from its tokens alone."""
    out = bytearray()
    for _, t in walk(blocks):
        if isinstance(t, int):
            out.append(t)
        elif isinstance(t, (bytes, bytearray)):
            out += t
        else:
            copy_match(out, t[0], t[1])
    return bytes(out)


def copy_match(out, length, dist):
    assert isinstance(length, int) and 3 <= length <= 258 and 1 <= dist <= min(len(out), WINDOW), (length, dist, len(out))
    if dist >= length:
        out += out[len(out) - dist:len(out) - dist + length]
    else:
        unit = bytes(out[-dist:])
        out += (unit * (length // dist + 1))[:length]


def wrap(raw, text, isize=None, crc=None):
    """One BGZF member around a raw stream."""
    size = 18 + len(raw) + 8
    assert size <= 65536, "the member does not fit BSIZE"
    head = struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, 66, 67, 2, size - 1)
    return head + raw + struct.pack("<II", zlib.crc32(text) & 0xffffffff if crc is None else crc, len(text) if isize is None else isize)


def gzip_wrap(raw, text):
    """One plain gzip member around a raw stream."""
    return struct.pack("<BBBBIBB", 0x1f, 0x8b, 8, 0, 0, 0, 0xff) + raw + struct.pack("<II", zlib.crc32(text) & 0xffffffff, len(text) & 0xffffffff)


def accepted(name, blocks, out):
    """Appends (name, blocks, raw, text) after zlib has agreed with the token lists."""
    raw, text = assemble(blocks), expand(blocks)
    try:
        got = zlib.decompress(raw, -15)
    except zlib.error as e:
        raise AssertionError("%s: zlib refuses it: %s (the test module is wrong)" % (name, e))
    assert got == text, "%s: zlib disagrees with the token list (the test module is wrong)" % name
    out.append((name, blocks, raw, text))


# ---- texts ------------------------------------------------------------------------------------------------------
def noise(n, seed):
    return random.Random(seed).randbytes(n)


def periodic_tokens(n, unit):
    """n bytes of `unit` repeated: the unit as literals, the rest as matches one period back."""
    p = len(unit)
    toks = list(unit[:min(n, p)])
    left = n - len(toks)
    while left >= 3:
        l = min(left, 258)
        if left - l in (1, 2):
            l -= 3
        toks.append((l, p))
        left -= l
    assert left == 0 or n < p + 3
    text = (unit * (n // p + 2))[:n]
    toks += list(text[n - left:]) if left else []
    return toks


# ---- directed valid streams -------------------------------------------------------------------------------------
FAR_DISTANCES = (WINDOW, WINDOW - 1, FAR + 1, BATCH_EDGE + 1, BATCH_EDGE - 1)
FAR_LENGTHS = (3, 64, 65, 257, 258)
FAR_LEADS = (0, 1, 255, 256, 300)


def _dyn(tokens, **over):
    opts = auto_codes(tokens)
    opts.update(over)
    return ("dynamic", tokens, opts)


@functools.lru_cache(maxsize=None)
def directed():
    """[(name, blocks, raw, text)]"""
    out = []
    lits = list(b"ACGTNacgtn\tchr1\n0|1.PASS")

    # -- degenerate codes
    accepted("dist_empty_hdist0", [("dynamic", lits, {"ll": auto_codes(lits)["ll"], "dl": [0]})], out)
    accepted("dist_empty_hdist29", [("dynamic", lits, {"ll": auto_codes(lits)["ll"], "dl": [0] * 30})], out)
    for name, blocks in (("dist_empty_hdist0", out[-2][1]), ("dist_empty_hdist29", out[-1][1])):
        assert not any(blocks[0][2]["dl"]) and all(isinstance(t, int) for t in blocks[0][1])
    toks = lits + [(10, 4), (258, 4), (3, 4)]
    b = _dyn(toks)
    assert [l for l in b[2]["dl"] if l] == [1] and b[2]["dl"][3] == 1
    accepted("dist_single_length1_used", [b], out)
    b = ("dynamic", [], {"ll": [0] * 256 + [1], "dl": [0]})
    accepted("lit_only_eob_length1", [b], out)
    accepted("lit_only_eob_length1_twice_then_text", [b, b, _dyn(lits)], out)

    # -- far matches behind 32 768 stored bytes
    back = noise(WINDOW, 40)
    for d in FAR_DISTANCES:
        for l in FAR_LENGTHS:
            for lead in FAR_LEADS:
                toks = [(65 + i % 26) for i in range(lead)] + [(l, d)]
                blk = ("fixed", toks) if (l + lead) % 2 else _dyn(toks)
                blocks = [("stored", back), blk]
                pos, t = list(walk(blocks))[-1]
                assert t == (l, d) and pos == WINDOW + lead and d > BATCH_EDGE - 2
                accepted("far/d%d_l%d_after%d" % (d, l, lead), blocks, out)
    for name, toks in (("far/two_at_window", [(258, WINDOW), (258, WINDOW)]), ("far/two_mixed", [(64, WINDOW - 1), (65, FAR + 1)]),
                       ("far/three_descending", [(258, WINDOW), (257, WINDOW - 1), (3, WINDOW - 2)]),
                       # literals behind a far match until the match's ring limit ends the batch (100 bytes behind its start)
                       ("far/literals_to_ring_limit", [(3, WINDOW - 100)] + [66 + i % 50 for i in range(255)]),
                       # ... until the token limit of a batch, and until its byte limit (matches of 258 at distance 1)
                       ("far/literals_to_token_limit", [(258, BATCH_EDGE + 1)] + [66 + i % 50 for i in range(600)]),
                       ("far/matches_to_byte_limit", [(3, BATCH_EDGE + 1)] + [(258, 1)] * 20 + [67] * 40 + [(258, FAR + 1)] + [(258, 1)] * 20),
                       ("far/every_token_far", [(3 + i % 256, WINDOW - i % 261) for i in range(120)])):
        accepted(name, [("stored", back), ("fixed", toks)], out)
        accepted(name + "_dynamic", [("stored", back), _dyn(toks)], out)

    # -- lengths 258 and 257
    toks = lits + [(258, 7), (257, 7), (258, 1), (257, 24)]
    b = _dyn(toks)
    assert b[2]["ll"][285] and b[2]["ll"][284] and length_code(257) == (284, 30) and length_code(258) == (285, 0)
    accepted("length_258_by_285_and_257_by_284", [b], out)
    accepted("length_258_by_285_and_257_by_284_fixed", [("fixed", toks)], out)

    # -- overlap: the match repeats its own output
    for d in (1, 2, 3, 63, 64, 65):
        toks = [97 + i % 23 for i in range(70)]
        for l in range(3, 259):
            toks += [(l, d), 48 + l % 10]
        accepted("overlap/d%d_fixed" % d, [("fixed", toks)], out)
        accepted("overlap/d%d_dynamic" % d, [_dyn(toks)], out)

    # -- code lengths
    ll = [0] * 286
    shape = list(range(1, 16)) + [15]                                 # 1, 2, ..., 14, 15, 15: complete
    assert kraft(shape) == 32768
    syms = [256, 65, 67, 71, 84, 10, 78, 97, 99, 103, 116, 9, 48, 49, 257, 285]          # the rarest get the longest codes
    for s, l in zip(syms, shape):
        ll[s] = l
    dl = [0] * 30
    for s, l in zip((0, 3, 29, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 1, 2, 5), [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 15]):
        dl[s] = l
    assert kraft(dl) == 32768 and 9 in dl and 15 in dl and 11 in ll and 15 in ll
    toks = [65, 67, 71, 84, 10, 78, 97, 99, 103, 116, 9, 48, 49] * 3 + [(3, 1), (258, 4), (3, 39)]
    toks += [(3, d) for d in (2, 3, 7, 8)] + [48, 49, 49, 48] * 700 + [(258, DBASE[s]) for s in (10, 12, 14, 16, 18, 20, 22, 24)] + [49, 9, 116]
    lu, du = used_symbols(toks)
    assert {116, 257, 285} <= lu and {2, 5, 20} <= du and ll[116] == 11 and ll[285] == 15 and dl[20] == 9 and dl[5] == 15
    accepted("lengths/ll_1_to_15_15_and_dist_9_to_15", [("dynamic", toks, {"ll": ll, "dl": dl, "rle": rle_plain(ll + dl)})], out)
    cl = [0] * 19
    for s, l in zip((0, 18, 17, 1, 2, 3, 4, 5), (1, 2, 3, 4, 5, 6, 7, 7)):
        cl[s] = l
    ll7 = [0] * 257
    for s, l in zip((65, 66, 67, 68, 256), (1, 2, 3, 4, 4)):
        ll7[s] = l
    rle = rle_greedy(ll7) + [1]
    assert kraft(cl) == 32768 and kraft(ll7) == 32768 and cl[4] == 7 and 4 in rle
    accepted("lengths/code_length_code_of_7_bits", [("dynamic", [65, 66, 67, 68] * 9, {"ll": ll7, "dl": [1], "cl": cl, "rle": rle})], out)
    for name, blocks in hclen_cases():
        accepted(name, blocks, out)

    # -- repeat codes across the literal / distance boundary, and a run that ends exactly at nlen + ndist
    for name, blocks, check in crossing_cases():
        assert check
        accepted(name, blocks, out)

    # -- block chains
    st = noise(700, 41)
    toks = [(30, 700), (258, 600), (3, 1), 65, (100, 988)]
    accepted("chain/stored_then_dynamic_reading_it", [("stored", st), _dyn(toks)], out)
    accepted("chain/stored_then_fixed_reading_it", [("stored", st), ("fixed", toks)], out)
    # (a stored block of 65 535 bytes does not fit a BGZF member: gzip_cases() has it; this is the largest round one that does)
    accepted("chain/dynamic_stored0_stored1_stored64000_fixed", stored_chain(64000), out)
    accepted("chain/six_alternating", [("stored", st[:100]), ("fixed", [(50, 100)] + lits), _dyn(lits + [(40, 150)]), ("stored", st[100:300]),
                                       _dyn([(200, 200), 65, (258, 1)]), ("fixed", [(9, 3), 10])], out)
    for name, toks, pad in (("chain/eob_on_last_bit_of_byte", [200] * 6, 0), ("chain/eob_then_7_pad_bits", [200] * 7, 7)):
        info = {}
        assemble([("stored", b"xy"), ("fixed", toks)], info)
        assert info["pad"] == pad, (name, info)
        accepted(name, [("stored", b"xy"), ("fixed", toks)], out)
    return out


def stored_chain(n):
    lits = list(b"ACGTNacgtn\tchr1\n0|1.PASS")
    return [_dyn(lits * 3 + [(20, 5)]), ("stored", b""), ("stored", b"Z"), ("stored", noise(n - 200, 42) + bytes(200)),
            ("fixed", [(258, 200), (258, WINDOW), 66, (77, 1)])]


def hclen_cases():
    """HCLEN = 5 and 19, HLIT = 257 and 286, HDIST = 1 and 30.  HCLEN = 4 gives lengths to the symbols 16, 17, 18 and 0 alone:
    every code length such a block can state is 0, its end-of-block code included, so no valid block has it (it is a
    refused case below); 5, which adds the symbol 8, is the smallest that can be valid."""
    out = []
    ll = [8] * 255 + [0, 8]                                            # 256 codes of 8 bits: complete
    cl = [0] * 19
    cl[18], cl[0], cl[8], cl[16] = 2, 2, 2, 2
    assert kraft(ll) == 32768 and [CL_ORDER.index(s) for s in (16, 18, 0, 8)] == [0, 2, 3, 4]
    toks = list(b"HCLEN five: only 0 and 8 are code lengths")
    out.append(("header/hclen5_hlit257_hdist1", [("dynamic", toks, {"ll": ll, "dl": [0], "cl": cl, "hclen": 5})]))
    # HCLEN 19 (symbol 15 is the last of the order), HLIT 286, HDIST 30
    ll = [0] * 286
    shape = list(range(1, 16)) + [15]
    for s, l in zip((256, 65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 77, 285, 284), shape):
        ll[s] = l
    dl = [0] * 30
    dl[29], dl[0] = 1, 1
    toks = [65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 77] * 4 + [(258, 1), (257, 1), (227, 1)]
    b = ("dynamic", toks, {"ll": ll, "dl": dl, "rle": rle_greedy(ll + dl)})
    cl = default_cl(b[2]["rle"])
    assert cl[15] and len(ll) == 286 and len(dl) == 30
    out.append(("header/hclen19_hlit286_hdist30", [b]))
    return out


def crossing_cases():
    """Repeat codes whose run starts in the last literal/length lengths and ends in the first distance lengths, and runs
    that end exactly at nlen + ndist."""
    out = []
    # 16 with a non-zero value: ll[283] = ll[284] = 4 and dl[0 .. 4) = 4, one run of five over 284 .. 289
    toks = list(b"crossing") + [(5, 1), (4, 2), (3, 3)]
    ll, dl = [0] * 285, [0] * 16
    used = sorted(used_symbols(toks)[0])
    for s, l in zip(used, _complete_beside(len(used), 2, 4)):
        ll[s] = l
    ll[283] = ll[284] = 4
    for s, l in zip(range(4, 16), _complete_beside(12, 4, 4)):
        dl[s] = l
    dl[0] = dl[1] = dl[2] = dl[3] = 4
    seq = ll + dl
    rle = rle_plain(seq[:284]) + [(16, 5)] + rle_plain(seq[289:])
    assert kraft(ll) == 32768 and kraft(dl) == 32768 and seq[283:289] == [4] * 6 and rle_total(rle) == len(seq)
    out.append(("cross/16_nonzero", [("dynamic", toks, {"ll": ll, "dl": dl, "rle": rle})], 284 < len(ll) < 289))
    # 17 and 18 with zeros: the literal/length lengths end in `tail` zeros, the distance lengths begin with `head`
    for sym, rep, tail, head in ((17, 7, 3, 4), (18, 40, 25, 15)):
        toks = list(b"crossing") * 60 + [(5, DBASE[head]), (4, DBASE[head + 2])]
        opts = auto_codes(toks, nlen=260 + tail)
        opts["dl"] = [0] * head + [1, 0, 1]
        seq = opts["ll"] + opts["dl"]
        a = len(opts["ll"]) - tail
        assert seq[a:a + rep] == [0] * rep and a + rep == len(opts["ll"]) + head and seq[a - 1] and seq[a + rep]
        opts["rle"] = rle_plain(seq[:a]) + [(sym, rep)] + rle_plain(seq[a + rep:])
        out.append(("cross/%d_zeros" % sym, [("dynamic", toks, opts)], a < len(opts["ll"]) < a + rep))
    # a run that ends exactly at nlen + ndist, one of each repeat code
    toks = list(b"ends") + [(3, 1), (3, 2), (3, 3), (3, 4), (3, 5), (3, 7), (3, 9), (3, 13)]
    opts = auto_codes(toks)
    opts["dl"] = [3] * 8
    opts["rle"] = rle_greedy(opts["ll"]) + [3, 3, (16, 6)]
    assert rle_total(opts["rle"]) == len(opts["ll"]) + 8
    out.append(("cross/run_ends_at_the_end_16", [("dynamic", toks, opts)], True))
    for sym, rep in ((17, 10), (18, 29)):
        toks = list(b"ends") + [(3, 1)]
        opts = auto_codes(toks)
        opts["dl"] = [1] + [0] * rep
        opts["rle"] = rle_greedy(opts["ll"]) + [1, (sym, rep)]
        assert rle_total(opts["rle"]) == len(opts["ll"]) + len(opts["dl"]) <= 286 + 30
        out.append(("cross/run_ends_at_the_end_%d" % sym, [("dynamic", toks, opts)], True))
    return out


def _complete_beside(k, n_fixed, fixed_len):
    """k lengths that complete a code which already holds n_fixed codes of fixed_len."""
    room = 32768 - n_fixed * (1 << (15 - fixed_len))
    # binary expansion of the room into k powers of two: start from the largest pieces and split the smallest
    parts = [15 - i for i in range(16) if room >> i & 1]
    parts.sort()
    while len(parts) < k:
        d = parts.pop(0)                                   # the shallowest (largest) piece
        parts += [d + 1, d + 1]
        parts.sort()
    assert len(parts) == k and max(parts) <= 15 and min(parts) >= 1
    return parts


# ---- member sizes -----------------------------------------------------------------------------------------------
SIZES = (0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 32767, 32768, 32769, 65535, 65536)


@functools.lru_cache(maxsize=None)
def sized():
    """[(name, blocks, raw, text)] in file order: for every size and every r in 1..16 a member of r bytes, the member of
    that size, and a member that brings the output offset back to a multiple of 16 - the sized member starts at every
    residue mod 16."""
    out = []
    unit = bz.fasta_text(61 + 12, seed=5)[12:]
    for n in SIZES:
        toks = periodic_tokens(n, unit)
        body = [("fixed", toks)] if n % 2 else [_dyn(toks)]
        for r in range(1, 17):
            accepted("size/%d_at%d_lead" % (n, r % 16), [("stored", bytes(range(64, 64 + r)))], out)
            accepted("size/%d_at%d" % (n, r % 16), body, out)
            assert len(out[-1][3]) == n
            accepted("size/%d_at%d_trail" % (n, r % 16), [("fixed", [88] * (-(r + n) % 16))], out)
    return out


# ---- random valid streams ---------------------------------------------------------------------------------------
COUNTERS = ("far", "at_window", "batch_edge", "blocks_no_dist", "blocks_one_dist", "cross17", "cross18", "len258", "overlap")


def _biased(rng, n):
    """0 .. n, the two ends favoured."""
    r = rng.random()
    return 0 if r < 0.3 else n if r < 0.6 else rng.randint(0, n)


def _draw_tokens(rng, text, lits, lsyms, dsyms, ntok, room, cnt):
    toks = []
    for _ in range(ntok):
        have = len(text)
        ds = [d for d in dsyms if DBASE[d] <= have]
        if lsyms and ds and room >= 3 and (not lits or rng.random() < 0.5):
            s = rng.choice(lsyms)
            l = LBASE[s - 257] + _biased(rng, 30 if s == 284 else (1 << LEXT[s - 257]) - 1)        # (258 is symbol 285's)
            d = rng.choice(ds)
            dist = min(DBASE[d] + _biased(rng, (1 << DEXT[d]) - 1), have)
            if l > room:
                break
            toks.append((l, dist))
            copy_match(text, l, dist)
            room -= l
            cnt["far"] += dist > FAR
            cnt["at_window"] += dist == WINDOW
            cnt["batch_edge"] += dist > BATCH_EDGE
            cnt["len258"] += l == 258
            cnt["overlap"] += dist < l
            cnt["max_distance"] = max(cnt["max_distance"], dist)
        elif lits and room >= 1:
            c = rng.choice(lits)
            toks.append(c)
            text.append(c)
            room -= 1
        else:
            break
    return toks


def _random_rle(rng, seq, nlen, cnt):
    out, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        rep = 1
        if v == 0 and run >= 3 and rng.random() < 0.7:
            if run >= 11 and rng.random() < 0.7:
                rep = rng.randint(11, min(run, 138))
                out.append((18, rep))
                cnt["cross18"] += i < nlen < i + rep
            else:
                rep = rng.randint(3, min(run, 10))
                out.append((17, rep))
                cnt["cross17"] += i < nlen < i + rep
        elif v and i and seq[i - 1] == v and run >= 3 and rng.random() < 0.7:
            rep = rng.randint(3, min(run, 6))
            out.append((16, rep))
            cnt["cross16"] += i < nlen < i + rep
        else:
            out.append(v)
        i += rep
    return out


def random_blocks(seed, cnt):
    rng = random.Random(seed)
    blocks, text = [], bytearray()
    for _ in range(rng.randint(1, 6)):
        room = 65536 - len(text)
        budget = min(room, rng.choice((rng.randint(0, 400), rng.randint(0, 40000), 65536)))
        kind = rng.randrange(3)
        if kind == 0:
            data = rng.randbytes(min(budget, 65535, rng.choice((0, 1, 300, 33000, 40000))))
            text += data
            blocks.append(("stored", data))
        elif kind == 1:
            blocks.append(("fixed", _draw_tokens(rng, text, list(range(256)), list(range(257, 286)), list(range(30)), rng.randint(0, 700), budget, cnt)))
        else:
            nd = rng.randint(0, 12)
            dsyms = rng.sample(range(28), nd)
            if nd and rng.random() < 0.7:
                dsyms[0] = 29
            if nd > 1 and rng.random() < 0.5:
                dsyms[1] = 28
            nl = rng.choice((0, 1, 2, rng.randint(3, 40), rng.randint(3, 256)))
            lits = rng.sample(range(256), nl)
            lsyms = rng.sample(range(257, 285), rng.randint(0 if lits else 1, 20)) if nd else []
            if nd and rng.random() < 0.5:
                lsyms.append(285)
            ll = lengths_for(lits + [256] + lsyms, max(257, max(lsyms, default=0) + 1), 15, rng)
            dl = lengths_for(dsyms, max(1, max(dsyms, default=0) + 1), 15, rng)
            if rng.random() < 0.5:
                ll += [0] * rng.randint(0, 286 - len(ll))
            if rng.random() < 0.5:
                dl += [0] * rng.randint(0, 30 - len(dl))
            cnt["blocks_no_dist"] += nd == 0
            cnt["blocks_one_dist"] += nd == 1
            rle = _random_rle(rng, ll + dl, len(ll), cnt)
            used = set(rle_symbols(rle)) | set(rng.sample(range(19), rng.randint(0, 3)))
            if len(used) == 1:
                used.add((min(used) + 1) % 19)
            cl = lengths_for(used, 19, 7, rng)
            lo = max(4, 1 + max(i for i in range(19) if cl[CL_ORDER[i]]))
            toks = _draw_tokens(rng, text, lits, lsyms, dsyms, rng.randint(0, 700), budget, cnt)
            blocks.append(("dynamic", toks, {"ll": ll, "dl": dl, "cl": cl, "rle": rle, "hclen": rng.randint(lo, 19)}))
    return blocks


N_SEEDS = 600


@functools.lru_cache(maxsize=None)
def random_corpus(n_seeds=N_SEEDS, first=1000):
    """([(name, blocks, raw, text)], counters): one member per seed; a member that does not fit BSIZE is dropped and counted."""
    cnt = dict.fromkeys(COUNTERS + ("cross16", "max_distance", "drops", "seeds"), 0)
    out = []
    for seed in range(first, first + n_seeds):
        trial = dict(cnt)
        blocks = random_blocks(seed, trial)
        if len(assemble(blocks)) + 26 > 65536:
            cnt["drops"] += 1
            continue
        cnt = trial
        accepted("random/seed%d" % seed, blocks, out)
    cnt["seeds"] = n_seeds
    return out, cnt


def accepted_cases():
    """Every accepted member: directed, sized (in file order), random."""
    return directed() + sized() + random_corpus()[0]


def accepted_files():
    """The accepted members as BGZF files: 64 to a file, the sized ones one size (16 triples) to a file."""
    return bgzf_files(directed()) + bgzf_files(sized(), 48) + bgzf_files(random_corpus()[0])


def bgzf_files(cases, per_file=64):
    """[(file bytes, block table, [(name, text)])]: the members of `cases` in order, per_file to a file, the EOF block last."""
    files = []
    for i in range(0, len(cases), per_file):
        data, table, names, at, off = [], [], [], 0, 0
        for name, _, raw, text in cases[i:i + per_file]:
            m = wrap(raw, text)
            table.append((at, off, len(m), len(text)))
            names.append((name, text))
            data.append(m)
            at += len(m)
            off += len(text)
        table.append((at, off, len(bz.EOF_BLOCK), 0))
        files.append((b"".join(data) + bz.EOF_BLOCK, table, names))
    return files


def gzip_cases():
    """[(name, file bytes, text)]: plain gzip members (the host path) around a subset of the raw streams, several members in
    one file, and one member of more than 64 KiB whose blocks are those of several streams."""
    pool = directed()[::7] + random_corpus()[0][::25]
    out = [("gzip/" + name, gzip_wrap(raw, text), text) for name, _, raw, text in pool]
    blocks = stored_chain(65535)
    out.append(("gzip/chain_dynamic_stored0_stored1_stored65535_fixed", gzip_wrap(assemble(blocks), expand(blocks)), expand(blocks)))
    out.append(("gzip/members_chained", b"".join(d for _, d, _ in out[:12]), b"".join(t for _, _, t in out[:12])))
    big = [c for c in directed() if c[0].startswith("far/")][:3] + random_corpus()[0][:5] + [c for c in directed() if c[0].startswith("chain/")]
    blocks = [b for c in big for b in c[1]]
    raw, text = assemble(blocks), expand(blocks)
    assert text == b"".join(c[3] for c in big) and len(text) > 2 * 65536
    out.append(("gzip/one_member_over_64k", gzip_wrap(raw, text), text))
    for name, data, text in out:
        assert gzip.decompress(data) == text, name
    return out


# ---- streams that must be refused -------------------------------------------------------------------------------
INVALID, LENGTH, CRC = "invalid DEFLATE stream", "length mismatch", "CRC mismatch"


@functools.lru_cache(maxsize=None)
def refused():
    """[(name, member bytes, reason)]: one fault each in an otherwise valid BGZF member; gzip.decompress raises on every one."""
    out = []
    lits = list(b"refuse me: ACGT\n")
    text = bytes(lits)
    good = auto_codes(lits)
    good["dl"] = [1]                                           # (valid under every reading of the rules for degenerate codes)

    def add(name, blocks, lenient=b"", reason=INVALID, isize=None, crc=None, raw=None):
        out.append((name, wrap(assemble(blocks) if raw is None else raw, lenient, isize, crc), reason))

    def dyn(name, lenient=text, toks=lits, **over):
        opts = dict(good)
        opts.update(over)
        add(name, [("dynamic", toks, opts)], lenient)

    add("block_type_3", [("bits", [(3, 2)])])
    add("stored_len_nlen_not_complementary", [("stored", text, {"nlen": (len(text) ^ 0xffff) ^ 0x100})], text)
    dyn("hlit_287", ll=good["ll"] + [0] * (287 - len(good["ll"])))
    dyn("hlit_288", ll=good["ll"] + [0] * (288 - len(good["ll"])))
    dyn("hdist_31", dl=[0] * 31)
    dyn("hdist_32", dl=[0] * 32)
    rle = rle_greedy(good["ll"] + good["dl"])
    used = sorted(set(rle_symbols(rle)))
    cl = default_cl(rle)
    deepest = max(used, key=lambda s: cl[s])
    less = list(cl); less[deepest] += 1
    assert kraft(cl) == 32768 and 0 < kraft(less) < 32768 and less[deepest] <= 7
    dyn("clen_code_incomplete", cl=less, rle=rle)
    more = list(cl); more[deepest] -= 1
    assert kraft(more) > 32768
    dyn("clen_code_oversubscribed", cl=more, rle=rle)
    one = [0] * 19; one[8] = 1
    dyn("clen_code_single_symbol_length1", b"", [], ll=[8] * 257, dl=[8], cl=one, rle=[8] * 258)
    seq = good["ll"] + good["dl"]
    assert seq[:3] == [0, 0, 0]
    dyn("code_16_first", rle=[(16, 3)] + rle_greedy(seq[3:]))
    past = rle_greedy(good["ll"]) + [1, (17, 5)]
    assert rle_total(past) == len(good["ll"]) + 5 + 1
    dyn("run_passes_the_end_by_one", dl=[1, 0, 0, 0, 0], rle=past)
    four = [0] * 19; four[16], four[17], four[18], four[0] = 2, 2, 2, 2
    dyn("hclen_4_no_length_but_0", b"", [], ll=[0] * 257, dl=[0], cl=four, hclen=4, rle=[(18, 138), (18, 120)], eob=False)
    no_eob = list(good["ll"])
    swap = max(s for s in range(256) if not no_eob[s])
    no_eob[swap], no_eob[256] = no_eob[256], 0
    assert kraft(no_eob) == 32768
    dyn("no_end_of_block_code", ll=no_eob, eob=False)
    k = sorted(used_symbols(lits)[0])
    ll = list(good["ll"]); ll[k[0]] -= 1
    assert kraft(ll) > 32768
    dyn("lit_code_oversubscribed", ll=ll)
    ll = list(good["ll"]); ll[k[0]] += 1
    assert 0 < kraft(ll) < 32768
    dyn("lit_code_incomplete", ll=ll)
    two = [0] * 257; two[65], two[256] = 1, 2
    dyn("lit_code_incomplete_two_symbols", b"AAAA", [65] * 4, ll=two)
    dyn("lit_code_single_symbol_length2", b"", [], ll=[0] * 256 + [2])
    mt = lits + [(3, 1), (3, 2), (3, 4)]
    mtext = expand([("fixed", mt)])
    mg = auto_codes(mt)
    dyn("dist_code_oversubscribed", mtext, mt, ll=mg["ll"], dl=[1, 1, 0, 1])
    t2 = lits + [(3, 1), (3, 2)]
    g2 = auto_codes(t2)
    dyn("dist_code_incomplete_two_symbols", expand([("fixed", t2)]), t2, ll=g2["ll"], dl=[1, 2])
    t1 = lits + [(3, 1), (4, 1)]
    g1 = auto_codes(t1)
    dyn("dist_code_single_symbol_length2", expand([("fixed", t1)]), t1, ll=g1["ll"], dl=[2])
    dyn("dist_code_single_symbol_length15", expand([("fixed", t1)]), t1, ll=g1["ll"], dl=[15])
    dyn("length_symbol_with_empty_dist_code", text, lits + [("L", 257, 0)], ll=g1["ll"], dl=[0])
    for s in (286, 287):
        add("fixed_symbol_%d" % s, [("fixed", lits + [("L", s, 0), ("D", 0, 0)])], text)
    for s in (30, 31):
        add("fixed_distance_code_%d" % s, [("fixed", lits + [("L", 257, 0), ("D", s, 0)])], text)
    add("distance_beyond_start_at_0", [("fixed", [("L", 257, 0), ("D", 0, 0)] + lits)], text)
    add("distance_beyond_start_after_stored", [("stored", text), ("fixed", [("L", 257, 0), ("D", *dist_code(len(text) + 1))] + lits)], text + text)
    assert dist_code(len(text) + 1) == (8, 0) and DBASE[8] == len(text) + 1
    # the text one byte longer than ISIZE (by a literal, a match, a stored block), and one byte shorter
    for name, blocks in (("literal", [("fixed", lits)]), ("match", [("fixed", lits[:-3] + [(3, 5)])]), ("stored", [("fixed", lits[:4]), ("stored", text[4:])])):
        t = expand(blocks)
        add("text_longer_than_isize_by_" + name, blocks, t, LENGTH, isize=len(t) - 1)
    add("text_shorter_than_isize", [("fixed", lits)], text, LENGTH, isize=len(text) + 1)
    raw = assemble([("fixed", lits)])
    add("padding_byte_before_trailer", None, text, raw=raw + b"\0")
    info = {}
    raw = assemble([("fixed", lits)], info)
    assert info["pad"] == 6                                    # the last byte holds the last two bits of the end-of-block code
    add("end_of_block_cut_off", None, text, raw=raw[:-1])
    unit = bz.vcf_text(997, seed=9)
    blocks = [_dyn(periodic_tokens(65536, unit))]
    t = expand(blocks)
    assert len(t) == 65536
    add("crc_wrong_on_65536_bytes", blocks, t, CRC, crc=(zlib.crc32(t) ^ 0x00010000) & 0xffffffff)
    for name, member, _ in out:
        assert bz.EOF_BLOCK[:4] == member[:4]
        try:
            gzip.decompress(member)
        except Exception:
            continue
        raise AssertionError("%s: gzip.decompress accepts it (the test module is wrong)" % name)
    return out


def refused_files():
    """[(name, file bytes, reason)]: a valid member, the faulty member, a valid member - the refusal names block 1."""
    ok = [c for c in directed() if c[0] == "chain/six_alternating"][0]
    valid = wrap(ok[2], ok[3])
    return [(name, valid + member + valid, reason) for name, member, reason in refused()]


# ---- the corpora as a file for tests/cpp/test_inflate.cpp ---------------------------------------------------------
def write_corpus_file(path, with_accepted=True):
    with open(path, "wb") as f:
        if with_accepted:
            for name, _, raw, text in accepted_cases():
                f.write(bz._record(0, 1, name, wrap(raw, text), text))
            for name, data, text in gzip_cases():
                f.write(bz._record(0, 2, name, data, text))
        for name, data, reason in refused_files():
            f.write(bz._record(1, 0, name, data, ("1\n%s" % reason).encode()))


def host_run(root, workdir, with_accepted=True):
    """(returncode, {refused case: error text}, log) of the sanitized host decoder over the corpora of this module."""
    import os
    import subprocess
    exe = bz.build_test_inflate(root, os.path.join(workdir, "test_inflate_deflate_spec"))
    corpus_file = os.path.join(workdir, "deflate_corpus.bin")
    write_corpus_file(corpus_file, with_accepted)
    r = subprocess.run([exe, corpus_file], capture_output=True, text=True)
    return r.returncode, dict(line.split("\t", 1) for line in r.stdout.splitlines()), r.stderr


def far_lz77(text, min_dist=FAR + 1):
    """Tokens of `text` by a trivial LZ77 that looks only min_dist .. 32768 bytes back (first occurrence of the next four
    bytes in that window, extended as far as it goes)."""
    toks, i, n = [], 0, len(text)
    while i < n:
        lo, hi = max(0, i - WINDOW), i - min_dist
        j = text.find(text[i:i + 4], lo, hi + 4) if hi >= lo and i + 4 <= n else -1
        if j < 0:
            toks.append(text[i])
            i += 1
            continue
        l = 4
        while l < 258 and i + l < n and text[j + l] == text[i + l]:
            l += 1
        toks.append((l, i - j))
        i += l
    return toks
