"""The device-resident MSA calls (edsx_msa_plan_device, edsx_msa_emit_device, edsx_msa_synth_device[_aligned]) on
memory the CALLER owns and on a stream the CALLER chooses, as include/edsx.h words the contract: outputs of exactly the
planned sizes, pointers at any byte address, an input with nothing readable around it, completion in stream order,
emit repeated after one plan.  Buffers are tests/arena.py payloads between two 64 KiB zones (what libedsx_guard.so does
for the library's own buffers); alignments and their premises are in tests/msa_resident_cases.py (premises checked on
the CPU by tests/test_msa_resident_cpu.py).  Every comparison is byte-equal with the CPU oracle."""
import pytest

import msa_resident_cases as mc
import oracle_lib as o
from arena import ZONE, Arena

pytestmark = pytest.mark.gpu

OUT_FILLS = [0x00, 0xFF, ord("{"), ord("}"), ord(",")]
IN_FILLS = [0x00, 0xFF, ord("\n"), ord(">"), ord("A")]
OFFSETS = [0, 1, 3, 4, 8, 15, 128]
EDSX_ERR_INVALID_FORMAT, EDSX_ERR_INVALID_PARAMETER = 2, 3


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    c = edsparser_amd.Context(0)              # one context for the whole file: the library's own buffers are not the subject
    yield c
    c.close()


_ORACLE = {}


def _want(key, text, l):
    """The oracle's (eds, seds) of a case, computed once and shared by the tests."""
    if key not in _ORACLE:
        _ORACLE[key] = o.msa(text, l)
    return _ORACLE[key]


_CASES, _IMPOSSIBLE = mc.constructed_cases()
_GROUPS = {"S%d" % S: [c for c in _CASES if c.S == S and c.l == 0 and c.kind != "huge"] for S in mc.ROWS + mc.ROUTE_ROWS}
_GROUPS["huge"] = [c for c in _CASES if c.kind == "huge"]
for _l in mc.MIXED_L:
    _GROUPS["mixed_l%d" % _l] = [c for c in _CASES if c.l == _l]
_GROUP_SIZES = {"S2": 39, "S70": 57, "S999": 57, "S1000": 57, "S1025": 29, "S8193": 29, "huge": 4, "mixed_l3": 52, "mixed_l10": 52}


def _sync(stream=None):
    """Wait for the caller's stream only (never the device)."""
    import torch
    (stream or torch.cuda.current_stream()).synchronize()


def _emit_into_arenas(ctx, E, Q, fill, tag, off_e=0, off_q=0, stream=0):
    ae, aq = Arena(E, fill, off_e, name=tag + " eds"), Arena(Q, fill, off_q, name=tag + " seds")
    ctx.msa_emit_device(ae.ptr, aq.ptr, stream)
    return ae, aq


def _check_outputs(ae, aq, want, tag):
    assert ae.download() == want[0], tag + ": .eds"
    assert aq.download() == want[1], tag + ": .seds"
    ae.assert_clean()
    aq.assert_clean()


# ---- the helper itself ----------------------------------------------------------------------------------------
def test_arena_reports_a_planted_byte_exactly_where_it_is():
    for n, off in [(0, 0), (1, 1), (1000, 15), (4097, 128)]:
        a = Arena(n, 0x5A, off, name="probe")
        assert (a.ptr - off) % 256 == 0 and a.payload.numel() == n
        assert a.check() == [] and a.download() == b"\x5a" * n
        a.payload.fill_(0x11)                                        # the payload itself is the caller's to write
        assert a.check() == []
        a.buf[a.start + n] = 0x7B                                    # payload offset N: the first byte behind it
        assert a.check() == ["probe %d bytes, back zone, offsets +0..+0, fill 5a, found 7b" % n]
        a.buf[a.start - 1] = 0x7D                                    # payload offset -1
        a.buf[a.start + n + ZONE - 1] = 0x00                         # the far end of the reach
        assert a.check() == ["probe %d bytes, front zone, offsets -1..-1, fill 5a, found 7d" % n,
                             "probe %d bytes, back zone, offsets +0..+%d, fill 5a, found 7b 00" % (n, ZONE - 1)]
        with pytest.raises(AssertionError):
            a.assert_clean()
    b = Arena(8, 0x00, 0, front=0xFF, back=ord(">"))
    z = b.buf.cpu().numpy()
    assert set(z[b.start - ZONE:b.start]) == {0xFF} and set(z[b.start + 8:b.start + 8 + ZONE]) == {ord(">")}


def test_the_groups_cover_every_constructed_case():
    assert sum(len(g) for g in _GROUPS.values()) == len(_CASES) == mc.N_CONSTRUCTED == 376
    assert {k: len(g) for k, g in _GROUPS.items()} == _GROUP_SIZES
    assert len(_IMPOSSIBLE) == 30 and all(S == 2 or (kind == "a1" and wrapped) for kind, S, wrapped in _IMPOSSIBLE)


# ---- output containment ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(_GROUPS))
def test_outputs_of_exactly_the_planned_sizes(ctx, group):
    """d_eds and d_seds of exactly E and Q bytes: after emit and a wait for the stream every payload byte equals the
    oracle under five fills (so every byte was written) and no byte of the zones in front of and behind them changed.
    One plan, five emits.  Routing through n_slow_segments (the rule is in the CPU premises test)."""
    ran = 0
    for c in _GROUPS[group]:
        text, _rows = c.build()
        want = _want(c.id, text, c.l)
        inp = Arena(len(text), name=c.id + " msa").upload(text)
        E, Q = ctx.msa_plan_device(inp.ptr, len(text), c.l)
        assert (E, Q) == (len(want[0]), len(want[1])), c.id
        info = ctx.msa_info()
        assert (info["n_rows"], info["n_cols"]) == (c.S, c.width()), c.id
        if c.l == 0:
            assert info["n_slow_segments"] == c.slow, c.id
        elif c.slow:
            assert info["n_slow_segments"] >= 1, c.id
        for fill in OUT_FILLS:
            tag = "%s fill %02x" % (c.id, fill)
            ae, aq = _emit_into_arenas(ctx, E, Q, fill, tag)
            _sync()
            _check_outputs(ae, aq, want, tag)
        inp.assert_clean()
        ran += 1
    assert ran == _GROUP_SIZES[group]


def test_launch_counts_tell_the_route(ctx):
    """Up to 1024 rows: the wave-per-segment emitters (main, wide8, wide16), the generic one on a side stream and the two
    common-text kernels, once each; more rows: the row-loop emitter and the generic one."""
    ctx.set_timing(True)
    try:
        for c in mc.one_per_route():
            text, _ = c.build()
            want = _want(c.id, text, 0)
            inp = Arena(len(text)).upload(text)
            ctx.set_timing(True)                                     # (clears the counts)
            E, Q = ctx.msa_plan_device(inp.ptr, len(text), 0)
            ae, aq = _emit_into_arenas(ctx, E, Q, 0xFF, c.id)
            _sync()
            n = {name: cnt for name, _ms, cnt in ctx.get_timing()}
            common = {"k_scan_extract": 1, "k_emit_common_seg": 1, "k_emit_common_long": 1}
            if c.S <= 1024:
                exp = dict(common, k_seg_meta=1, k_emit_fast=1, k_emit_fast_wide8=1, k_emit_fast_wide16=1, k_emit_variant_slow=1)
                absent = ("k_rl_count", "k_rl_emit", "k_emit_variant")
            else:
                exp = dict(common, k_rl_count=1, k_rl_emit=1, k_emit_variant=1)
                absent = ("k_seg_meta", "k_emit_fast", "k_emit_variant_slow")
            assert {k: n.get(k) for k in exp} == exp, (c.id, n)
            assert not [k for k in absent if k in n], (c.id, n)
            assert ("k_vmap" in n) == bool(c.lw), c.id        # wrapped rows: mv.lw != 0
            _check_outputs(ae, aq, want, c.id)
    finally:
        ctx.set_timing(False)


# ---- pointer alignment ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["d_msa", "d_eds", "d_seds", "all"])
def test_pointers_at_any_byte_address(ctx, which):
    """The three pointers a bytes off a 256-byte boundary, one at a time and all three at once, one case per route.
    (The plan and emit kernels touch caller memory through byte accesses, load16u / store16u / store_small - memcpy forms
    that assume no alignment - and never with atomics; every typed cast in them is on the library's own tables.)"""
    combos = [(1, 3, 15), (15, 1, 8), (128, 4, 3), (3, 128, 1)] if which == "all" else \
             [tuple(a if w == which else 0 for w in ("d_msa", "d_eds", "d_seds")) for a in OFFSETS]
    ran = 0
    for c in mc.one_per_route():
        text, _ = c.build()
        want = _want(c.id, text, 0)
        planned_at = None
        for am, ae_, aq_ in combos:
            tag = "%s offsets %d/%d/%d" % (c.id, am, ae_, aq_)
            if planned_at != am:
                inp = Arena(len(text), 0, am, name=tag + " msa").upload(text)
                assert inp.ptr % 256 == am
                assert ctx.msa_plan_device(inp.ptr, len(text), 0) == (len(want[0]), len(want[1])), tag
                planned_at = am
            ae, aq = _emit_into_arenas(ctx, len(want[0]), len(want[1]), 0xFF, tag, ae_, aq_)
            assert (ae.ptr % 256, aq.ptr % 256) == (ae_, aq_)
            _sync()
            _check_outputs(ae, aq, want, tag)
            inp.assert_clean()
            ran += 1
    assert ran == len(combos) * len(mc.one_per_route()) and len(mc.one_per_route()) == 22


# ---- input independence ---------------------------------------------------------------------------------------
_INPUTS = mc.input_cases()
_TEXTS = {}


def _input_text(c):
    if c.id not in _TEXTS:
        _TEXTS[c.id] = c.build()
    return _TEXTS[c.id]


@pytest.mark.parametrize("fill", IN_FILLS + ["mixed"], ids=lambda f: f if f == "mixed" else "%02x" % f)
def test_result_does_not_depend_on_bytes_around_the_input(ctx, fill):
    """The alignment in a payload of exactly n bytes; the 64 KiB in front of and behind it hold NUL, 0xFF, newlines,
    '>' or letters ("mixed": different bytes in front and behind, every fourth case).  The result is the oracle's under
    every fill, for every way the text can end."""
    ran = 0
    pairs = [(0x00, 0xFF), (ord(">"), ord("\n")), (ord("\n"), ord("A")), (ord("A"), ord(">")), (0xFF, 0x00)]
    for i, c in enumerate(_INPUTS):
        if fill == "mixed" and i % 4:
            continue
        front, back = pairs[(i // 4) % len(pairs)] if fill == "mixed" else (fill, fill)
        text = _input_text(c)
        want = _want("in " + c.id, text, c.l)
        tag = "%s zones %02x/%02x" % (c.id, front, back)
        inp = Arena(len(text), 0, i % 16, front=front, back=back, name=tag).upload(text)
        assert ctx.msa_plan_device(inp.ptr, len(text), c.l) == (len(want[0]), len(want[1])), tag
        info = ctx.msa_info()
        assert (info["n_rows"], info["n_cols"]) == (c.S, c.L), tag
        ae, aq = _emit_into_arenas(ctx, len(want[0]), len(want[1]), 0x00, tag)
        _sync()
        _check_outputs(ae, aq, want, tag)
        inp.assert_clean()
        ran += 1
    assert ran == (mc.N_INPUT // 4 if fill == "mixed" else mc.N_INPUT)


def test_format_errors_do_not_depend_on_bytes_around_the_input(ctx):
    """A ragged last row (and the other texts of test_msa_gpu.py::test_format_errors): the same refusal whatever lies
    around the text - with zones of letters, '>' or newlines a read past the end would find a longer row or another
    header there - and in the words the library has for that text (a short, a long and a differently wrapped last row
    are all "rows must have equal length ..."; none of them names a row).  Emit after the failed plan is refused as well."""
    import edsparser_amd
    ragged = "Invalid MSA: rows must have equal length and a uniform line width"
    expected = {b"": "Invalid MSA: empty input",
                b"ACGT\n": "Invalid MSA: expected a FASTA header line starting with '>'",
                b">a\nACGT\n": "Invalid MSA: at least two sequences are required",
                b">a\nACGT\n>b\nAC\n": ragged, b">a\nACGT\n>b\nACGTA\n": ragged, b">a\nAC\nGT\n>b\nACG\nT\n": ragged}
    assert set(expected) == set(mc.FORMAT_ERRORS)
    for bad in mc.FORMAT_ERRORS:
        seen = set()
        for front, back in [(f, f) for f in IN_FILLS] + [(ord("\n"), ord("A")), (ord("A"), ord(">"))]:
            inp = Arena(len(bad), 0, 1, front=front, back=back).upload(bad)
            with pytest.raises(edsparser_amd.EdsxError) as ei:
                ctx.msa_plan_device(inp.ptr, len(bad), 0)
            assert ei.value.code == EDSX_ERR_INVALID_FORMAT and ei.value.message == expected[bad], (bad, front, back)
            seen.add(ei.value.message)
            out = Arena(64, 0xFF)
            with pytest.raises(edsparser_amd.EdsxError) as ei:
                ctx.msa_emit_device(out.ptr, out.ptr)
            assert ei.value.code == EDSX_ERR_INVALID_PARAMETER, bad
            _sync()
            assert out.download() == b"\xff" * 64
            out.assert_clean()
            inp.assert_clean()
        assert len(seen) == 1, (bad, seen)


# ---- stream semantics -----------------------------------------------------------------------------------------
def _pinned_copy(torch, t):
    h = torch.empty(t.numel(), dtype=torch.uint8, pin_memory=True)
    h.copy_(t, non_blocking=True)
    return h


def test_results_are_complete_in_stream_order(ctx):
    """Everything on one non-blocking stream of the caller's: plan, emit, an asynchronous copy of both outputs into pinned
    memory, and a wait for THAT stream as the only wait (emit forks onto two internal streams and joins them back: a
    missing join would leave the copy with unwritten bytes).  One case per route."""
    import torch
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for c in mc.one_per_route():
            text, _ = c.build()
            want = _want(c.id, text, 0)
            inp = Arena(len(text), name=c.id + " msa").upload(text)
            E, Q = ctx.msa_plan_device(inp.ptr, len(text), 0, stream=s.cuda_stream)
            ae, aq = _emit_into_arenas(ctx, E, Q, 0xFF, c.id, stream=s.cuda_stream)
            he, hq = _pinned_copy(torch, ae.payload), _pinned_copy(torch, aq.payload)
            s.synchronize()
            assert he.numpy().tobytes() == want[0] and hq.numpy().tobytes() == want[1], c.id
            ae.assert_clean()
            aq.assert_clean()


@pytest.mark.parametrize("S,L,l", [(1000, 60000, 10), (2000, 20000, 5)])
def test_generated_alignment_on_the_callers_stream(ctx, S, L, l):
    """msa_synth_device, plan and emit on one non-blocking stream, shapes that put work on both internal streams of emit
    (the generic emitter and the common text beside the wide emitters); the only wait is for the caller's stream."""
    import torch
    import edsparser_amd
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        n = edsparser_amd.synth_size(S, L)
        inp = Arena(n, 0xFF, name="synth")
        assert ctx.msa_synth_device(inp.ptr, n, S, L, seed=42 + S, stream=s.cuda_stream) == n
        E, Q = ctx.msa_plan_device(inp.ptr, n, l, stream=s.cuda_stream)
        ae, aq = _emit_into_arenas(ctx, E, Q, 0xFF, "synth", stream=s.cuda_stream)
        hm, he, hq = _pinned_copy(torch, inp.payload), _pinned_copy(torch, ae.payload), _pinned_copy(torch, aq.payload)
        s.synchronize()
        want = o.msa(hm.numpy().tobytes(), l)
        assert ctx.msa_info()["n_slow_segments"] > 0
        assert (E, Q) == (len(want[0]), len(want[1]))
        assert he.numpy().tobytes() == want[0] and hq.numpy().tobytes() == want[1]
        for a in (inp, ae, aq):
            a.assert_clean()


def test_two_transforms_back_to_back_on_one_stream(ctx):
    """Two plan + emit pairs on the same stream into different outputs with no wait of the caller's between them, then
    the copies and one wait.  (The second plan waits for the stream itself to hand its sizes back, so the first emit has
    finished before the tables are reused: what this pins is that the FIRST pair's outputs and zones are still right
    after a second transform went through the same context, and that the second emit is complete after the one wait.)"""
    import torch
    sub = {c.id: c for c in mc.one_per_route()}
    pairs = [("v1-S1000-oneline-l0", "gstrings-S1025-oneline-l0"), ("gstrings-S1025-oneline-l0", "w9-S70-oneline-l0"),
             ("c513-S2-lw60-l0", "v1-S1000-oneline-l0"), ("c1-S8193-oneline-l0", "gcols-S2-oneline-l0")]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for ida, idb in pairs:
            held = []
            for c in (sub[ida], sub[idb]):
                text, _ = c.build()
                want = _want(c.id, text, 0)
                inp = Arena(len(text), name=c.id + " msa").upload(text)
                E, Q = ctx.msa_plan_device(inp.ptr, len(text), 0, stream=s.cuda_stream)
                ae, aq = _emit_into_arenas(ctx, E, Q, 0xFF, c.id, stream=s.cuda_stream)
                held.append((c, want, inp, ae, aq))
            copies = [(_pinned_copy(torch, ae.payload), _pinned_copy(torch, aq.payload)) for _c, _w, _i, ae, aq in held]
            s.synchronize()
            for (c, want, inp, ae, aq), (he, hq) in zip(held, copies):
                assert he.numpy().tobytes() == want[0] and hq.numpy().tobytes() == want[1], (ida, idb, c.id)
                ae.assert_clean()
                aq.assert_clean()


# ---- repeated emit --------------------------------------------------------------------------------------------
def test_emit_twice_after_one_plan(ctx):
    """The plan survives an emit (bench.py plans once and emits per step): two emits into two outputs with different
    fills, no wait between them, both the oracle's; a plan that fails forgets the earlier plan."""
    import edsparser_amd
    for c in mc.one_per_route():
        text, _ = c.build()
        want = _want(c.id, text, 0)
        inp = Arena(len(text)).upload(text)
        E, Q = ctx.msa_plan_device(inp.ptr, len(text), 0)
        first = _emit_into_arenas(ctx, E, Q, 0x00, c.id + " first")
        second = _emit_into_arenas(ctx, E, Q, 0xFF, c.id + " second")
        _sync()
        _check_outputs(*first, want, c.id + " first")
        _check_outputs(*second, want, c.id + " second")
    bad = b">a\nACGT\n>b\nAC\n"
    inp = Arena(len(bad)).upload(bad)
    with pytest.raises(edsparser_amd.EdsxError) as ei:
        ctx.msa_plan_device(inp.ptr, len(bad), 0)
    assert ei.value.code == EDSX_ERR_INVALID_FORMAT
    out = Arena(E + Q, 0xFF)
    with pytest.raises(edsparser_amd.EdsxError) as ei:
        ctx.msa_emit_device(out.ptr, out.ptr)
    assert ei.value.code == EDSX_ERR_INVALID_PARAMETER and "without a successful plan" in ei.value.message
    _sync()
    assert out.download() == b"\xff" * (E + Q)
    out.assert_clean()


# ---- generators -----------------------------------------------------------------------------------------------
GEN_S = [2, 9, 10, 11, 99, 100, 101, 1000]
GEN_L = [1, 15, 16, 17, 63, 64, 65, 1000]


@pytest.mark.parametrize("row_align", [0, 4, 128])
def test_generators_fill_exactly_their_size(ctx, row_align):
    """msa_synth_device / msa_synth_device_aligned into a payload of exactly synth_size bytes: the same bytes over a
    payload of NULs and one of 0xFF (every byte is written), clean zones, a text the oracle reads as S rows of L columns;
    row counts around every change of the digits of ">s<idx>", row lengths around the 16-byte chunks of the fill kernel,
    a column offset, three pointer offsets.  One byte less of capacity is refused and nothing is written."""
    import edsparser_amd
    ran = 0
    for S in GEN_S:
        for L in GEN_L:
            n = edsparser_amd.synth_size(S, L, row_align)
            for col0 in (0, 12345):
                texts = set()
                for a in (0, 1, 15):
                    for fill in (0x00, 0xFF):
                        out = Arena(n, fill, a, name="synth S=%d L=%d col0=%d align=%d offset %d" % (S, L, col0, row_align, a))
                        assert ctx.msa_synth_device(out.ptr, n, S, L, col0=col0, seed=7, row_align=row_align) == n
                        _sync()
                        texts.add(out.download())
                        out.assert_clean()
                        ran += 1
                assert len(texts) == 1, (S, L, col0, row_align)
                text = texts.pop()
                lines = text.split(b"\n")
                assert text.endswith(b"\n") and len(lines) == 2 * S + 1, (S, L, row_align)
                assert all(ln.split()[0] == b">s%d" % i for i, ln in enumerate(lines[0:-1:2]))
                assert all(len(ln) == L for ln in lines[1::2])
                if row_align:
                    starts, at = [], 0
                    for i in range(S):
                        at += len(lines[2 * i]) + 1
                        starts.append(at)
                        at += L + 1
                    assert all(st % row_align == 0 for st in starts), (S, L, row_align)
                _eds, seds = o.msa(text, 0)                          # the oracle takes it; a variant segment lists all S rows
                ids = [int(t) for t in seds.replace(b"}{", b",").strip(b"{}").split(b",")]
                assert max(ids) in (0, S), (S, L, row_align)
            short = Arena(n - 1, 0xFF, name="one byte short")
            with pytest.raises(edsparser_amd.EdsxError) as ei:
                ctx.msa_synth_device(short.ptr, n - 1, S, L, row_align=row_align)
            assert ei.value.code == EDSX_ERR_INVALID_PARAMETER
            _sync()
            assert short.download() == b"\xff" * (n - 1)
            short.assert_clean()
    assert ran == len(GEN_S) * len(GEN_L) * 2 * 3 * 2
