"""The contract of the C ABI boundary (include/edsx.h, csrc/capi.hip), pinned through raw ctypes: the status a failure
maps to, the text it leaves, and what every out-parameter holds afterwards.  The Context wrappers raise before the
out-parameters can be looked at, so nothing here goes through them.

Before a failing call every out-parameter is filled with a sentinel: an edsx_buf with a non-null data pointer that is
never dereferenced and size 7, 0xff bytes in the structs, -1 in the ints.  Afterwards a buffer reads {NULL, 0}, a
struct is all zero and an int is 0."""
import ctypes
import json
import os

import pytest

import bgzf_spec as bz
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

MSA = b">a\nACGT\n>b\nAGGT\n"                                     # two rows, four columns
EDS, SEDS = b"{ACGT}{A,C}{GT}", b"{0}{1}{2}{0}"
SOURCE_COUNT = "sEDS: Source count (5) does not match EDS cardinality (6)"
U64_MAX = 2 ** 64 - 1


def _vcf_case():
    for c in json.load(open(os.path.join(GOLDEN, "gen_vcf.json")))["cases"]:
        if c["expect"].get("error") == SOURCE_COUNT:
            assert c["l"] == 1 and "chr1\t4\t.\tATT\tC" in c["vcf"] and "chr1\t11\t.\tT\tT" in c["vcf"]
            return c["vcf"].encode(), c["fasta"].encode()
    raise AssertionError("the fixture is gone")


VCF, FASTA = _vcf_case()


# ---- out-parameters: a factory per kind; each makes the sentinel-filled object of one call
class _Out:
    def __init__(self, obj, checked=True):
        self.obj, self.checked = obj, checked
        self.arg = ctypes.byref(obj)

    def cleared(self):
        if isinstance(self.obj, ctypes.Structure) and hasattr(self.obj, "data") and hasattr(self.obj, "size"):
            return (self.obj.data, self.obj.size) == (None, 0)
        return bytes(self.obj) == bytes(ctypes.sizeof(self.obj))


def _filled(cls, byte=0xff):
    obj = cls()
    ctypes.memset(ctypes.byref(obj), byte, ctypes.sizeof(obj))
    return obj


def BUF():
    from edsparser_amd._capi import _Buf
    return _Out(_Buf(0xdead0000, 7))


def _struct(name, checked):
    def make():
        from edsparser_amd import _capi
        return _Out(_filled(getattr(_capi, name)), checked)
    return make


VST, EST, RSC = _struct("VcfStats", True), _struct("EdsStatistics", True), _struct("EdsRangeScan", True)


def INT():
    return _Out(ctypes.c_int(-1))


def U64Z():
    return _Out(ctypes.c_uint64(U64_MAX))


def PTR():                                                          # a session handle: NULL after a failed open
    return _Out(ctypes.c_void_p(0xdead0000))


def free(cls_name=None, ctype=None):                                # an out-parameter the boundary does not clear
    def make():
        from edsparser_amd import _capi
        return _Out(_filled(getattr(_capi, cls_name)) if cls_name else ctype(), False)
    return make


U64, SZ, CINT = free(ctype=ctypes.c_uint64), free(ctype=ctypes.c_size_t), free(ctype=ctypes.c_int)


def MISS():
    return _Out((ctypes.c_uint64 * 8)(), False)


def IDS():
    return _Out((ctypes.c_uint64 * 1)(1), False)


def CONTIGS():
    from edsparser_amd._capi import Contig
    return _Out(ctypes.POINTER(Contig)(), False)


def NAME():
    return _Out(ctypes.c_char_p(), False)


V, F, E, Q = (VCF, len(VCF)), (FASTA, len(FASTA)), (EDS, len(EDS)), (SEDS, len(SEDS))

# (handle kind, function, arguments after the handle, index of the argument whose NULL is a "null argument" or None)
TABLE = [
    ("ctx", "edsx_msa_plan_device", [None, 0, 0, None, U64, U64], 4),
    ("ctx", "edsx_msa_emit_device", [None, None, None], 0),
    ("ctx", "edsx_msa_last_info", [free("MsaInfo")], None),
    ("ctx", "edsx_msa_edge_info", [free("MsaEdges")], 0),
    ("ctx", "edsx_msa_anchor_info", [1, free("MsaAnchors")], 1),
    ("ctx", "edsx_msa_copy_columns", [0, 1, None], 2),
    ("ctx", "edsx_msa_locate_segment", [0, U64, U64, U64, U64], 1),
    ("ctx", "edsx_msa_transform", [MSA, len(MSA), 0, BUF, BUF], 3),
    ("ctx", "edsx_msa_transform_batched", [MSA, len(MSA), 0, 2, BUF, BUF, INT], 4),
    ("ctx", "edsx_leds_merge", [*E, *Q, 1, 1, BUF, BUF], 6),
    ("ctx", "edsx_eds_stats", [*E, *Q, 0, EST], 5),
    ("ctx", "edsx_leds_merge_range", [*E, *Q, 1, 1, 0, 0, BUF, BUF, INT, INT], 10),
    ("ctx", "edsx_eds_genpatterns", [*E, 2, 3, 1, BUF, BUF, BUF, BUF], 5),
    ("ctx", "edsx_eds_check_positions", [*E, None, 0, 1, None, None, None, None, None, None], 10),
    ("ctx", "edsx_query_last_info", [free("QueryInfo")], None),
    ("ctx", "edsx_eds_scan_range", [*E, 0, len(EDS), 0, RSC], 5),
    ("ctx", "edsx_seds_scan_range", [*Q, 0, len(SEDS), None, 0, INT, U64Z, None, None], 6),
    ("ctx", "edsx_vcf_transform", [*V, *F, 0, BUF, BUF, VST], 5),
    ("ctx", "edsx_vcf_session_open", [*V, *F, PTR], 4),
    ("ctx", "edsx_vcf_transform_contig", [*V, *F, b"chr1", 0, BUF, BUF, VST], 6),
    ("ctx", "edsx_gz_inflate", [*V, BUF], 2),
    ("ctx", "edsx_gz_last_info", [0, free("GzInfo")], None),
    ("ctx", "edsx_vcf_session_open_z", [*V, *F, PTR], 4),
    ("ctx", "edsx_vcf_transform_z", [*V, *F, b"chr1", 0, BUF, BUF, VST], 6),
    ("ctx", "edsx_paths_open", [*E, *Q, PTR], 4),
    ("ctx", "edsx_eds_spell_paths", [*E, *Q, None, 0, None, None, 60, BUF, MISS], 9),
    ("ctx", "edsx_vcf_index", [*V, BUF, BUF, BUF, BUF, VST], 2),
    ("ctx", "edsx_vcf_transform_range", [*V, *F, 0, U64_MAX, BUF, BUF, VST], 6),
    ("ctx", "edsx_genrandomeds", [100, 0.1, 2, 4, 10, 0.7, b"ACGT", 0, 42, BUF, BUF, U64], 9),
    ("ctx", "edsx_genvcf", [100, 2, 2, 42, BUF, BUF], 4),
    ("ctx", "edsx_msa_synth_device", [None, 0, 1, 0, 1, 0.05, 42, None, SZ], None),
    ("ctx", "edsx_msa_synth_device_aligned", [None, 0, 1, 0, 1, 0.05, 42, 128, None, SZ], None),
    ("multi", "edsx_msa_transform_multi", [MSA, len(MSA), 0, BUF, BUF], None),       # (its null check reports no text)
    ("multi", "edsx_multi_last_partition", [CINT, CINT], None),
    ("multi", "edsx_vcf_transform_multi", [*V, *F, 0, BUF, BUF, VST], 5),
    ("multi", "edsx_multi_last_vcf", [free("VcfMultiInfo")], None),
    ("multi", "edsx_leds_merge_multi", [*E, *Q, 1, 1, BUF, BUF], 6),
    ("multi", "edsx_multi_last_merge", [free("MergeMultiInfo")], None),
    ("vcf_session", "edsx_vcf_session_contigs", [CONTIGS, SZ], None),
    ("vcf_session", "edsx_vcf_session_find", [b"chr1", SZ], 1),
    ("vcf_session", "edsx_vcf_session_transform", [0, 0, BUF, BUF, VST], 2),
    ("vcf_session", "edsx_vcf_session_info", [free("VcfSessionStats")], None),
    ("vcf_session", "edsx_vcf_session_unknown_contigs", [BUF], 0),
    ("vcf_session", "edsx_vcf_session_contig_name", [0, NAME, SZ], None),
    ("paths_session", "edsx_paths_info", [free("PathsInfo")], None),
    ("paths_session", "edsx_paths_lengths", [IDS, 1, MISS, MISS], 2),
    ("paths_session", "edsx_paths_spell", [None, 0, None, None, 60, BUF, MISS], 5),
    ("paths_session", "edsx_paths_last_timing", [free("PathsTiming")], None),
]
IDS_OF = [row[1] for row in TABLE]


def _call(lib, handle, fn, args, null=None):
    """-> (status, the out-parameters of this call); argument `null` is passed as NULL"""
    outs, real = [], []
    for i, a in enumerate(args):
        if callable(a):
            a = a()
        if i == null:
            a = None
        elif isinstance(a, _Out):
            outs.append(a)
            a = a.arg
        real.append(a)
    return getattr(lib, fn)(handle, *real), outs


@pytest.fixture(scope="module")
def lib():
    import edsparser_amd
    return edsparser_amd.load_library()


@pytest.fixture(scope="module")
def handles(lib):
    """One valid handle of every kind; the multi handle is one device with the in-process exchange."""
    h = {k: ctypes.c_void_p() for k in ("ctx", "multi", "vcf_session", "paths_session")}
    assert lib.edsx_ctx_create(0, ctypes.byref(h["ctx"])) == 0
    assert lib.edsx_multi_create((ctypes.c_int * 1)(0), 1, 0, ctypes.byref(h["multi"])) == 0
    assert lib.edsx_vcf_session_open(h["ctx"], *V, *F, ctypes.byref(h["vcf_session"])) == 0
    assert lib.edsx_paths_open(h["ctx"], *E, *Q, ctypes.byref(h["paths_session"])) == 0
    yield h
    lib.edsx_paths_close(h["paths_session"])
    lib.edsx_vcf_session_close(h["vcf_session"])
    lib.edsx_multi_destroy(h["multi"])
    lib.edsx_ctx_destroy(h["ctx"])


def _error(lib, handles, kind):
    if kind == "multi":
        return lib.edsx_multi_last_error(handles["multi"]).decode()
    return lib.edsx_last_error(handles["ctx"]).decode()


@pytest.mark.parametrize("kind,fn,args,null", TABLE, ids=IDS_OF)
def test_null_handle(lib, kind, fn, args, null):
    rc, outs = _call(lib, None, fn, args)
    assert rc == 3
    for o in outs:
        assert not o.checked or o.cleared(), (fn, type(o.obj).__name__, bytes(o.obj))


@pytest.mark.parametrize("kind,fn,args,null", [r for r in TABLE if r[3] is not None], ids=[r[1] for r in TABLE if r[3] is not None])
def test_null_output(lib, handles, kind, fn, args, null):
    rc, outs = _call(lib, handles[kind], fn, args, null)
    assert rc == 3 and _error(lib, handles, kind) == "null argument"
    for o in outs:
        assert not o.checked or o.cleared(), (fn, type(o.obj).__name__, bytes(o.obj))


def test_null_output_of_the_multi_msa_transform_reports_no_text(lib, handles):
    """edsx_msa_transform_multi checks its pointers before it clears the handle's text: 3, and the text of the call
    before stays."""
    rc, outs = _call(lib, handles["multi"], "edsx_msa_transform_multi", [MSA, 0, 0, BUF, BUF])
    assert rc == 2 and _error(lib, handles, "multi") == "Invalid MSA: empty input"
    rc, outs = _call(lib, handles["multi"], "edsx_msa_transform_multi", [MSA, len(MSA), 0, BUF, BUF], 3)
    assert rc == 3 and _error(lib, handles, "multi") == "Invalid MSA: empty input"
    assert all(o.cleared() for o in outs)


@pytest.mark.parametrize("kind,fn,args", [("ctx", "edsx_msa_transform", [MSA, 0, 0, BUF, BUF]),
                                          ("ctx", "edsx_msa_transform_batched", [MSA, 0, 0, 2, BUF, BUF, INT]),
                                          ("multi", "edsx_msa_transform_multi", [MSA, 0, 0, BUF, BUF])],
                         ids=["edsx_msa_transform", "edsx_msa_transform_batched", "edsx_msa_transform_multi"])
def test_empty_msa(lib, handles, kind, fn, args):
    rc, outs = _call(lib, handles[kind], fn, args)
    assert rc == 2 and _error(lib, handles, kind) == "Invalid MSA: empty input"
    assert all(o.cleared() for o in outs)


# ---- VCF counters on failure: (vcf, fasta, l) -> (status, text, the five counters)
COUNTER_NAMES = ("total_variants", "processed_variants", "skipped_malformed", "skipped_unsupported_sv", "variant_groups")
VCF_FAILURES = {
    # the merge refuses the EDS text: every counter is out by then, variant_groups included
    "merge": ((VCF, FASTA, 1), (2, SOURCE_COUNT, (2, 2, 0, 0, 2))),
    # nothing parsed yet
    "before_parse": ((VCF, b">chr1 test\n", 0), (2, "FASTA file is empty", (0, 0, 0, 0, 0))),
    # the transform refuses the reference after its tokeniser has counted the records
    "after_parse": ((VCF, b">chr1 test\n\nACGT\n", 0), (2, "Invalid FASTA format: empty first sequence line", (2, 2, 0, 0, 0))),
}


def _vcf_failure(lib, handles, entry, vcf, fasta, l):
    if entry == "edsx_vcf_transform":
        rc, outs = _call(lib, handles["ctx"], entry, [vcf, len(vcf), fasta, len(fasta), l, BUF, BUF, VST])
        text = _error(lib, handles, "ctx")
    elif entry == "edsx_vcf_transform_multi":
        rc, outs = _call(lib, handles["multi"], entry, [vcf, len(vcf), fasta, len(fasta), l, BUF, BUF, VST])
        text = _error(lib, handles, "multi")
    else:                                                           # a session on these inputs, record 0
        s = ctypes.c_void_p()
        rc = lib.edsx_vcf_session_open(handles["ctx"], vcf, len(vcf), fasta, len(fasta), ctypes.byref(s))
        text = _error(lib, handles, "ctx")
        # (a FASTA that the open refuses leaves no session: the transform then clears its outputs for the null handle)
        rc2, outs = _call(lib, s, entry, [0, l, BUF, BUF, VST])
        if rc == 0:
            rc, text = rc2, _error(lib, handles, "ctx")
        lib.edsx_vcf_session_close(s)
    eds, seds, st = outs
    assert eds.cleared() and seds.cleared()
    return rc, text, tuple(int(getattr(st.obj, n)) for n in COUNTER_NAMES)


@pytest.mark.parametrize("entry", ["edsx_vcf_transform", "edsx_vcf_session_transform", "edsx_vcf_transform_multi"])
@pytest.mark.parametrize("case", list(VCF_FAILURES))
def test_vcf_counters_on_failure(lib, handles, case, entry):
    (vcf, fasta, l), want = VCF_FAILURES[case]
    got = _vcf_failure(lib, handles, entry, vcf, fasta, l)
    print(case, entry, got)
    assert got == want


# ---- exception classes on the multi handle: FormatError -> 2, ParamError -> 3, LimitError -> 4
def _class_inputs():
    return {"format": ("msa", b"ACGT\n"), "param": ("merge", 0),                  # (a merge with context length 0)
            "limit": ("msa", b">\nA\n" * 10_000_000)}                           # (tests/test_msa_gpu.py: the build's row limit)


def _fail(lib, handle, multi, kind, arg):
    suffix = "_multi" if multi else ""
    if kind == "msa":
        rc, outs = _call(lib, handle, "edsx_msa_transform" + suffix, [arg, len(arg), 0, BUF, BUF])
    else:
        rc, outs = _call(lib, handle, "edsx_leds_merge" + suffix, [*E, *Q, arg, 1, BUF, BUF])
    assert all(o.cleared() for o in outs)
    return rc, (lib.edsx_multi_last_error if multi else lib.edsx_last_error)(handle).decode()


@pytest.fixture(scope="module")
def class_failures(lib, handles):
    """name -> (input, (status, text) of the single-GPU entry point)"""
    return {name: (inp, _fail(lib, handles["ctx"], False, *inp)) for name, inp in _class_inputs().items()}


def test_exception_classes_single_gpu(class_failures):
    assert class_failures["format"][1] == (2, "Invalid MSA: expected a FASTA header line starting with '>'")
    assert class_failures["param"][1] == (3, "context_length must be > 0 for l-EDS transformation")
    assert class_failures["limit"][1] == (4, "MSA has more sequences than this build supports (9999999)")


@pytest.mark.parametrize("ranks", [1, 2])
def test_exception_classes_on_the_multi_handle(lib, class_failures, ranks):
    """The code and the text of the single-GPU entry point, through one rank and through two ranks that share device 0
    (in-process exchange)."""
    multi = ctypes.c_void_p()
    assert lib.edsx_multi_create((ctypes.c_int * ranks)(*[0] * ranks), ranks, 0, ctypes.byref(multi)) == 0
    try:
        for name, (inp, want) in class_failures.items():
            got = _fail(lib, multi, True, *inp)
            print(name, ranks, got)
            assert got == want, name
    finally:
        lib.edsx_multi_destroy(multi)


# ---- success
@pytest.mark.parametrize("kind,fn,args", [r[:3] for r in TABLE if BUF in r[2]], ids=[r[1] for r in TABLE if BUF in r[2]])
def test_success(lib, handles, kind, fn, args):
    rc, outs = _call(lib, handles[kind], fn, args)
    assert rc == 0 and _error(lib, handles, kind) == ""
    bufs = [o for o in outs if hasattr(o.obj, "data")]
    assert bufs
    for b in bufs:
        lib.edsx_buf_free(b.arg)
        assert b.cleared()


def test_bgzf_index_without_a_context(lib):
    """edsx_bgzf_index takes no context: the block table of a BGZF file, 2 and cleared outputs for anything else, 3 and
    cleared outputs for a null argument."""
    from edsparser_amd._capi import BgzfBlock
    data, table = bz.write(VCF)
    blocks, n = BUF(), U64Z()
    assert lib.edsx_bgzf_index(data, len(data), blocks.arg, n.arg) == 0
    assert blocks.obj.size == len(table) * ctypes.sizeof(BgzfBlock) and n.obj.value == len(VCF)
    lib.edsx_buf_free(blocks.arg)
    assert blocks.cleared()
    for args, want in (((VCF, len(VCF)), 2), ((None, 1), 3)):
        blocks, n = BUF(), U64Z()
        assert lib.edsx_bgzf_index(*args, blocks.arg, n.arg) == want
        assert blocks.cleared() and n.cleared()
