"""Child program of tests/test_msa_export_guard_gpu.py: `python msa_export_guard_child.py msa` with
EDSX_LIB=libedsx_guard.so.  The alignment export's boundary shapes (tests/test_msa_export_gpu.py) through the guard library,
as tests/vcf_export_guard_child.py runs the VCF export: a fresh context per fill byte, the result equal to the
specification's under every fill, no zone dirty after the call or after close.  k_path_align stores 16-byte chunks at any
byte address: a chunk past the end of the text, or a gap run that does not stop at the row's end, lands in a zone; a fill
equal to the case's gap byte hides nothing but the gaps, so whatever else is missing shows."""
import sys

from guard_child import EDS_FILLS, Guard                                  # (puts the repository and tests/ on sys.path)

from test_msa_export_gpu import BOUNDARY, library, spec  # noqa: E402

MSA_EXPORT_FILLS = EDS_FILLS + (ord("-"),)


def fills(kw):
    """the common fills, and the case's own gap byte: a gap that was never stored shows only under another fill, a gap
    stored where none belongs only under this one"""
    g = ord(kw.get("gap", "-"))
    return MSA_EXPORT_FILLS + (() if g in MSA_EXPORT_FILLS else (g,))


def msa():
    g = Guard()
    for name, eds, seds, kw in BOUNDARY:
        g.case(name, lambda ctx: library(ctx, eds, seds, kw), spec(eds, seds, kw), fills(kw))
    g.finish("msa", len(BOUNDARY))


if __name__ == "__main__":
    {"msa": msa}[sys.argv[1]]()
