"""Child program of tests/test_vcf_export_guard_gpu.py: `python vcf_export_guard_child.py vcf` with
EDSX_LIB=libedsx_guard.so.  The VCF export's boundary shapes (tests/test_vcf_export_gpu.py) through the guard library, as
tests/gfa_guard_child.py runs the GFA export: a fresh context per fill byte, the result equal to the specification's under
every fill, no zone dirty after the call or after close.  The emitters store aligned 16-byte chunks: a chunk past the end
of the body or of the FASTA, or in front of them, lands in a zone."""
import sys

from guard_child import EDS_FILLS, Guard                                  # (puts the repository and tests/ on sys.path)

from test_vcf_export_gpu import BOUNDARY, library, spec  # noqa: E402

VCF_EXPORT_FILLS = EDS_FILLS + (ord("\t"), ord("/"))


def vcf():
    g = Guard()
    for name, eds, seds, kw in BOUNDARY:
        g.case(name, lambda ctx: library(ctx, eds, seds, kw), spec(eds, seds, kw), VCF_EXPORT_FILLS)
    g.finish("vcf", len(BOUNDARY))


if __name__ == "__main__":
    {"vcf": vcf}[sys.argv[1]]()
