"""Out-of-buffer device accesses, which byte-equality with the oracle cannot see: every test here starts one child process
that loads `libedsx_guard.so` through EDSX_LIB (built by edsparser_amd.build for the tests only: every DevBuf between two
64 KiB zones of known bytes, zones and payload filled with a byte the child chooses, csrc/dev_alloc.hip with -DEDSX_GUARD).
The child (tests/guard_child.py) runs each case on a fresh context once per fill byte, compares with the oracle and asserts
that no zone was written, after the call and after the context is closed.  DESIGN.md section 2.1 says what this sees and
what it cannot see."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "edsparser_amd", "libedsx_guard.so")


def _child(name, min_cases, timeout=600, env=None):
    assert os.path.exists(LIB), "python -m edsparser_amd.build builds it"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "guard_child.py"), name], capture_output=True, text=True,
                       env=dict(os.environ, EDSX_LIB=LIB, **(env or {})), timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    m = re.search(r"^guard %s: cases (\d+) runs (\d+) allocations (\d+) guarded_bytes (\d+) checks (\d+)" % name, r.stdout, re.M)
    assert m, r.stdout[-3000:]
    print(m.group(0))
    cases, runs, allocations, guarded, checks = map(int, m.groups())
    assert cases >= min_cases and runs >= cases and allocations > 0 and guarded > 0 and checks >= 2 * runs, m.group(0)
    return r


def test_guard_selftest():
    """The checker checks: planted bytes at payload offsets N and -1 are reported at exactly those offsets, the in-bounds
    store at N-1 is not; with EDSX_GUARD_TRACE=1 every allocation is one stderr line with its serial number and call site."""
    r = _child("selftest", 36, timeout=120, env={"EDSX_GUARD_TRACE": "1"})
    assert " back zone, offsets +0..+0," in r.stdout and " front zone, offsets -1..-1," in r.stdout
    serials = [int(x) for x in re.findall(r"^edsx-guard: alloc #(\d+) \d+ bytes from \S+\+0x[0-9a-f]+", r.stderr, re.M)]
    assert serials and serials == list(range(1, len(serials) + 1)), r.stderr[-2000:]
    assert "edsx-guard: alloc #1 1 bytes from libedsx_guard.so+0x" in r.stderr


def test_guard_msa():
    _child("msa", 280)


def test_guard_vcf():
    _child("vcf", 77)


def test_guard_merge():
    _child("merge", 155)


def test_guard_eds_consumers():
    _child("eds_consumers", 120)


def test_guard_multi_rank_one_device():
    _child("multi_rank_one_device", 3)


def test_guard_contig_edges():
    """the FASTA index and the classification at lane, block and buffer ends (tests/contig_walk_cases.py): a dozen shifts
    of the sweep, the ends, the long walks and K = 256"""
    _child("contig_edges", 69)
