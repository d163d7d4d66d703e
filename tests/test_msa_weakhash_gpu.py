"""The hash-then-compare sites of the MSA grouping over real collisions.  With full-width hashes
the byte compares behind the hashes never have to say "no"; libedsx_weakhash.so (built by edsparser_amd.build for the tests
only: csrc/msa_device.hip with -DEDSX_MSA_HASH_BITS=1) keeps one bit of every such hash, and the directed cases of
tests/msa_collision_cases.py hold three distinct strings per segment, so two of them collide whatever the hash is.

Every weak-library test starts ONE child process (tests/msa_weakhash_child.py) that loads the library through EDSX_LIB,
compares .eds and .seds byte for byte with the oracle at l = 0 and l = 3, and checks the route through
msa_info()["n_slow_segments"]; the parent checks the heavy work list through the EDSX_COUNTS line of every case.  The same
cases run on the product library in this process: a failure on both sides is the kernels', one on the weak side alone is a
compare's."""
import os
import re
import subprocess
import sys

import pytest

import msa_collision_cases as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "edsparser_amd", "libedsx_weakhash.so")


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    c = edsparser_amd.Context(0)
    yield c
    c.close()


def _child(name, timeout=300):
    """one child, started once; -> (cases, runs, stderr)"""
    assert os.path.exists(LIB), "python -m edsparser_amd.build builds it"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "msa_weakhash_child.py"), name], capture_output=True, text=True,
                       env=dict(os.environ, EDSX_LIB=LIB, EDSX_COUNTS="1"), timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    m = re.search(r"^weakhash %s: cases (\d+) runs (\d+) seconds ([0-9.]+)" % name, r.stdout, re.M)
    assert m, r.stdout[-2000:]
    print(m.group(0))
    return int(m.group(1)), int(m.group(2)), r.stderr


def _check_heavy(stderr, family):
    """Every case's marker line is followed by the library's count line of that plan.  Up to 1024 rows and without the
    column scan's fused grouping (l > 0), the heavy work list holds exactly the segments of 11..64 columns and the mixed
    ones - those that reach the one-row-per-lane branch and the root join."""
    lines = stderr.splitlines()
    seen = checked = 0
    for i, line in enumerate(lines):
        m = re.match(r"weakhash-case (\S+) l=(\d+) rows=(\d+) slow=(\d+) heavy=(\d+)$", line)
        if not m:
            continue
        seen += 1
        assert i + 1 < len(lines), line
        c = re.match(r"\[edsx\] segments \d+ variant (\d+) \| grouping list \d+ heavy (\d+) \|", lines[i + 1])
        assert c, (line, lines[i + 1])
        if int(m.group(2)) > 0 and int(m.group(3)) <= 1024:
            assert int(c.group(2)) == int(m.group(5)), (line, lines[i + 1])
            checked += 1
    assert seen == 2 * len(mc.cases(family)), (seen, family)
    return checked


@pytest.mark.parametrize("family", mc.FAMILIES)
def test_weak_hash_directed(family):
    cases, runs, stderr = _child(family)
    assert cases == len(mc.cases(family)) and cases > 0 and runs == 2 * cases, (cases, runs)
    checked = _check_heavy(stderr, family)
    assert checked == sum(1 for c in mc.cases(family) if c.S <= 1024), checked


@pytest.mark.parametrize("family", mc.FAMILIES)
def test_product_library_directed(ctx, family):
    """the same cases and expectations with full-width hashes"""
    import edsparser_amd
    from msa_weakhash_child import run_family
    assert os.path.basename(edsparser_amd._capi.lib_path()) != os.path.basename(LIB)
    cases, runs = run_family(ctx, family)
    assert cases == len(mc.cases(family)) and runs == 2 * cases


@pytest.mark.parametrize("name,expect", [("wide", 48), ("wide_nul", 48), ("campaign", 48)])
def test_weak_hash_seeded_generators(name, expect):
    """the suite's seeded generators (tests/msa_cases.py) under one-bit hashes"""
    cases, runs, _ = _child(name)
    assert cases == expect and runs == expect, (cases, runs)
