"""GPU: the diversity through `libedsx_guard.so` (tests/div_guard_child.py, in a child process as tests/test_ld_guard_gpu.py
starts its child): the boundary shapes of tests/test_div_gpu.py, a fresh context per fill byte, the specification's result
under every fill and no guard zone written."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "edsparser_amd", "libedsx_guard.so")


def test_guard_div():
    assert os.path.exists(LIB), "python -m edsparser_amd.build builds it"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "div_guard_child.py"), "div"], capture_output=True, text=True,
                       env=dict(os.environ, EDSX_LIB=LIB), timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    m = re.search(r"^guard div: cases (\d+) runs (\d+) allocations (\d+) guarded_bytes (\d+) checks (\d+)", r.stdout, re.M)
    assert m, r.stdout[-3000:]
    print(m.group(0))
    cases, runs, allocations, guarded, checks = map(int, m.groups())
    assert cases >= 10 and runs == 5 * cases and allocations > 0 and guarded > 0 and checks >= 2 * runs, m.group(0)
