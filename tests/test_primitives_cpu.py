"""csrc/byte_ops.hpp as host code: ne_bytes4 / eq_byte4 against a byte loop (every value pair of every byte position, a
million random dwords, the values around the carry of the 0x7f trick) and ndigits against snprintf at every power of ten,
in tests/cpp/test_byte_ops.cpp under ASan and UBSan.  tests/test_primitives_gpu.py runs the device compilation of the same
header over the same structured cases."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_byte_ops_host(tmp_path):
    exe = str(tmp_path / "test_byte_ops")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-I", os.path.join(ROOT, "edsparser_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_byte_ops.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    m = re.search(r"^byte_ops ok: (\d+) checks$", r.stdout, re.M)
    assert m and int(m.group(1)) >= 4 * 65536 + 1000000 + 30, r.stdout[-2000:]
