"""GPU: the edsparser::eds_to_gfa shim (tests/cpp/test_gfa.cpp), built against the host library as
tests/test_host_cpp.py builds its programs."""
import os
import subprocess

import pytest

from test_paths_cpu import BUILD, HOST, INC, LIBDIR, ROOT


@pytest.mark.gpu
def test_eds_to_gfa_cpp_shim():
    subprocess.run(["make", "-s", "-C", HOST], check=True)        # (libedsx.so itself comes from build())
    exe = os.path.join(BUILD, "test_gfa")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", INC, os.path.join(ROOT, "tests", "cpp", "test_gfa.cpp"),
                    os.path.join(BUILD, "libedsparser_lib.a"), "-L", LIBDIR, "-ledsx", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr
