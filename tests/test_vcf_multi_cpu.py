"""CPU side of the C++ multi-GPU VCF path: the rank barrier that carries a failure to every rank thread
(edsparser_amd/csrc/rank_barrier.hpp, driven by tests/cpp/test_rank_barrier.cpp) and vcf2eds's --gpus option, which is
checked before any file or device is touched."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "edsparser_amd", "csrc")


def test_rank_barrier_failure_reaches_every_rank(tmp_path):
    exe = str(tmp_path / "test_rank_barrier")
    subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "test_rank_barrier.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)      # a lost rank hangs: the timeout fails it
    assert r.returncode == 0, r.stderr
    assert "rank barrier ok" in r.stdout


def _vcf2eds():
    from test_host_cpp import BUILD, _build_host
    _build_host()
    return os.path.join(BUILD, "vcf2eds")


def test_vcf2eds_help_lists_gpus():
    r = subprocess.run([_vcf2eds(), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    assert "--gpus" in r.stdout


def test_vcf2eds_gpus_out_of_range(tmp_path):
    # the files do not exist and no device is visible: the option is refused before either is looked at
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    for bad in ("0", "65"):
        r = subprocess.run([_vcf2eds(), "-i", str(tmp_path / "none.vcf"), "-r", str(tmp_path / "none.fa"), "--gpus", bad],
                           capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 1
        assert "--gpus must be between 1 and 64" in r.stderr
        assert "not found" not in r.stderr
        assert not (tmp_path / "none.eds").exists()
