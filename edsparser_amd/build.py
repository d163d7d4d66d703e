"""Build libedsx.so (HIP kernels + C ABI) for gfx950 with hipcc, in-tree.

One object per source under edsparser_amd/build/ (compiled in parallel, only when stale), then one link; three more
libraries for the tests only (libedsx_smallstacks.so, libedsx_guard.so, libedsx_weakhash.so) relink the same objects
with one source each compiled with other flags, and a fifth and a sixth (libedsx_primitives.so, libedsx_msagroup.so) are one
translation unit of the tests' own each.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "libedsx.so")
SOURCES = ["dev_alloc.hip", "msa_device.hip", "msa_scan.hip", "eds_device.hip", "merge_device.hip", "merge_scan.hip", "vcf_device.hip", "vcf_contig.hip", "bgzf_device.hip", "synth.hip", "genrandom.hip", "genvcf.hip", "multi_gpu.hip", "vcf_multi.hip", "merge_multi.hip", "query_device.hip", "locate_device.hip", "path_device.hip", "lift_device.hip", "subset_device.hip", "slice_device.hip", "dist_device.hip", "ld_device.hip", "ibs_device.hip", "mosaic_device.hip", "div_device.hip", "gfa_device.hip", "vcf_export_device.hip", "capi.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
# per-source flags.  msa_scan.hip: machine scheduler off - the column scan's loads stay in source order (bench shape: scan
# 26.5 instead of 26.9 ms; the same flag on msa_device.hip costs its emitters 0.2 ms: alternating A/B runs, EXPERIMENTS.md)
EXTRA_FLAGS = {"msa_scan.hip": ["-mllvm", "-enable-misched=false"]}
# A second library for the tests only: the merge's final-text kernel with a 256-entry LDS stack and a 2-entry register stack
# in its serial walk, so that ordinary inputs take the overflow -> serial walk -> HBM spill-stack path that otherwise needs
# merge trees deeper than 96 (tests/test_merge_gpu.py::test_deep_tree_fallback_paths).  Never loaded by the product.
TEST_LIB = os.path.join(HERE, "libedsx_smallstacks.so")
TEST_FLAGS = {"merge_device.hip": ["-DEDSX_EXPERIMENTS", "-DEDSX_FW_STACK=256", "-DEDSX_FIN_STACK=2"]}
# A third one, also for the tests only: every DevBuf between two 64 KiB zones of known bytes that are looked at after each
# call (csrc/dev_alloc.hip with -DEDSX_GUARD, tests/test_guard_gpu.py).  Never loaded by the product.
GUARD_LIB = os.path.join(HERE, "libedsx_guard.so")
GUARD_FLAGS = {"dev_alloc.hip": ["-DEDSX_GUARD"]}
# A fourth one, also for the tests only: the MSA grouping with every hash of its hash-then-compare sites cut to ONE bit
# (msa_hash() in csrc/msa_wave.hpp), so that of any three distinct strings two share a hash and the byte compares behind
# the hashes decide over real collisions (tests/test_msa_weakhash_gpu.py).  Never loaded by the product.
WEAKHASH_LIB = os.path.join(HERE, "libedsx_weakhash.so")
WEAKHASH_FLAGS = {"msa_device.hip": ["-DEDSX_MSA_HASH_BITS=1"]}
# A fifth one, also for the tests only: plain C launchers around the shared device primitives of csrc/dev_util.hpp and
# csrc/byte_ops.hpp (scans, set-id text, bisection, 16-byte and wave helpers, the pinned download), one translation unit
# linked on its own (tests/hip/primitives_harness.hip, tests/test_primitives_gpu.py).  Never loaded by the product.
PRIM_LIB = os.path.join(HERE, "libedsx_primitives.so")
PRIM_SRC = os.path.join(HERE, "..", "tests", "hip", "primitives_harness.hip")
# A sixth one, built the same way: plain C launchers around the wave64 grouping code of the MSA transform - the helpers of
# csrc/msa_wave.hpp, fast_group of csrc/msa_fast_kernels.hpp and fused_group_run of csrc/msa_scan_kernels.hpp, called on
# segments of the tests' own (tests/hip/msa_group_harness.hip, tests/test_msa_group_gpu.py).  Never loaded by the product.
MSAGROUP_LIB = os.path.join(HERE, "libedsx_msagroup.so")
MSAGROUP_SRC = os.path.join(HERE, "..", "tests", "hip", "msa_group_harness.hip")


def _headers():
    hs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    hs.append(os.path.join(HERE, "..", "include", "edsx.h"))
    return hs


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _compile(src, obj, extra, verbose):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + FLAGS + extra + ["-c", src, "-o", obj]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)


def _link(objs, lib, verbose):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", lib] + objs + ["-L/opt/rocm/lib", "-lrccl", "-Wl,-rpath,/opt/rocm/lib"]   # RCCL: the multi-GPU boundary stitch
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)


def build(force=False, verbose=False):
    os.makedirs(OBJ, exist_ok=True)
    hdrs = _headers()
    sources = [s for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    jobs = []
    objs = []
    for s in sources:
        src, obj = os.path.join(CSRC, s), os.path.join(OBJ, s.replace(".hip", ".o"))
        objs.append(obj)
        if force or _newer(obj, [src] + hdrs):
            jobs.append((src, obj, EXTRA_FLAGS.get(s, [])))
    if jobs:
        with ThreadPoolExecutor(max_workers=min(6, len(jobs))) as ex:
            list(ex.map(lambda j: _compile(j[0], j[1], j[2], verbose), jobs))
    if force or _newer(LIB, objs):
        _link(objs, LIB, verbose)
    for lib, tag, flags in ((TEST_LIB, "smallstacks", TEST_FLAGS), (GUARD_LIB, "guard", GUARD_FLAGS),
                           (WEAKHASH_LIB, "weakhash", WEAKHASH_FLAGS)):
        tobjs = list(objs)
        for name, extra in flags.items():
            src, obj = os.path.join(CSRC, name), os.path.join(OBJ, name.replace(".hip", ".%s.o" % tag))
            tobjs[tobjs.index(os.path.join(OBJ, name.replace(".hip", ".o")))] = obj
            if force or _newer(obj, [src] + hdrs):
                _compile(src, obj, EXTRA_FLAGS.get(name, []) + extra, verbose)
        if force or _newer(lib, tobjs):
            _link(tobjs, lib, verbose)
    for src, lib in ((PRIM_SRC, PRIM_LIB), (MSAGROUP_SRC, MSAGROUP_LIB)):
        if os.path.exists(src) and (force or _newer(lib, [src] + [h for h in hdrs if h.endswith(".hpp")])):
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            cmd = [hipcc] + FLAGS + ["-I", CSRC, "-shared", src, "-o", lib, "-Wl,-rpath,/opt/rocm/lib"]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            subprocess.run(cmd, check=True)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
