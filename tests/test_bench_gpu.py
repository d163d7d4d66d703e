"""bench.py as the driver starts it for N > 1 (torch.distributed.run, one rank per GPU), rehearsed on the one-GPU box:
two ranks sharing the card over gloo (the multi-rank logic: slabs, stitch, reductions, one JSON line from rank 0), and the
production backend (nccl = RCCL) with the single rank the box allows (--force-dist: process group on the device, the
stitcher's tensor collectives and the all_reduces on device tensors)."""
import json
import os
import subprocess
import sys

import pytest

from test_vcf_shard_cpu import _free_port

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--steps", "2", "--warmup", "1", "--cols", "4000000", "--cpu-baseline-mb", "0", "--verify", "0"]


def _run(nproc, extra):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", str(nproc)] + COMMON + extra
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                  # rank 0 prints ONE line
    return json.loads(lines[0])


def test_two_ranks_share_the_gpu_over_gloo():
    j = _run(2, ["--backend", "gloo", "--share-gpu"])
    assert j["n_gpus"] == 2 and j["scaling"] == "strong" and j["metric"] == "msa2eds_input_MB_per_s"
    assert j["config"]["cols_total"] == 4000000 and j["config"]["cols_per_gpu"] == 2000000
    assert j["value"] > 0 and j["steps"] == 2 and j["warmup"] == 1
    assert j["config"]["stitch"] == 1                         # one boundary between the two slabs: one chain


def test_rccl_single_rank_takes_the_multi_rank_path():
    j = _run(1, ["--backend", "nccl", "--force-dist"])
    assert j["n_gpus"] == 1 and j["value"] > 0 and j["config"]["stitch"] is not None


# ---- bench.py as one process on one GPU: the plain run, --dump-outputs and --full ----

SMALL = ["--rows", "64", "--cols", "100000"]                # E and Q stay below bench.DUMP_WHOLE: dumped whole


def _single(args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_what_the_last_step_computed(tmp_path):
    import numpy as np
    import torch
    import bench
    import edsparser_amd
    import oracle_lib
    j = _single(["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)] + SMALL)
    assert j["metric"] == "msa2eds_input_MB_per_s" and j["unit"] == "MB/s" and j["higher_is_better"] is True
    assert j["dtype"] == "u8" and j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
    assert j["verify"] is None and j["aligned_rows"] is None and j["cpu_baseline"] is None   # --full only
    E, Q = j["config"]["eds_bytes"], j["config"]["seds_bytes"]
    assert 0 < E <= bench.DUMP_WHOLE and 0 < Q <= bench.DUMP_WHOLE
    sizes = np.load(tmp_path / "sizes.npy")
    assert sizes.dtype == np.float64 and sizes.tolist() == [E, Q]
    S, L = 64, 100000
    n = edsparser_amd.synth_size(S, L)
    buf = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    edsparser_amd.Context(0).msa_synth_device(buf.data_ptr(), n, S, L, variant_fraction=0.05, seed=42)
    torch.cuda.synchronize()
    want = dict(zip(("eds", "seds"), oracle_lib.msa(bytes(buf.cpu().numpy()), 0)))
    for name, ref in want.items():
        got = np.load(tmp_path / (name + ".npy"))
        assert got.dtype == np.float32 and got.astype(np.uint8).tobytes() == ref, name
        blocks = np.load(tmp_path / (name + "_blocks.npy"))
        assert blocks.dtype == np.float64 and blocks.shape[1] == 2 and blocks[:, 0].sum() == got.astype(np.float64).sum(), name


def test_dump_of_a_large_output_is_a_fixed_sample(tmp_path):
    import numpy as np
    import bench
    args = ["--steps", "1", "--warmup", "1", "--cols", "4000000"]
    runs = []
    for d in ("a", "b"):
        runs.append(_single(args + ["--dump-outputs", str(tmp_path / d)]))
    Q = runs[0]["config"]["seds_bytes"]
    assert Q > bench.DUMP_WHOLE and runs[1]["config"]["seds_bytes"] == Q
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) == ["eds.npy", "eds_blocks.npy", "seds.npy", "seds_blocks.npy",
                                                           "sizes.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / nm) for nm in names) <= 64 << 20
    for nm in names:                                          # same arguments, same inputs: the same arrays
        assert np.array_equal(np.load(tmp_path / "a" / nm), np.load(tmp_path / "b" / nm)), nm
    seds = np.load(tmp_path / "a" / "seds.npy")
    blocks = np.load(tmp_path / "a" / "seds_blocks.npy")
    assert seds.size == bench.DUMP_WHOLE and blocks.shape[0] <= bench.DUMP_BLOCKS
    bs = -(-Q // bench.DUMP_BLOCKS)                           # the sample's head holds the first block whole
    assert bs <= bench.DUMP_WHOLE // 4
    head = seds[:bs].astype(np.float64)
    assert blocks[0, 0] == head.sum() and blocks[0, 1] == (head * np.arange(1, bs + 1)).sum()


def test_full_run_keeps_the_oracle_check_aligned_rows_and_cpu_baseline():
    j = _single(["--steps", "2", "--warmup", "1", "--full", "--cpu-baseline-mb", "20"] + SMALL)
    assert j["verify"]["windows"] > 0 and j["verify"]["size_rule"] == "ok"
    assert j["aligned_rows"]["outputs_equal_headline_run"] is True and j["aligned_rows"]["ms_per_step"] > 0
    assert j["cpu_baseline"]["value"] > 0 and j["cpu_baseline"]["unit"] == "MB/s"
