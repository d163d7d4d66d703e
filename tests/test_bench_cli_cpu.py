"""bench.py without a GPU: its options and the --dump-outputs reductions (on host tensors)."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_help_names_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def _blocks_ref(host, n, blocks):
    bs = max(1, -(-n // blocks))
    out = []
    for b0 in range(0, n, bs):
        blk = host[b0:min(n, b0 + bs)].astype(np.int64)
        out.append([blk.sum(), (blk * np.arange(1, blk.size + 1)).sum()])
    return np.array(out, dtype=np.float64).reshape(-1, 2)


def test_dump_sample_and_block_digest():
    rng = np.random.default_rng(1)
    for n, blocks, cap in [(0, 16, 8), (5, 16, 8), (1000, 16, 64), (1000003, 65536, 4096), (12345, 7, 100)]:
        host = rng.integers(0, 256, size=n + 16, dtype=np.uint8)   # + the 16 bytes of slack the bench allocates
        v = torch.from_numpy(host)
        d = bench._block_digest(torch, v, n, blocks)
        assert d.dtype == np.float64 and np.array_equal(d, _blocks_ref(host, n, blocks)), n
        s = bench._sample(torch, v, n, cap)
        assert s.dtype == np.float32 and s.size == min(n, cap), n
        if n <= cap:
            assert np.array_equal(s, host[:n])
        else:
            k = cap // 4
            assert np.array_equal(s[:k], host[:k]) and np.array_equal(s[-k:], host[n - k:n])
            assert np.array_equal(s, bench._sample(torch, v, n, cap))          # fixed by the size alone
