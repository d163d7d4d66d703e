"""The C++ multi-GPU path of eds2leds (edsx_leds_merge_multi, csrc/merge_multi.hip) and its device range scans
(edsx_eds_scan_range / edsx_seds_scan_range, csrc/merge_scan.hip).  On the one-GPU box N ranks share the device and
exchange in process (RCCL does not run two ranks on one device); the RCCL exchange runs with one rank.
Expected: the Python scans (multigpu.eds_scan_range / seds_scan_range, the spec), the reference's fixtures, the oracle,
the Python MergeSharder's ranges, and the unpartitioned edsx_leds_merge."""
import json
import os
import random
import shutil
import subprocess
import sys

import pytest

import oracle_lib as o
from conftest import GOLDEN
from test_merge_gpu import _matches
from test_merge_shard_cpu import run_sharded, shaped_eds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edsparser_amd import multigpu as mg  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def multi():
    import edsparser_amd
    made = {}

    def get(n, rccl=False):
        if (n, rccl) not in made:
            made[(n, rccl)] = edsparser_amd.MultiGpu([0] * n, use_rccl=rccl)
        return made[(n, rccl)]
    yield get
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def ctx():
    import edsparser_amd
    c = edsparser_amd.Context(0)
    yield c
    c.close()


def _run(m, eds, seds, l, compact=True):
    import edsparser_amd
    try:
        out, so = m.leds_merge(eds, seds, l, compact)
        return {"out": out, "seds_out": so}
    except edsparser_amd.EdsxError as ex:
        return {"error": ex.message, "code": ex.code}


# ---- 1. the device range scans against the Python spec

def _check_scan(ctx, eds, lo, hi, l):
    end = mg._text_end(eds)
    want = mg.eds_scan_range(eds, lo, hi, l, end)
    got = ctx.eds_scan_range(eds, lo, hi, l)
    assert got == want, (eds[:200], len(eds), lo, hi, l)
    return want


def test_eds_scan_random_slices(ctx):
    rng = random.Random(11)
    cuts = checked = 0
    for it in range(40):
        l = rng.choice([1, 2, 5, 10, 32])
        linear = rng.random() < 0.5
        eds, _ = shaped_eds(rng, rng.randint(3, 150), l, rng.random() < 0.5, linear,
                            short_frac=rng.choice([0.0, 0.1, 0.4]), adj_frac=rng.choice([0.0, 0.1, 0.3]))
        end = mg._text_end(eds)
        braces = [i for i in range(end) if eds[i] in b"{},"]
        for _ in range(60):
            if rng.random() < 0.4 and braces:                  # slice edges on braces and commas, and next to them
                lo = min(end, max(0, rng.choice(braces) + rng.choice([-1, 0, 0, 1])))
                hi = min(end, max(0, rng.choice(braces) + rng.choice([-1, 0, 1, 1])))
            else:
                lo, hi = rng.randint(0, end), rng.randint(0, end)
            if lo > hi and rng.random() < 0.8:
                lo, hi = hi, lo
            cuts += _check_scan(ctx, eds, lo, hi, rng.choice([l, 0, 1, 3 * l]))["cut"] is not None
            checked += 1
        for lo, hi in [(0, end), (0, 0), (end, end), (end // 2, end // 2), (0, end // 3), (end // 3, end)]:
            _check_scan(ctx, eds, lo, hi, l)
            checked += 1
    assert checked >= 2000
    assert cuts > 200


def test_eds_scan_every_brace_kind_at_the_edges(ctx):
    rng = random.Random(12)
    for compact_in in (True, False):
        eds, _ = shaped_eds(rng, 40, 4, compact_in, False, short_frac=0.2, adj_frac=0.2)
        end = mg._text_end(eds)
        for kind in b"{},":
            for i in [j for j in range(end) if eds[j] == kind][:25]:
                for lo in (i, i + 1):
                    _check_scan(ctx, eds, lo, end, 4)
                    _check_scan(ctx, eds, lo, min(end, lo + 37), 4)
                    _check_scan(ctx, eds, max(0, lo - 29), lo, 4)


def test_eds_scan_text_that_is_not_plain(ctx):
    rng = random.Random(13)
    base, _ = shaped_eds(rng, 30, 3, True, False)
    base = base.rstrip(b"\n")
    texts = [b"{A,C} GGGG {T,G}\nAAAA{C,T}", base.replace(b"}", b"}\r\n", 3) + b"\r\n",
             base[:40] + b" " + base[40:], base[:30] + b"\t" + base[30:] + b"\n\n",
             b"ACGT,TT{A,C}GGGG{T,G}CCCC", b"{A,{C,G}}TTTT{A,C}GGGG{A,T}", b"{A,C}}GGGG{T,G}AAAA{{C,T}GG",
             b"{A,C}GGGG{T,G}AAAA{C,T", b"A,C}GGGG{T,G}AAAA{C,T}", b"", b"\n", b"ACGT", b"{A,C}"]
    for t in texts:
        end = mg._text_end(t)
        for lo in range(0, max(end, 1), max(1, end // 12)):
            for hi in sorted({lo, min(end, lo + 1), min(end, lo + 7), (lo + end) // 2, end}):
                _check_scan(ctx, t, lo, hi, 3)
                _check_scan(ctx, t, lo, hi, 0)


def test_eds_scan_long_slices_cross_many_blocks(ctx):
    rng = random.Random(14)
    eds, _ = shaped_eds(rng, 6000, 8, True, False, short_frac=0.3, adj_frac=0.2)
    end = mg._text_end(eds)
    for k in range(1, 8):
        _check_scan(ctx, eds, end * k // 8, end * (k + 1) // 8, 8)
        _check_scan(ctx, eds, end * k // 8, end * (k + 1) // 8, 10 ** 6)      # p never long enough: no cut
    _check_scan(ctx, eds, 0, end, 8)


def test_seds_scan_count_and_locate(ctx):
    import numpy as np
    rng = random.Random(15)
    for it in range(40):
        _, seds = shaped_eds(rng, rng.randint(3, 800), 4, True, True)
        n = len(seds)
        for _ in range(8):
            lo, hi = sorted((rng.randint(0, n), rng.randint(0, n)))
            want_ok, want_count = mg.seds_scan_range(seds, lo, hi)
            a = np.frombuffer(seds, dtype=np.uint8)[lo:hi]
            pos = np.flatnonzero(a == ord("{"))
            ords = sorted(rng.sample(range(len(pos)), min(len(pos), 5))) if want_ok and len(pos) else []
            ok, count, spans = ctx.seds_scan_range(seds, lo, hi, ords)
            assert (ok, count) == (want_ok, want_count), (it, lo, hi)
            assert count == (len(pos) if ok else 0)
            want_spans = [(int(pos[k]) + lo, seds.find(b"}", int(pos[k]) + lo) + 1) for k in ords]
            assert spans == want_spans, (it, lo, hi, ords)
    # whitespace inside the slice; a set whose '}' lies behind the slice; none at all
    assert ctx.seds_scan_range(b"{1}{2} {3}\n", 0, 10) == (False, 0, [])
    assert ctx.seds_scan_range(b"{1}{2}{3,4}\n", 0, 7, [2]) == (True, 3, [(6, 11)])
    assert ctx.seds_scan_range(b"{1}{2}{3,4", 0, 10, [2]) == (True, 3, [(6, 0)])


# ---- 2. the reference's fixtures

def test_reference_fixtures_gen_merge(multi):
    cases = json.load(open(os.path.join(GOLDEN, "gen_merge.json")))["cases"]
    for i, c in enumerate(cases):
        eds = c["eds"].encode()
        seds = c["seds"].encode() if c["seds"] is not None else None
        for n in (2, 3, 5):
            got = _run(multi(n), eds, seds, c["l"], c["compact"])
            got.pop("code", None)
            if "out" in got:
                got = {"out": got["out"].decode(), "seds_out": got["seds_out"].decode()}
            assert got == c["expect"], (i, n, c.get("name"))


def test_reference_fixtures_gen2_merge(multi):
    for c in json.load(open(os.path.join(GOLDEN, "gen2_merge.json")))["cases"]:
        out, so = multi(4).leds_merge(c["eds"].encode(), c["seds"].encode() if c["seds"] is not None else None, c["l"],
                                      c["compact"])
        assert _matches(c["expect"]["out"], out) and _matches(c["expect"]["seds_out"], so), c["name"]


# ---- 3. shaped inputs: the oracle's bytes, MergeSharder's ranges

@pytest.mark.parametrize("seed", range(4))
def test_shaped_inputs_equal_oracle_and_sharder(multi, seed):
    import edsparser_amd
    rng = random.Random(900 + seed)
    partitioned = 0
    for it in range(10):
        l = rng.choice([2, 5, 10, 32])
        linear = rng.random() < 0.6
        eds, seds = shaped_eds(rng, rng.randint(5, 300), l, rng.random() < 0.5, linear,
                               short_frac=rng.choice([0.0, 0.1, 0.4]), adj_frac=rng.choice([0.0, 0.1, 0.3]) if linear else 0.05,
                               collapse_frac=rng.choice([0.0, 0.0, 0.2]))
        compact = rng.random() < 0.5
        try:
            want = o.merge(eds, seds, l, compact)
        except o.OracleError as ex:
            for n in (2, 4):
                with pytest.raises(edsparser_amd.EdsxError) as ei:
                    multi(n).leds_merge(eds, seds, l, compact)
                assert ei.value.message == str(ex)
            continue
        for n in (2, 4, 8):
            got = multi(n).leds_merge(eds, seds, l, compact)
            info = multi(n).last_merge()
            _, _, sharder = run_sharded(eds, seds, l, compact, n)
            assert got == want, (seed, it, n, info)
            assert (info["partitioned"], info["ranges"]) == (sharder["partitioned"], sharder["ranges"]), (seed, it, n, info, sharder["why"])
            partitioned += info["partitioned"]
    assert partitioned > 8


# ---- 4. fallbacks: rank 0 merges the whole text, with edsx_leds_merge's bytes or error

def test_collapsing_neighbour_falls_back(multi):
    unit = "{A,C}GGGGGGGG"
    eds = (unit * 8 + "{C,G}" + "TTTTTTTT" + "{A,T}{G,C}{A,C}" + "GGGGGGGG{A,C}" * 5).encode()
    seds = ("{1}{2}{0}" * 8 + "{1}{2}" + "{0}" + "{1}{2}{1}{3}{1}{2}" + "{0}{1}{2}" * 5).encode()
    want = o.merge(eds, seds, 4, True)
    assert multi(2).leds_merge(eds, seds, 4, True) == want
    info = multi(2).last_merge()
    assert not info["partitioned"] and info["fallback"] == 5 and info["ranges"] == 1
    # CARTESIAN products never collapse: the same text is partitioned
    assert multi(2).leds_merge(eds, None, 4, True) == o.merge(eds, None, 4, True)
    assert multi(2).last_merge()["partitioned"]


def test_fallbacks_equal_the_single_call(multi, ctx):
    import edsparser_amd
    rng = random.Random(16)
    eds, seds = shaped_eds(rng, 200, 4, True, True)
    body = eds.rstrip(b"\n")
    sbody = seds.rstrip(b"\n")
    k = len(body) // 2
    cases = [
        (body[:k] + b" " + body[k:] + b"\n", seds, 4, 2),                 # whitespace inside: not plain
        (body[:k] + b"\r\n" + body[k:] + b"\r\n", seds, 4, 2),
        (body.replace(b"}", b"},", 1), None, 4, 2),                       # a comma outside braces
        (b"{A,{C,G}}" + body, None, 4, 2),                                 # nested braces
        (body + b"{A,C", None, 4, 2),                                      # unbalanced
        (eds, sbody + b"{1}\n", 4, 4),                                     # one source set too many
        (eds, sbody[:sbody.rfind(b"{")] + b"\n", 4, 4),                    # one too few
        (eds, sbody.replace(b"{1", b"{x", 1) + b"\n", 4, None),            # a bad source id
        (eds, seds, 0, 1),                                                 # l = 0
        (eds, None, 0, 1),
        (b"{A,C}{G,T}", b"{1}{2}{1}{2}", 3, 3),                            # no sentinel
        (b"", None, 3, 3),
    ]
    for i, (e, s, l, why) in enumerate(cases):
        try:
            want = {"out": ctx.leds_merge(e, s, l, True)}
        except edsparser_amd.EdsxError as ex:
            want = {"error": ex.message, "code": ex.code}
        for n in (2, 3):
            try:
                got = {"out": multi(n).leds_merge(e, s, l, True)}
            except edsparser_amd.EdsxError as ex:
                got = {"error": ex.message, "code": ex.code}
            assert got == want, (i, n)
            if why is not None and "out" in got:
                info = multi(n).last_merge()
                assert not info["partitioned"] and info["fallback"] == why, (i, n, info)


# ---- 5. BASELINE configs[2] shape at 1/10

def test_configs2_shape_tenth(multi, ctx):
    from merge_cases import genrandomeds_shaped
    eds, seds = genrandomeds_shaped(10, 0.10, 3)
    whole = ctx.leds_merge(eds, seds, 32, True)
    for n in (4, 8):
        assert multi(n).leds_merge(eds, seds, 32, True) == whole, n
        info = multi(n).last_merge()
        assert info["partitioned"] and info["ranges"] == n and info["fallback"] == 0, info
        if n == 8:
            assert info["eds_h2d_bytes_max"] <= len(eds) // 3, info
            assert info["seds_h2d_bytes_max"] <= len(seds) // 3, info
            assert info["range_bytes_max"] < len(eds) // 4, info


# ---- 6. RCCL with one rank

def test_rccl_one_rank_equals_single_call(multi, ctx):
    rng = random.Random(17)
    for compact in (True, False):
        for linear in (True, False):
            eds, seds = shaped_eds(rng, 150, 5, compact, linear)
            want = ctx.leds_merge(eds, seds, 5, compact)
            assert multi(1, rccl=True).leds_merge(eds, seds, 5, compact) == want, (compact, linear)
            info = multi(1, rccl=True).last_merge()
            assert not info["partitioned"] and info["fallback"] == 1


# ---- 7. eds2leds --gpus

def _eds2leds():
    from test_host_cpp import BUILD, _build_host
    _build_host()
    return os.path.join(BUILD, "eds2leds")


def _cli(tmp_path, sub, src_eds, src_seds, args):
    d = tmp_path / sub
    d.mkdir()
    shutil.copy(src_eds, d / "in.eds")
    cmd = [_eds2leds(), "-i", str(d / "in.eds")] + args
    if src_seds:
        shutil.copy(src_seds, d / "in.seds")
        cmd += ["-s", str(d / "in.seds")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    return r, d


def test_eds2leds_gpus_writes_the_same_files(tmp_path):
    g = os.path.join(GOLDEN, "ref_data")
    for name, e, s, args in [("linear", os.path.join(g, "vcf", "small.eds"), os.path.join(g, "vcf", "small.seds"), ["-l", "4"]),
                             ("cartesian", os.path.join(g, "eds", "test_iterative.eds"), None, ["-l", "4", "--full"])]:
        r1, d1 = _cli(tmp_path, name + "_one", e, s, args)
        r2, d2 = _cli(tmp_path, name + "_gpus", e, s, args + ["--gpus", "1"])
        assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr, r2.stderr)
        files = sorted(p.name for p in d1.iterdir())
        assert files == sorted(p.name for p in d2.iterdir())
        assert "in_l4.leds" in files and (s is None or "in_l4.seds" in files)
        for f in files:
            assert (d1 / f).read_bytes() == (d2 / f).read_bytes(), (name, f)
        assert "  GPUs: 1 (not partitioned: one GPU merges the file)" in r2.stdout
        lines = r2.stdout.splitlines()           # (RCCL may print lines of its own in between)
        threads = [i for i, x in enumerate(lines) if x.startswith("  Threads:")]
        assert threads and threads[0] < lines.index("  GPUs: 1 (not partitioned: one GPU merges the file)")
        assert "GPUs" not in r1.stdout


def test_eds2leds_gpus_malformed_input(tmp_path):
    bad = tmp_path / "bad.eds"
    bad.write_bytes(b"{A,C}GGGG{T,G")
    r1, _ = _cli(tmp_path, "one", bad, None, ["-l", "3"])
    r2, _ = _cli(tmp_path, "gpus", bad, None, ["-l", "3", "--gpus", "1"])
    assert r1.returncode == 1 and r2.returncode == 1
    err1 = [x for x in r1.stderr.splitlines() if x.startswith("Error:")]
    err2 = [x for x in r2.stderr.splitlines() if x.startswith("Error:")]
    assert err1 and err1 == err2
