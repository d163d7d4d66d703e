"""CPU: the per-thread device code of contig selection and the host arithmetic of VcfSession (csrc/vcf_contig_walk.hpp) as
host code under the address and undefined-behaviour sanitizers (tests/cpp/test_contig_walk.cpp, a stand-alone program), on
buffers of exactly the sizes the session allocates, filled with NUL, line feeds, 0xFF, '>' or tabs.  Every load and store of
that source is checked there, the masked ones the guard build cannot see included.  What the program finds must equal
tests/contig_spec.py and the oracle under every fill: every field of every FASTA record, the key of every record line,
the regrouped line starts and first[], the counts, the verdict "the host classifies this file", the host classification,
and the texts of the picked contigs, transformed from the record where it lies inside the whole FASTA buffer.

Measured: the whole file takes 37 s on the development machine, 21 s of it the build of the program; the two K = 65 536
families run under two fills (they are half of the program's time under five)."""
import time

import numpy as np
import pytest

import contig_walk_cases as w
import contig_walk_expect as x


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("contig_walk")
    return w.build_test_contig_walk(w.ROOT, str(d / "test_contig_walk")), str(d)


@pytest.fixture(scope="module")
def families():
    return w.families()


def _check_run(case, r):
    """one (case, fill) result of the program against the specification; returns the number of contigs compared in full"""
    tag = (case["name"], "fill 0x%02x" % r["fill"])
    assert r["status"] == w.OK, tag + (r["status"], r.get("detail"))
    e = x.expected(case)
    K = e["K"]
    assert r["K"] == K, tag
    got = r["recs"]
    for col, field in enumerate(w.REC_FIELDS[:7]):
        bad = np.nonzero(got[:, col] != e["recs"][:, col])[0]
        assert bad.size == 0, tag + (field, int(bad[0]), int(got[bad[0], col]), int(e["recs"][bad[0], col]))
    assert np.array_equal(got[:, 8], e["duplicate"]), tag
    assert r["passes"] == e["passes"], tag
    assert r["oob"] == 0, tag
    assert bool(r["on_device"]) == (not e["host"] and len(case["V"]) > 0), tag + ("verdict",)
    # host classification: always
    assert (r["host_total"], r["host_without_token"], r["host_unknown"]) == (e["nr"], e["without_token"], e["unknown"]), tag
    assert np.array_equal(r["host_counts"], e["counts"]), tag
    assert r["host_unknown_text"] == e["unknown_text"], tag
    assert np.array_equal(got[:, 7], e["counts"]), tag                       # vcf_records, from whichever side classified
    if r["on_device"]:
        assert r["nr"] == e["nr"], tag
        assert np.array_equal(r["keys"], e["keys"]), tag
        assert np.array_equal(r["lsorted"], e["lsorted"]), tag
        assert np.array_equal(r["first"], e["first"]), tag
        assert np.array_equal(r["counts"], e["counts"]) and r["unknown"] == e["unknown"], tag
    # the picked contigs
    assert [c["index"] for c in r["contigs"]] == w.pick_indices(case, x.records_of(case)), tag
    full = 0
    for nm, c in zip(case["pick"], r["contigs"]):
        want = x.expected_texts(case, nm)
        if "error" in want:
            assert c["verdict"] == w.REFUSED, tag + (nm, want["error"])
        else:
            assert c["verdict"] == w.OK, tag + (nm, c["verdict"])
            assert (c["eds"], c["seds"]) == (want["eds"], want["seds"]), tag + (nm,)
            full += 1
        lines = c["text"].split(b"\n")
        assert (lines[:-1] if lines[-1] == b"" else lines) == x.contig_lines(case, nm), tag + (nm, "host text")
    return full


def _run(program, cases, tag):
    exe, workdir = program
    t0 = time.time()
    res = w.run_program(exe, workdir, cases, x.records_of, tag)
    t1 = time.time()
    runs = full = picks = 0
    for c in cases:
        assert [r["fill"] for r in res[c["name"]]] == list(c.get("fills", w.FILLS)), c["name"]
        for r in res[c["name"]]:
            full += _check_run(c, r)
            picks += len(c["pick"])
            runs += 1
    print("%s: %d cases, %d runs, %d of %d contigs compared in full, program %.1f s, comparison %.1f s"
          % (tag, len(cases), runs, full, picks, t1 - t0, time.time() - t1))
    assert full * 10 >= picks * 9, (full, picks)                # (the oracle refuses one record of the long walks: it has no sequence)
    return res


def test_fasta_index_shift_sweep(program, families):
    """a first record of p bytes in front of ten records with a bit of everything: every '>', header newline, name end and
    record end 1 before, at and 1 after every multiple of 16 and of 1024 (asserted by the case module)"""
    assert len(families["shift"]) >= 60
    _run(program, families["shift"], "shift")


def test_fasta_index_ends_and_edges(program, families):
    cases = families["ends"]
    assert len(cases) == len(w.END_TARGETS) * 5 + 4
    _run(program, cases, "ends")


def test_fasta_index_long_walks(program, families):
    """every exit of fi_next_newline through the index, and the two block walks against byte-by-byte walks over a grid of
    arguments the index never makes (a limit in front of the block's newlines)"""
    cases = families["walks"]
    assert all(c.get("sweep") for c in cases) and len(cases) == 16 + 6
    _run(program, cases, "walks")


def test_fasta_index_two_scan_tiles(program, families):
    (case,) = families["tile"]
    assert len(case["F"]) == 2 * 1024 * 1024 + 17
    _run(program, [case], "tile")


def test_classification_names(program, families):
    res = _run(program, families["names"], "names")
    on_device = sum(r["on_device"] for runs in res.values() for r in runs)
    assert on_device == sum(len(runs) for runs in res.values())            # all of them are plain


def test_classification_host_bound(program, families):
    cases = families["hostbound"]
    assert len(cases) == 7 and all(x.host_bound(c["V"]) for c in cases)
    res = _run(program, cases, "hostbound")
    assert not any(r["on_device"] for runs in res.values() for r in runs)
    assert any(r["host_without_token"] for r in res["hostbound/whitespace_only"])


def test_record_count_switches(program, families):
    cases = families["counts"]
    assert [x.expected(c)["K"] for c in cases] == [255, 256, 65535, 65536, 256, 256, 256]
    assert [x.expected(c)["nr"] for c in cases] == [3000] * 4 + [2047, 2048, 2049]
    assert [x.expected(c)["passes"] for c in cases] == [1, 2, 2, 3, 2, 2, 2]
    for c in cases:
        assert x.expected(c)["unknown"] == 20                                # the key K itself is in play
    _run(program, cases, "counts")


def test_weak_hash_instantiation(program):
    """a 4-bit hash: the names family and K = 256 with up to 16 and more names per hash value, so the loop "the hash finds,
    the bytes decide" runs over collisions; the results are those of the full hash"""
    cases = w.weak_hash_cases()
    assert len(cases) == 25 + 1
    _run(program, cases, "weak")
