"""CPU: the query side of the edsparser::EDS container (check_position / extract / generate_patterns) against the
fixture cases (tests/golden/query_cases.json) and the Python restatement (tests/query_oracle.py), and the
edsparser-genpatterns argument errors that end before any device work."""
import json
import os
import random
import shutil
import subprocess

import pytest

import query_oracle as qo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "edsparser_amd", "host")
BUILD = os.path.join(HOST, "build")
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "edsparser_amd")
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "query_cases.json")))


def _build_host():
    import edsparser_amd.build as b
    b.build()
    subprocess.run(["make", "-s", "-C", HOST], check=True)


@pytest.fixture(scope="module")
def runner(tmp_path_factory):
    _build_host()
    exe = os.path.join(BUILD, "test_query")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", INC, os.path.join(ROOT, "tests", "cpp", "test_query.cpp"),
                    os.path.join(BUILD, "libedsparser_lib.a"), "-L", LIBDIR, "-ledsx", "-Wl,-rpath," + LIBDIR,
                    "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    d = tmp_path_factory.mktemp("query")

    def run(cmds, want_stderr=False):
        f = d / "cmds.txt"
        f.write_text("".join("\t".join(str(x) for x in c) + "\n" for c in cmds))
        r = subprocess.run([exe, str(f)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = r.stdout.split("\n")[:-1]
        assert len(out) == len(cmds)
        return (out, r.stderr) if want_stderr else out
    return run


def _check_cmd(eds, seds, pos, choices, pattern):
    return ("C", eds, "-" if seds is None else seds, pos, ",".join(str(c) for c in choices), pattern)


def _norm(r):
    if r in ("true", "false"):
        return r == "true"
    return r.split(":", 1)[0]


def test_check_position_fixture_cases(runner):
    cs = CASES["check"]
    out = runner([_check_cmd(c["eds"], c["seds"], c["pos"], c["choices"], c["pattern"]) for c in cs])
    for c, r in zip(cs, out):
        assert _norm(r) == c["expected"], (c["src"], r)
        assert qo.check(qo.Eds(c["eds"], c["seds"]), c["pos"], c["choices"], c["pattern"]) == c["expected"], c["src"]


def test_check_position_warns_about_extra_choices(runner):
    out, err = runner([_check_cmd("{ACGT}{A,ACA}{CGT}{T,TG}", None, 0, [0, 2, 3], "ACGTACGTT")], want_stderr=True)
    assert out == ["true"]
    assert "Warning: More degenerate strings provided (3) than needed (2). Extra strings will be ignored." in err


def test_extract_fixture_cases(runner):
    cs = CASES["extract"]
    out = runner([("X", c["eds"], c["pos"], c["len"], ",".join(str(x) for x in c["changes"])) for c in cs])
    for c, r in zip(cs, out):
        if "expected" in c:
            assert r == "=" + c["expected"], (c["src"], r)
        else:
            assert r.startswith(c["error"] + ":"), (c["src"], r)
            assert c.get("message", "") in r, (c["src"], r)


def test_generate_patterns_fixture_cases(runner):
    cs = CASES["generate"]
    out = runner([("G", c["eds"], c["count"], c["length"], 1234 + k) for k, c in enumerate(cs)])
    for c, r in zip(cs, out):
        if "error" in c:
            assert r.startswith(c["error"] + ":") and c["message"] in r, (c["src"], r)
            continue
        lines = r[1:].split("|")[:-1] if r != "=" else []
        assert len(lines) == c["count"] and all(len(x) == c["length"] for x in lines), (c["src"], r)
        assert len(set(lines)) >= c["min_distinct"], (c["src"], r)


def test_metadata_tables(runner):
    out = runner([("M", "{ACGT}{A,ACA}{CGT}{T,TG}"), ("M", ""), ("M", "{A,C}{}{GG}{T,,A}")])
    assert out == ["0,4,4,7,7;0,0,2,2,4", ";", "0,0,0,2,2;0,2,2,2,5"]


def _random_eds(rng):
    n = rng.randint(1, 7)
    sets = []
    for _ in range(n):
        k = rng.choice([1, 1, 2, 2, 3])
        sets.append([("".join(rng.choice("AC") for _ in range(rng.choice([0, 1, 1, 2, 3])))) for _ in range(k)])
    eds = "".join("{" + ",".join(s) + "}" for s in sets)
    seds = None
    if rng.random() < 0.5:
        m = sum(len(s) for s in sets)
        groups = []
        for _ in range(m):
            r = rng.random()
            ids = {0} if r < 0.2 else set(rng.sample(range(1, 5), rng.randint(1, 3)))
            if r > 0.9:
                ids.add(0)
            groups.append("{" + ",".join(str(x) for x in sorted(ids)) + "}")
        seds = "".join(groups)
    return eds, seds


def _random_query(rng, e):
    """A walk of a random path (valid choices), then mutated: a changed character, a wrong symbol, an out-of-range or
    negative number, a missing or extra choice, the empty pattern, a position past the end."""
    pos = rng.randrange(e.C + 2) if e.C else rng.randrange(2)
    choices, text = [], ""
    if pos < e.C:
        s, off = qo._start(e, pos)
        L = rng.randint(1, 8)
        for sym in range(s, e.n):
            if len(text) >= L:
                break
            if e.deg[sym]:
                j = rng.randrange(len(e.sets[sym]))
                choices.append(e.cum_deg[sym] + j)
                text += e.sets[sym][j]
            else:
                text += e.sets[sym][0][off if sym == s else 0:]
        text = text[:L]
    pattern = text
    r = rng.random()
    if r < 0.15 and pattern:
        i = rng.randrange(len(pattern))
        pattern = pattern[:i] + rng.choice("ACG") + pattern[i + 1:]
    elif r < 0.25 and choices:
        choices[rng.randrange(len(choices))] = rng.randrange(e.cum_deg[-1] + 1) if e.cum_deg[-1] else 0
    elif r < 0.3 and choices:
        choices[rng.randrange(len(choices))] = e.cum_deg[-1] + rng.randrange(3)
    elif r < 0.35 and choices:
        choices[rng.randrange(len(choices))] = -rng.randint(1, 3)
    elif r < 0.45 and choices:
        choices.pop(rng.randrange(len(choices)))
    elif r < 0.5:
        choices.append(rng.randrange(-1, e.cum_deg[-1] + 2))
    elif r < 0.55:
        pattern = ""
    elif r < 0.65:
        pattern += rng.choice("AC")
    return pos, choices, pattern


def test_check_position_against_restatement(runner):
    rng = random.Random(7)
    cmds, want = [], []
    for _ in range(400):
        eds, seds = _random_eds(rng)
        e = qo.Eds(eds, seds)
        for _ in range(10):
            pos, choices, pattern = _random_query(rng, e)
            cmds.append(_check_cmd(eds, seds, pos, choices, pattern))
            want.append(qo.check(e, pos, choices, pattern))
    out = runner(cmds)
    kinds = set()
    for c, r, w in zip(cmds, out, want):
        assert _norm(r) == w, (c, r, w)
        kinds.add(w if isinstance(w, str) else str(w))
    assert kinds == {"True", "False", "out_of_range", "invalid_argument"}


def test_seeded_sampler_against_restatement(runner):
    rng = random.Random(11)
    edss = ["ACGT{A,C}GG", "{A,C}{G,T}", "{,A}{,}{TTT}{G,GG,GGG}", "{ACGT}{A,ACA}{CGT}{T,TG}", "{A}{,}"]
    for _ in range(60):
        edss.append(_random_eds(rng)[0])
    cmds, want = [], []
    for eds in edss:
        for seed in (0, 1, 2**63 + 5):
            L = rng.randint(1, 12)
            cmds.append(("G", eds, 7, L, seed))
            try:
                want.append("=" + qo.generate(qo.Eds(eds), 7, L, seed)[0].decode().replace("\n", "|"))
            except RuntimeError as x:
                want.append("runtime_error: " + str(x))
    out = runner(cmds)
    for c, r, w in zip(cmds, out, want):
        assert r == w, (c, r, w)
    # every non-wrapped witness of the restatement is a true check_position of the container
    checks = []
    for eds in edss[:20]:
        e = qo.Eds(eds)
        try:
            text, wit = qo.generate(e, 20, 6, 99)
        except RuntimeError:
            continue
        for pat, (p, ch) in zip(text.decode().split("\n"), wit):
            if p is not None:
                checks.append(_check_cmd(eds, None, p, ch, pat))
    assert len(checks) > 50
    assert runner(checks) == ["true"] * len(checks)


def test_genpatterns_cli_argument_errors(tmp_path):
    _build_host()
    exe = os.path.join(BUILD, "edsparser-genpatterns")
    eds = tmp_path / "x.eds"
    eds.write_text("{ACGT}{A,C}")
    cases = [
        ([], "the option '--input' is required but missing"),
        (["-i", str(eds)], "the option '--output' is required but missing"),
        (["-i", str(tmp_path / "missing.eds"), "-o", str(tmp_path / "p.txt")], "Error: Input file does not exist:"),
        (["-i", str(eds), "-o", str(tmp_path / "p.txt"), "-n", "0"], "Error: Pattern count must be greater than 0"),
        (["-i", str(eds), "-o", str(tmp_path / "p.txt"), "-l", "0"], "Error: Pattern length must be greater than 0"),
        (["-i", str(eds), "-o", str(tmp_path / "p.txt"), "--seed", "x"], "for option '--seed' is invalid"),
        (["-i", str(eds), "-o", str(tmp_path / "p.txt"), "--bogus"], "unrecognised option '--bogus'"),
    ]
    for args, msg in cases:
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)
        assert "[Performance] Runtime:" in r.stderr
    assert not (tmp_path / "p.txt").exists()
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--count" in r.stdout and "--length" in r.stdout and "--witness" in r.stdout


def test_reference_style_caller_against_installed_package(tmp_path):
    """A caller written against the reference's API compiles and links against the installed CMake package, which
    also installs edsparser-genpatterns."""
    if not shutil.which("cmake"):
        pytest.skip("cmake not installed")
    _build_host()
    b, prefix = tmp_path / "b", tmp_path / "prefix"
    for cmd in (["cmake", "-S", HOST, "-B", str(b), "-DCMAKE_INSTALL_PREFIX=" + str(prefix)],
                ["cmake", "--build", str(b), "-j4"], ["cmake", "--install", str(b)]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    assert (prefix / "bin" / "edsparser-genpatterns").exists()
    user = tmp_path / "user"
    user.mkdir()
    (user / "CMakeLists.txt").write_text(
        "cmake_minimum_required(VERSION 3.16)\nproject(user CXX)\nfind_package(EDSParser REQUIRED)\n"
        "add_executable(user main.cpp)\ntarget_link_libraries(user EDSParser::EDSParser)\n")
    (user / "main.cpp").write_text(
        '#include "edsparser/formats/eds.hpp"\n#include <sstream>\n#include <stdexcept>\nusing namespace edsparser;\n'
        'int main() {\n  EDS eds("{ACGT}{A,ACA}{CGT}{T,TG}");\n'
        '  bool thrown = false;  // position 4 starts at {CGT}: string 0 belongs to symbol 1 (eds.cpp:1171)\n'
        '  try { eds.check_position(4, {0, 2}, "ACGTT"); } catch (const std::invalid_argument&) { thrown = true; }\n'
        '  bool b = eds.check_position(0, {0, 2}, "ACGTACGTT");\n'
        '  std::ostringstream os;\n  eds.generate_patterns(os, 3, 4);\n  eds.generate_patterns(os, 3, 4, 7);\n'
        '  const auto& md = eds.get_metadata();\n'
        '  return (thrown && b && eds.extract(1, 2, {1, 0}) == "ACACGT" && md.cum_common_positions.size() == 5 &&\n'
        '          md.cum_degenerate_counts.back() == 4 && os.str().size() == 30) ? 0 : 1;\n}\n')
    for cmd in (["cmake", "-S", str(user), "-B", str(user / "b"), "-DCMAKE_PREFIX_PATH=" + str(prefix)],
                ["cmake", "--build", str(user / "b")]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    env = dict(os.environ, LD_LIBRARY_PATH=str(prefix / "lib") + ":/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([str(user / "b" / "user")], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
