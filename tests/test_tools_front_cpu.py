"""CPU: the front end the command-line tools share (edsparser_amd/host/tools/tool_front.hpp).  Its pure pieces - path lists,
the -i / -s / -o defaults, the --names table - run under ASan and UBSan in a program of their own, and the part of every
path tool's command line that needs no device is pinned to the byte: exit status, stderr and --help, as recorded from the
tools before they were moved onto the shared front end (tests/golden/tool_help/)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "edsparser_amd", "host")
BUILD = os.path.join(HOST, "build")
HELP = os.path.join(ROOT, "tests", "golden", "tool_help")


def _invalid(text, option):
    return "error: the argument ('%s') for option '--%s' is invalid" % (text, option)


def test_front_end_pieces(tmp_path):
    exe = str(tmp_path / "test_tool_front")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-I", os.path.join(HOST, "tools"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_tool_front.cpp"), "-o", exe], check=True)
    # four lines for the five paths of the cases below: CRLF line ends, an empty line, a name with a blank, no last line end
    names = str(tmp_path / "names.txt")
    open(names, "wb").write(b"alpha\r\n\r\nbe ta\r\ndelta")
    P = 5
    no_name = "error: The names file has no name for path %d"
    no_cell = "error: The name of path %d is empty or holds a tab, blank or line feed"
    out_of_range = "error: Path id %d out of range (1..5)"
    N = ["--names", names]
    cases = [
        # the list grammar, under the name of the option that carries it
        (["p", "paths", "1,5,7-9"], "1 5 7 8 9"), (["p", "targets", "9-7"], _invalid("9-7", "targets")), (["p", "paths", "1,,2"], _invalid("1,,2", "paths")),
        (["p", "donors", "1,x"], _invalid("1,x", "donors")), (["p", "paths", "-3"], _invalid("-3", "paths")), (["p", "paths", ""], _invalid("", "paths")),
        (["p", "paths", "1-4294967298"], _invalid("1-4294967298", "paths")), (["p", "paths", "7-7,0,18446744073709551615"], "7 0 18446744073709551615"),
        (["p", "paths", "18446744073709551616"], _invalid("18446744073709551616", "paths")), (["p", "paths", "3, 4"], _invalid("3, 4", "paths")),
        # no list: 1..P; a list: every id within 1..P, the first one that is not is named
        (["r", P, "-"], "1 2 3 4 5"), (["r", 0, "-"], ""), (["r", P, "5"], "5"), (["r", P, "0"], out_of_range % 0), (["r", P, "6"], out_of_range % 6),
        (["r", P, "2,6,0"], out_of_range % 6), (["r", P, "5,1,5"], "5 1 5"),
        # -s: the input with the .seds extension; -o: <input stem><suffix> next to the input, for a tool that has a default
        (["f", ".fa", "-i", "noext"], "noext|noext.seds|noext.fa|0"), (["f", ".fa", "-i", "a.b.eds"], "a.b.eds|a.b.seds|a.b.fa|0"),
        (["f", ".msa", "-i", "x.eds"], "x.eds|x.seds|x.msa|0"), (["f", ".ld", "-i", "./x.eds"], "./x.eds|./x.seds|./x.ld|0"),
        (["f", "_subset.eds", "-i", "/d.1/x.leds"], "/d.1/x.leds|/d.1/x.seds|/d.1/x_subset.eds|0"),
        (["f", ".gfa", "-i", "d/x.eds", "-s", "y.seds"], "d/x.eds|y.seds|d/x.gfa|1"), (["f", ".gfa", "-i", "d/x.eds", "-o", "o.txt"], "d/x.eds|d/x.seds|o.txt|0"),
        (["f", "-", "-i", "d/x.eds"], "d/x.eds|d/x.seds||0"), (["f", "-", "-i", "x.eds", "-o", "o.tsv"], "x.eds|x.seds|o.tsv|0"),
        (["f", ".fa", "-i", "x.eds", "-s", ""], "x.eds|x.seds|x.fa|0"),
        # a name as a FASTA header, a GFA path or a sample (eds2fasta, eds2msa, eds2gfa, subset): the line has to be there and not empty
        (["n", 0, 1] + N, "alpha"), (["n", 0, 2] + N, no_name % 2), (["n", 0, 3] + N, "be ta"), (["n", 0, 4] + N, "delta"), (["n", 0, 0] + N, no_name % 0),
        (["n", 0, P] + N, no_name % P), (["n", 0, P + 1] + N, no_name % (P + 1)), (["n", 0, 1], "s0"), (["n", 0, P, "--prefix", "row"], "row4"),
        (["n", 0, 1, "--names", str(tmp_path / "none.txt")], "error: Cannot open names file: " + str(tmp_path / "none.txt")),
        # a name as a cell of a table (dist, ibs, mosaic): nothing empty, no tab, blank or line feed, from the file or from --prefix
        (["n", 1, 1] + N, "alpha"), (["n", 1, 2] + N, no_cell % 2), (["n", 1, 3] + N, no_cell % 3), (["n", 1, 4] + N, "delta"), (["n", 1, 0] + N, no_name % 0),
        (["n", 1, P] + N, no_name % P), (["n", 1, P + 1] + N, no_name % (P + 1)), (["n", 1, 1], "s0"), (["n", 1, P, "--prefix", ""], "4"),
        (["n", 1, 2, "--prefix", "a b"], no_cell % 2),
        # the view the C ABI takes
        (["v", "4,1,3"] + N, "delta|alpha|be ta"), (["v", "1,2"] + N, no_name % 2), (["v", "2-3"], "s1|s2"),
    ]
    (tmp_path / "cases.txt").write_bytes(b"".join("\t".join(str(x) for x in c).encode() + b"\n" for c, _ in cases))
    r = subprocess.run([exe, str(tmp_path / "cases.txt")], capture_output=True, text=True,
                       env={k: v for k, v in os.environ.items() if k != "LD_PRELOAD"})
    assert r.returncode == 0, r.stderr[-3000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(cases)
    for (c, want), g in zip(cases, got):
        assert g == want, c


# ---- the command lines that end before any device work: (arguments, stderr in front of the "[Performance]" line) --------------
X = ["-i", "{d}/x.eds"]
REGION = ["-r", "1:0-5", "--table"]
REQUIRED = ([], "Error: the option '--input' is required but missing\n")
UNKNOWN = (["--nope"], "Error: unrecognised option '--nope'\n")
NO_INPUT = (["-i", "{d}/none.eds"], "Error: Input file does not exist: {d}/none.eds\n")
NO_SOURCES = (["-i", "{d}/y.eds"], "Error: Path spelling needs sources (.seds): {d}/y.seds does not exist\n")
NO_GIVEN_SOURCES = (X + ["-s", "{d}/none.seds"], "Error: Sources file does not exist: {d}/none.seds\n")


def _bad(option, value, flag=None):
    return (X + [flag or "--" + option, value], "Error: the argument ('%s') for option '--%s' is invalid\n" % (value, option))


CLI = {
    "eds2fasta": [REQUIRED, UNKNOWN, NO_INPUT, NO_SOURCES, _bad("paths", "1,x", "-p"), (X + ["--batch-mb", "0"], "Error: --batch-mb must be > 0\n"),
                  _bad("line-width", "x"), _bad("batch-mb", "-1")],
    "eds2msa": [REQUIRED, UNKNOWN, NO_INPUT, NO_SOURCES, _bad("paths", "1,x", "-p"), (X + ["--batch-mb", "0"], "Error: --batch-mb must be > 0\n"),
                (X + ["--gap", "ab"], "Error: --gap takes one character\n"), (X + ["--gap", ","], "Error: Gap character is not usable in an alignment\n"),
                _bad("max-mb", "x"), _bad("line-width", "-2")],
    "eds2gfa": [REQUIRED, UNKNOWN, NO_INPUT, NO_GIVEN_SOURCES,
                (["-i", "{d}/y.eds", "-p", "1"], "Error: --paths and --names need sources (.seds): {d}/y.seds does not exist\n"),
                (X + ["--no-paths", "-p", "1"], "Error: --no-paths does not go with --sources, --paths or --names\n"), _bad("paths", "1,x", "-p"),
                (X + ["--batch-mb", "0"], "Error: --batch-mb must be > 0\n"), _bad("max-links", "x")],
    # (--ref-path, --line-width and --max-bytes are read after the context is created: they need a device)
    "eds2vcf": [REQUIRED, UNKNOWN, NO_INPUT, NO_GIVEN_SOURCES,
                (["-i", "{d}/y.eds", "--names", "{d}/names.txt"], "Error: --names needs sources (.seds): {d}/y.seds does not exist\n"),
                (X + ["--no-samples", "--ref-path", "1"], "Error: --no-samples does not go with --sources, --names or --ref-path\n"),
                (X + ["--names", "{d}/none.txt"], "Error: Cannot open names file: {d}/none.txt\n")],
    "edsparser-subset": [REQUIRED, UNKNOWN, NO_INPUT, (["-i", "{d}/y.eds"], "Error: Path subsetting needs sources (.seds): {d}/y.seds does not exist\n"),
                         _bad("paths", "1,x", "-p"), (X, "Error: One of --paths and --paths-file is required\n"),
                         (X + ["-p", "1", "--paths-file", "{d}/ids.txt"], "Error: --paths and --paths-file exclude each other\n"),
                         (X + ["--paths-file", "{d}/badids.txt"], "Error: Paths file line 3 is not a path id\n"),
                         (X + ["--paths-file", "{d}/none.txt"], "Error: Cannot open paths file: {d}/none.txt\n"),
                         (X + ["-p", "1", "--names", "{d}/names.txt"], "Error: --names and --names-out go together\n")],
    "edsparser-lift": [REQUIRED, UNKNOWN, (["-i", "{d}/none.eds"], "Error: Input file does not exist: \"{d}/none.eds\"\n"), NO_SOURCES, _bad("to", "x"),
                       (X + ["--bed"], "Error: --bed needs --to\n"),
                       (X + ["--sites", "--bed", "--to", "1"], "Error: --sites, --from-eds and --bed exclude each other\n"),
                       (X + ["-q", "{d}/none.tsv"], "Error: Query file does not exist: \"{d}/none.tsv\"\n"),
                       (X + ["-q", "{d}/badq.tsv"], "Error: Query file line 3 is malformed: \"1\tx\t2\"\n")],
    "edsparser-slice": [REQUIRED, UNKNOWN, (["-i", "{d}/none.eds"] + REGION, "Error: Input file does not exist: \"{d}/none.eds\"\n"),
                        (["-i", "{d}/y.eds"] + REGION, NO_SOURCES[1]), (X, "Error: No region given (-r, --columns or --bed)\n"), _bad("region", "1:5", "-r"),
                        _bad("columns", "a-b"), (X + REGION + ["--max-bytes", "x"], "Error: the argument ('x') for option '--max-bytes' is invalid\n"),
                        (X + ["-r", "1:0-5"], "Error: Nothing to do: give --output, --output-dir or --table\n"),
                        (X + ["--bed", "{d}/none.bed"], "Error: Cannot open BED file: \"{d}/none.bed\"\n"),
                        (X + ["--bed", "{d}/bad.bed"], "Error: BED file line 2 is malformed: \"1\t5\"\n")],
    "edsparser-dist": [REQUIRED, UNKNOWN, NO_INPUT, NO_SOURCES, _bad("paths", "1,x", "-p"), _bad("metric", "rows"), _bad("format", "csv"), _bad("max-mb", "x")],
    "edsparser-ld": [REQUIRED, UNKNOWN, NO_INPUT, NO_SOURCES, _bad("paths", "1,x", "-p"), _bad("window", "0"), _bad("min-r2", "2"), _bad("min-r2", "0.5x"),
                     _bad("min-count", "x"), _bad("max-pairs", "-1")],
    "edsparser-ibs": [REQUIRED, UNKNOWN, NO_INPUT, NO_SOURCES, _bad("paths", "1,x", "-p"), _bad("min-sites", "x"), _bad("min-columns", "1.5"),
                      _bad("max-segments", "x")],
    "edsparser-mosaic": [REQUIRED, UNKNOWN, NO_INPUT, NO_SOURCES, _bad("targets", "1,x", "-t"), _bad("donors", "1,x", "-d"),
                         (X + ["-t", "1", "-d", "9-7"], "Error: the argument ('9-7') for option '--donors' is invalid\n"), _bad("max-segments", "x")],
}


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    subprocess.run(["make", "-s", "-C", HOST], check=True)        # (libedsx.so itself comes from build())
    d = tmp_path_factory.mktemp("front")
    eds = b"{ACGTAC}{A,ACA,}{CGTTTTT}{,T}{GG}{C,G}{TTTTTTTTTT}{A,C,G}{}"
    (d / "x.eds").write_bytes(eds)
    (d / "x.seds").write_bytes(b"{0}{1,3}{2}{4}{0}{1,2}{3,4}{0}{1,2,3}{5,6}{0}{1,5}{2,6}{3}{0}")
    (d / "y.eds").write_bytes(eds)                               # without its sources
    (d / "names.txt").write_text("a\nb\nc\nd\ne\nf\n")
    (d / "ids.txt").write_text("1\n2\n")
    (d / "badids.txt").write_text("1\n\ntwo\n")
    (d / "badq.tsv").write_text("# c\n1\t0\t2\n1\tx\t2\n")
    (d / "bad.bed").write_text("1\t0\t5\n1\t5\n")
    return d


def _run(tool, args, d):
    r = subprocess.run([os.path.join(BUILD, tool)] + [a.replace("{d}", str(d)) for a in args], capture_output=True, text=True,
                       stdin=subprocess.DEVNULL, cwd=str(d))
    lines = r.stderr.splitlines(True)
    err = "".join("[Performance]\n" if l.startswith("[Performance] Runtime: ") else l for l in lines)
    return r.returncode, r.stdout, err


@pytest.mark.parametrize("tool", sorted(CLI))
def test_cli_without_device(tool, inputs):
    before = sorted(os.listdir(inputs))
    for args, err in CLI[tool]:
        assert _run(tool, args, inputs) == (1, "", err.replace("{d}", str(inputs)) + "[Performance]\n"), args
    assert _run(tool, ["--help"], inputs) == (0, open(os.path.join(HELP, tool + ".txt")).read(), "[Performance]\n")
    assert _run(tool, X + ["-h"], inputs)[1:] == _run(tool, ["--help"], inputs)[1:]
    assert sorted(os.listdir(inputs)) == before                  # none of these runs writes a file
