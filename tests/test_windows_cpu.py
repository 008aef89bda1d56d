"""-F <len>,<step> (reads sampled from long FASTA sequences), host side: the library's planner and `hisat2-align-amd --parse-only` against a pure-Python
restatement of the reference's FastaContinuousPatternSource (windows_util.restate, itself pinned to the QNAME column of the reference binary where oracle/_ref is
built); -s / -u on read ids; both spellings of the argument; every refusal; and the stand-alone checker of the expansion arithmetic under ASan + UBSan."""
import os
import subprocess

import numpy as np
import pytest

import windows_util as W
from hisat2_amd import api

pytestmark = pytest.mark.skipif(not os.path.exists(W.CLI), reason="hisat2-align-amd not built (python __graft_entry__.py)")

LEN_STEP = ((30, 10), (30, 1), (1, 1), (33, 0), (128, 129), (1024, 5))
COMBOS = ((1, 1), (700, 4), (1 << 20, 7))          # (--batch, -p)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    files = W.sample_files(np.random.default_rng(20261018))
    paths = W.write_files(tmp_path_factory.mktemp("wf"), files)
    return files, paths, {ls: W.restate(files, *ls) for ls in LEN_STEP}


def parse_only(args):
    r = subprocess.run([W.CLI, "--parse-only", "-x", "unused"] + [str(a) for a in args], check=True, capture_output=True, text=True)
    lines = r.stdout.split("\n")
    t = lines[0].split()
    ids = [tuple(int(x) for x in l.split()) for l in lines[1:] if l]
    return (int(t[0]), int(t[1]), int(t[2], 16), int(t[3]), int(t[4])), ids


def test_restatement_has_the_cases(case):
    """the inputs hold what they are meant to: names without a prefix, an N run, a record that yields nothing, ids that carry across the two files"""
    reads = case[2][(30, 10)]
    names = [r[0] for r in reads]
    assert names[:3] == ["0", "10", "20"] and "qa_0" in names and "tab_0" in names and "qb_0" in names and "qc_0" in names
    assert not any(n.startswith("short") or n.startswith("empty") for n in names)
    assert any(r[1] == "N" * 30 for r in reads) and any("N" in r[1] and r[0].startswith("tab_") for r in reads)
    qb0 = next(r for r in reads if r[0] == "qb_0")
    assert qb0[2] > 0 and qb0[2] != reads.index(qb0)              # rdid is no running count
    assert len(case[2][(33, 0)]) == 5 and len(case[2][(1, 1)]) == sum(len(r[1]) for r in case[2][(1, 1)])


@pytest.mark.skipif(not os.path.exists(os.path.join(W.REF, "hisat2-align-s")), reason="needs oracle/_ref")
@pytest.mark.parametrize("ls", ((30, 10), (33, 0), (128, 129)))
def test_restatement_equals_the_reference(case, g1_index, tmp_path, ls):
    """names and order of the restatement == QNAME of `hisat2-align-s -p 1 -F` (the .gz file inflated: one variable less)"""
    files, _, want = case
    paths = W.write_files(tmp_path, files, gz_last=False)
    out = subprocess.run([os.path.join(W.REF, "hisat2-align-s"), "-p", "1", "--no-hd", "--no-spliced-alignment", "-x", g1_index, "-F", "%d,%d" % ls, "-U", ",".join(paths)],
                         check=True, capture_output=True, text=True).stdout
    got = [(l.split("\t")[0], l.split("\t")[9]) for l in out.splitlines() if not (int(l.split("\t")[1]) & 256)]
    assert got == [(nm, s) for nm, s, _ in want[ls]]


@pytest.mark.parametrize("batch,p", COMBOS)
@pytest.mark.parametrize("ls", LEN_STEP)
def test_parse_only_equals_the_restatement(case, ls, batch, p):
    _, paths, want = case
    # (-p above 1 with a step other than 1 is taken only without the splice-site window: test_refused_arguments)
    got = parse_only(["-F", "%d,%d" % ls, "-U", ",".join(paths), "--batch", batch, "-p", p] + (["--no-temp-splicesite"] if p > 1 else []))
    assert got == W.expected(want[ls], batch)


@pytest.mark.parametrize("ls", LEN_STEP)
def test_planner_ranges_equal_the_restatement(case, ls):
    """the segments of any range of reads, expanded: a batch boundary may fall inside a record"""
    files, _, want = case
    reads = want[ls]
    plan = api.WindowPlan(*ls)
    for f in files:
        plan.add_file(f)
    assert plan.n_reads == len(reads) and plan.info().next_rdid >= reads[-1][2] + 1
    text, pre = plan.text(), plan.prefixes()
    rng = np.random.default_rng(5)
    ranges = [(0, len(reads)), (len(reads) - 1, 1)] + [(int(a), int(rng.integers(1, 40))) for a in rng.integers(0, len(reads), size=12)]
    for first, n in ranges:
        n = min(n, len(reads) - first)
        codes, offs, names, noffs, ids = api.expand_windows(text, plan.segments(first, n), ls[0], ls[1], pre)
        w = reads[first:first + n]
        assert bytes(codes) == b"".join(bytes(W.CODE[c] for c in s) for _, s, _ in w)
        assert [names[noffs[i]:noffs[i + 1]].decode() for i in range(n)] == [nm for nm, _, _ in w]
        assert list(ids) == [r[2] for r in w] and list(offs) == [ls[0] * i for i in range(n + 1)]
    plan.close()


def test_skip_and_upto_act_on_read_ids(case):
    """-s / -u cut inside a record and across the file boundary; a skip past a gap of ids starts at the next id there is"""
    _, paths, want = case
    reads = want[(30, 10)]
    qb0 = next(r for r in reads if r[0] == "qb_0")[2]
    for skip, upto in ((100, 50), (qb0 - 35, 120), (qb0 + 5, 1 << 30), (0, 7), (reads[-1][2] + 1, 10)):
        sel = W.select(reads, skip, upto)
        args = ["-F", "30,10", "-U", ",".join(paths), "-s", skip, "-u", upto, "--batch", 64]
        if not sel:
            assert parse_only(args)[0][0] == 0
            continue
        assert parse_only(args) == W.expected(sel, 64)


def test_both_spellings_of_the_argument(case):
    _, paths, want = case
    for arg in ("30,10", "k:30,i:10"):
        assert parse_only(["-F", arg, "-U", ",".join(paths), "--batch", 700]) == W.expected(want[(30, 10)], 700)
    # -5 / -3 are not applied by this source; the last of -f / -q / -F decides the format
    assert parse_only(["-f", "-F", "30,10", "-5", 3, "-3", 4, "-U", ",".join(paths), "--batch", 700]) == W.expected(want[(30, 10)], 700)
    r = subprocess.run([W.CLI, "--parse-only", "-x", "unused", "-F", "30,10", "-f", "-U", paths[1]], check=True, capture_output=True, text=True)
    assert len(r.stdout.splitlines()) == 1 and int(r.stdout.split()[0]) == 2       # plain FASTA: one read per '>' record


REFUSALS = (
    (["-1", "{u}", "-2", "{u}"], "-1/-2"), (["--tab5", "{u}"], "--tab5"), (["--tab6", "{u}"], "--tab6"), (["--12", "{u}"], "--12"), (["--qseq", "-U", "{u}"], "--qseq"),
    (["-c", "-U", "ACGT"], "-c"), (["-r", "-U", "{u}"], "-r"),
    (["--wrapper", "basic-0", "--un", "x", "-U", "{u}"], "--un"), (["--wrapper", "basic-0", "--al-gz", "x", "-U", "{u}"], "--al"),
)


@pytest.mark.parametrize("extra,word", REFUSALS)
def test_refused_together_with_F(case, extra, word):
    u = case[1][0]
    r = subprocess.run([W.CLI, "-x", "unused", "-F", "30,10"] + [a.replace("{u}", u) for a in extra], capture_output=True, text=True)
    assert r.returncode == 1 and "-F" in r.stderr and word in r.stderr and len(r.stderr.strip().splitlines()) == 1


@pytest.mark.parametrize("args,env,words", (
    (["-F", "0,10"], {}, ("-F", "0")),
    (["-F", "1025,10"], {}, ("-F", "1024")),
    (["-F", "30,10", "-p", "2"], {}, ("-F", "-p", "temporary-splice-site")),
    (["-F", "30,0", "-p", "3"], {}, ("-F", "-p", "temporary-splice-site")),
    (["-F", "30,1", "-p", "2"], {"H2G_WINDOW_FIRST_ID": str((1 << 32) - 100)}, ("-F", "2^32")),
    (["-F", "30,10", "-p", "1"], {"H2G_WINDOW_FIRST_ID": str((1 << 32) - 100)}, ("-F", "2^32")),
    (["-F", "30;10"], {}, ("-F", "<len>,<step>")),
))
def test_refused_arguments(case, args, env, words):
    """len 0, len beyond the reference's ring, a step other than 1 with a splice-site window, ids past 2^32 - 1 with temporary splice sites: one line, before any device is touched"""
    r = subprocess.run([W.CLI, "-x", "unused", "-U", case[1][0]] + args, capture_output=True, text=True, env=dict(os.environ, **env))
    assert r.returncode == 1 and all(w in r.stderr for w in words) and len(r.stderr.strip().splitlines()) == 1


def test_every_p_is_taken_without_a_splice_site_window(case):
    """--no-temp-splicesite / --no-spliced-alignment: any step at any -p passes the option checks (--parse-only ends the run before a device is needed)"""
    for mode in ("--no-temp-splicesite", "--no-spliced-alignment"):
        assert parse_only(["-F", "30,10", "-p", 4, mode, "-U", ",".join(case[1]), "--batch", 700]) == W.expected(case[2][(30, 10)], 700)


def test_expansion_arithmetic_under_sanitizers(tmp_path):
    """tests/windows/win_check.cpp drives the functions of csrc/h2g_windows.h lane by lane, as the kernels do, against a naive loop: clean under ASan + UBSan"""
    exe = str(tmp_path / "win_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", exe,
                    os.path.join(W.ROOT, "tests", "windows", "win_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout + r.stderr
