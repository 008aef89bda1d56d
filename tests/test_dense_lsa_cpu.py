"""The dense table of local rows (hisat2_amd/csrc/h2g_align.h: lsa_build_rows, lsa_resolve_row; h2g_fast.h fast_op_lcoords_walk) on the host: the table
built by the code the device runs equals the canonical walk for EVERY row of every local index ('$' rows included), the fast path and the general machine
give the same bytes with the table attached as without it (work counters included), and a walk stored half way by a run without the table is finished
correctly by a run with it.  With the saturation threshold lowered to 4 most rows miss the table and take the fallback (one local row in eight is sampled)."""
import os
import subprocess
import tempfile

import pytest

from hisat2_amd import synth
import fast_check as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
BUILD = os.path.join(ROOT, "oracle", "_ref", "hisat2-build-s")
needs_builder = pytest.mark.skipif(not os.path.exists(BUILD), reason="needs oracle/_ref/hisat2-build-s")
SATS = [255, 4]


@pytest.fixture(scope="module")
def libs():
    """the harness tests/dense_lsa/h2g_lsa_emul.cpp in the shipped kernel's configuration: [255] as shipped, [4] with the threshold lowered"""
    out = tempfile.mkdtemp(prefix="h2lsa")
    src = os.path.join(HERE, "dense_lsa", "h2g_lsa_emul.cpp")
    r = {}
    for sat in SATS:
        so = os.path.join(out, f"libh2gemu_lsa{sat}.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-w", "-fPIC", "-shared", "-DH2G_GHIT_EDITS=32", "-DH2G_NEW_EDITS=24", "-DFG_ALIGN_MATE=0",
                        f"-DH2G_LSA_DIST_SAT={sat}u", "-o", so, src], check=True)
        r[sat] = so
    return r


@pytest.fixture(scope="module")
def genome():
    """600 kbp in three contigs with N gaps (the shape of test_dense_sa_cpu.py's genome): local indexes at contig ends, indexes shorter than the
    interval and indexes of more than one fragment"""
    tmp = tempfile.mkdtemp(prefix="h2lsafa")
    contigs = synth.make_genome([400000, 150000, 60000], 9101, n_gaps=3, gap_len=300, repeats=40, repeat_len=500)
    fa = os.path.join(tmp, "g.fa")
    synth.write_fasta(fa, contigs)
    base = os.path.join(tmp, "g")
    subprocess.run([BUILD, "-q", fa, base], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return base, contigs


def _emu(monkeypatch, lib, base):
    from h2gemu_py import Emu
    monkeypatch.setenv("H2GEMU_LIB", lib)
    return Emu(base)


def _check_every_row(e, sat):
    assert e.lsa_sat() == sat
    e.lsa_build()
    out = e.table_check("lsa", 10)
    r = dict(zip(("wrong", "resolved_wrong", "saturated", "longest", "rows", "dollar", "multi_frag", "short", "empty", "n"), (int(x) for x in out)))
    print(f"sat {sat}: {r}")
    assert r["wrong"] == 0 and r["resolved_wrong"] == 0
    assert r["n"] > 0 and r["rows"] > 0
    assert r["dollar"] == r["n"] - r["empty"]                    # the '$' row of every (non-empty) local index was among the rows
    assert (r["saturated"] > 0) == (r["longest"] >= sat)
    if sat == 4:
        assert r["saturated"] > 0                                # the fallback was exercised
    return r


@pytest.mark.parametrize("sat", SATS)
def test_table_equals_the_walk_on_every_local_row_g1(libs, g1_index, monkeypatch, sat):
    _check_every_row(_emu(monkeypatch, libs[sat], g1_index), sat)


@needs_builder
@pytest.mark.parametrize("sat", SATS)
def test_table_equals_the_walk_on_every_local_row(libs, genome, monkeypatch, sat):
    r = _check_every_row(_emu(monkeypatch, libs[sat], genome[0]), sat)
    assert r["n"] >= 3 and r["short"] > 0 and r["multi_frag"] > 0    # contig ends, indexes shorter than the interval, nFrag > 1
    if sat == 4:
        assert r["saturated"] > r["rows"] // 4                   # one row in 8 is sampled: (7/8)^4 = 0.59 of the rows walk 4 steps or more


def _digest(e, reads1, reads2, midwalk=0):
    e.load_reads(reads1)
    out = e.table_digest("lsa", reads2, midwalk)
    return dict(machine=int(out[0]), fast=int(out[1]), completed=int(out[2]), nsteps=int(out[3])), int(out[4])


def _run_both(monkeypatch, lib, base, reads1, reads2):
    """without and with the table: fast path vs machine (FC.fast_check), and the digests of the raw rows both of them write; then the fast path once more
    with the table switched on in the middle of each read's first stored walk"""
    res = []
    for on in (0, 1):
        e = _emu(monkeypatch, lib, base)
        e.lsa_build()
        e.lsa_attach(on)
        r = FC.fast_check(base, list(reads1), None if reads2 is None else list(reads2), emu=e)
        res.append((r, _digest(e, reads1, reads2)[0]))
    e = _emu(monkeypatch, lib, base)                                             # (a fresh instance, as the two above: the digests are compared across instances)
    e.lsa_build()
    mid, switched = _digest(e, reads1, reads2, midwalk=1)
    return res, mid, switched


def _same(res, mid, switched):
    (r0, b0), (r1, b1) = res
    assert r0["mismatching"] == 0 and r1["mismatching"] == 0, (r0, r1)           # fast path == machine, each with its own way to the rows
    assert r0["completed"] == r1["completed"] and r0["bails"] == r1["bails"] and (r0["done"] == r1["done"]).all()
    print(b0, b1, mid, switched)
    assert b0 == b1 and b0["nsteps"] > 0                                         # the rows of both: the same bytes, nsteps included
    assert b1["completed"] == r1["completed"]
    assert switched > 0                                                          # walks were stored half way, and finished with the table
    assert (mid["fast"], mid["completed"]) == (b0["fast"], b0["completed"])      # ... to the bytes of the uninterrupted run (the fast path's rows: the switch is its alone)
    return r1


PAIR_CASES = [
    dict(n=3000, rdlen=101, sub=0.005),
    dict(n=2000, rdlen=101, sub=0.03),
    dict(n=1500, rdlen=75, sub=0.01, frag_mean=400, frag_sd=200),
]
READ_CASES = [
    dict(n=4000, rdlen=101, sub=0.005),
    dict(n=2000, rdlen=101, sub=0.02, indel=0.002),
    dict(n=1500, rdlen=60, sub=0.02, nrate=0.01),
]


@needs_builder
@pytest.mark.parametrize("sat", SATS)
@pytest.mark.parametrize("case", PAIR_CASES)
def test_pairs_same_bytes_with_and_without_the_table(libs, genome, monkeypatch, case, sat):
    base, contigs = genome
    m1, m2 = synth.make_pairs(contigs, case["n"], case["rdlen"], 77 + case["n"], frag_mean=case.get("frag_mean", 300), frag_sd=case.get("frag_sd", 30), sub_rate=case["sub"])
    r = _same(*_run_both(monkeypatch, libs[sat], base, m1, m2))
    assert r["completed"] > 0.2 * r["n"], r


@needs_builder
@pytest.mark.parametrize("sat", SATS)
@pytest.mark.parametrize("case", READ_CASES)
def test_reads_same_bytes_with_and_without_the_table(libs, genome, monkeypatch, case, sat):
    base, contigs = genome
    reads, _ = synth.make_reads(contigs, case["n"], case["rdlen"], 5 + case["n"], sub_rate=case["sub"], indel_rate=case.get("indel", 0.0), n_rate=case.get("nrate", 0.0))
    r = _same(*_run_both(monkeypatch, libs[sat], base, reads, None))
    assert r["completed"] > 0.4 * r["n"], r
