"""The dense SA table (hisat2_amd/csrc/h2g_core.h: sa_dense_build_rows, sa_resolve_row; h2g_fast.h fast_op_gcoords) on the host: the table built by the
same code the device runs equals the canonical walk for EVERY row, and the fast path and the general machine give the same bytes with the table
attached as without it (work counters included).  With the saturation threshold lowered to 8 most rows miss the table and take the fallback."""
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


@pytest.fixture(scope="module")
def libs():
    """the harness tests/dense_sa/h2g_dense_emul.cpp in the shipped kernel's configuration: [255] as shipped, [8] with the threshold lowered"""
    out = tempfile.mkdtemp(prefix="h2dense")
    src = os.path.join(HERE, "dense_sa", "h2g_dense_emul.cpp")
    r = {}
    for sat in (255, 8):
        so = os.path.join(out, f"libh2gemu_dense{sat}.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-w", "-fPIC", "-shared", "-DH2G_GHIT_EDITS=32", "-DH2G_NEW_EDITS=24", "-DFG_ALIGN_MATE=0",
                        f"-DH2G_SA_DIST_SAT={sat}u", "-o", so, src], check=True)
        r[sat] = so
    return r


@pytest.fixture(scope="module")
def genome():
    """the shape of test_fast_path_cpu.py's genome fixture"""
    tmp = tempfile.mkdtemp(prefix="h2densefa")
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
    assert e.dense_sat() == sat
    e.dense_build()
    wrong, resolved_wrong, saturated, longest = (int(x) for x in e.table_check("dense", 4))
    print(f"sat {sat}: {wrong} wrong entries, {resolved_wrong} rows resolved differently, {saturated} rows not in the table, longest walk {longest}")
    assert wrong == 0 and resolved_wrong == 0
    return saturated, longest


@pytest.mark.parametrize("sat", [255, 8])
def test_table_equals_the_walk_on_every_row_g1(libs, g1_index, monkeypatch, sat):
    e = _emu(monkeypatch, libs[sat], g1_index)
    saturated, longest = _check_every_row(e, sat)
    assert (saturated > 0) == (longest >= sat)
    if sat == 8:
        assert saturated > 0                                   # the fallback was exercised


@needs_builder
@pytest.mark.parametrize("sat", [255, 8])
def test_table_equals_the_walk_on_every_row(libs, genome, monkeypatch, sat):
    e = _emu(monkeypatch, libs[sat], genome[0])
    saturated, longest = _check_every_row(e, sat)
    assert (saturated > 0) == (longest >= sat)
    if sat == 8:
        assert saturated > 0


def _run_both(monkeypatch, lib, base, reads1, reads2):
    """without and with the table: fast path vs machine (FC.fast_check), and the digests of the raw rows both of them write"""
    res = []
    for on in (0, 1):
        e = _emu(monkeypatch, lib, base)
        e.dense_build()
        e.dense_attach(on)
        r = FC.fast_check(base, list(reads1), None if reads2 is None else list(reads2), emu=e)
        res.append((r, _digest(e, reads1, reads2)))
    return res


def _digest(e, reads1, reads2):
    e.load_reads(reads1)
    out = e.table_digest("dense", reads2)
    return dict(machine=int(out[0]), fast=int(out[1]), completed=int(out[2]), nsteps=int(out[3]))


PAIR_CASES = [
    dict(n=6000, rdlen=101, sub=0.005),
    dict(n=4000, rdlen=101, sub=0.03),
    dict(n=3000, rdlen=75, sub=0.01, frag_mean=400, frag_sd=200),
    dict(n=3000, rdlen=125, sub=0.02),
    dict(n=2000, rdlen=40, sub=0.01, frag_mean=200, frag_sd=40),
]
READ_CASES = [
    dict(n=8000, rdlen=101, sub=0.005),
    dict(n=4000, rdlen=101, sub=0.02, indel=0.002),
    dict(n=3000, rdlen=60, sub=0.02, nrate=0.01),
    dict(n=3000, rdlen=128, sub=0.01),
    dict(n=1000, rdlen=150, sub=0.01),
]


def _same(res):
    (r0, b0), (r1, b1) = res
    assert r0["mismatching"] == 0 and r1["mismatching"] == 0, (r0, r1)           # fast path == machine, each with its own way to the rows
    assert r0["completed"] == r1["completed"] and r0["bails"] == r1["bails"] and (r0["done"] == r1["done"]).all()
    print(b0, b1)
    assert b0 == b1 and b0["nsteps"] > 0                                         # the rows of both: the same bytes, nsteps included
    assert b1["completed"] == r1["completed"]
    return r1


@needs_builder
@pytest.mark.parametrize("sat", [255, 8])
@pytest.mark.parametrize("case", PAIR_CASES)
def test_pairs_same_bytes_with_and_without_the_table(libs, genome, monkeypatch, case, sat):
    base, contigs = genome
    m1, m2 = synth.make_pairs(contigs, case["n"], case["rdlen"], 77 + case["n"], frag_mean=case.get("frag_mean", 300), frag_sd=case.get("frag_sd", 30), sub_rate=case["sub"])
    r = _same(_run_both(monkeypatch, libs[sat], base, m1, m2))
    assert r["completed"] > 0.2 * r["n"], r


@needs_builder
@pytest.mark.parametrize("sat", [255, 8])
@pytest.mark.parametrize("case", READ_CASES)
def test_reads_same_bytes_with_and_without_the_table(libs, genome, monkeypatch, case, sat):
    base, contigs = genome
    reads, _ = synth.make_reads(contigs, case["n"], case["rdlen"], 5 + case["n"], sub_rate=case["sub"], indel_rate=case.get("indel", 0.0), n_rate=case.get("nrate", 0.0))
    r = _same(_run_both(monkeypatch, libs[sat], base, reads, None))
    if case["rdlen"] <= 128:
        assert r["completed"] > 0.4 * r["n"], r


# ---------------------------------------------------------------- fragmented assembly (tests/frag_cases.py)
@pytest.mark.parametrize("sat", [255, 8])
def test_table_equals_the_walk_on_every_row_gfrag(libs, golden_dir, tmp_path, monkeypatch, sat):
    import parity_cases as PC
    e = _emu(monkeypatch, libs[sat], PC.unpack_index(golden_dir, "gfrag", tmp_path))
    saturated, longest = _check_every_row(e, sat)
    assert (saturated > 0) == (longest >= sat)


@needs_builder
@pytest.mark.parametrize("sat", [255, 8])
def test_fragmented_assembly_same_bytes_with_and_without_the_table(libs, monkeypatch, sat):
    """the fast pass resolves rows from the dense table and then tests every element for a straddle itself: reads and pairs that straddle two texts or two
    fragments, hang off contig ends or abut N runs give the same bytes with the table as with the walk"""
    import frag_cases as FR
    g, reads, _, m1, m2, _ = FR.live_case()
    base = FR.build_index(g, tempfile.mkdtemp(prefix="h2densefrag"), os.path.dirname(BUILD))
    r = _same(_run_both(monkeypatch, libs[sat], base, reads, None))
    assert r["completed"] > 0, r
    r = _same(_run_both(monkeypatch, libs[sat], base, m1, m2))
    assert r["completed"] > 0, r
