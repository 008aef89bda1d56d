"""-m gpu: fragmented assemblies on the device (tests/frag_cases.py) — hundreds of texts, 300+ fragments, N runs of every small length, all-N records, reads and
pairs at every contig end.  The primitive checks are the ones tests/test_emul_golden.py runs on the host instantiation (tests/parity_cases.py), here through the
C ABI against the committed gfrag vectors of the reference's classes and the C oracle; the go() cases are the ones of tests/test_go_parity_cpu.py, here against
oracle/_ref/hisat2-align-s, through the C ABI and through the command line."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import frag_cases as FC
import h2o_py as H
import parity_cases as PC
import sam_util as SU
from hisat2_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
CLI = os.path.join(ROOT, "hisat2_amd", "hisat2-align-amd")
needs_ref = pytest.mark.skipif(not os.path.exists(os.path.join(REF, "hisat2-align-s")), reason="needs oracle/_ref")


@pytest.fixture(scope="module")
def gfrag_index(tmp_path_factory, golden_dir):
    return PC.unpack_index(golden_dir, "gfrag", tmp_path_factory.mktemp("gfrag"))


def _stream(base, golden_dir, quals=None):
    ix = api.Index(base, device=0)
    seqs, codes, offs = PC.load_frag_reads(golden_dir)
    st = api.Stream(ix, max_reads=len(seqs), max_bases=codes.size)
    st.set_reads(codes, offs, quals)
    st.seqs = seqs
    return ix, st


@pytest.fixture(scope="module")
def fgpu(gfrag_index, golden_dir):
    ix, st = _stream(gfrag_index, golden_dir)
    yield st
    st.close()
    ix.close()


def test_index_info(fgpu, golden_dir):
    d = PC.check_frag_info(fgpu.ix.info, golden_dir)
    assert d["nFrag"] >= 300


def test_coords_golden(fgpu, golden_dir):
    n, nstrad, nrej = PC.check_frag_coords(fgpu, golden_dir)
    assert n > 2000 and nstrad >= FC.MINIMA["coords_straddled"] and nrej >= FC.MINIMA["coords_rejected"]


@pytest.mark.parametrize("dense", ["default", "2"])
def test_sa_resolve_every_row_vs_oracle(oracle_lib, gfrag_index, golden_dir, monkeypatch, dense):
    """every row of the index, ranges, len 1 / 20 / 101, rejectStraddle 0 / 1; with H2G_DENSE_SA=2 the rows come from the dense table, which must itself equal the
    canonical walk on every row"""
    if dense == "2":
        monkeypatch.setenv("H2G_DENSE_SA", "2")
    ix, st = _stream(gfrag_index, golden_dir)
    try:
        if dense == "2":
            assert ix.dense_sa(verify=True) == (True, 0)
        oix = H.load_index(oracle_lib, gfrag_index)
        n, nstrad, nrej = PC.check_frag_sa_resolve_vs_oracle(st, oracle_lib, oix, ix.info.gbwtLen)
        assert n == ix.info.gbwtLen + 5000 and nstrad >= FC.MINIMA["sa_straddled"] and nrej >= FC.MINIMA["sa_rejected"]
    finally:
        st.close()
        ix.close()


@pytest.mark.parametrize("fn", ["probe_gfrag_extend.txt.gz", "probe_gfrag_extend_fq.txt.gz"])
def test_extend_golden(fgpu, gfrag_index, golden_dir, fn):
    fq = fn.endswith("_fq.txt.gz")
    ix = st = None
    if fq:
        seqs, _, _ = PC.load_frag_reads(golden_dir)
        ix, st = _stream(gfrag_index, golden_dir, quals=FC.seeded_quals(seqs, FC.GFRAG_SEED + 2))
    try:
        n, nstop = PC.check_frag_extend(st if fq else fgpu, golden_dir, fn, fgpu.seqs)
        assert n > 10000 and nstop >= FC.MINIMA["extend_stop_at_stretch_end" + ("_fq" if fq else "")]
    finally:
        if fq:
            st.close()
            ix.close()


def test_fm_search_and_seed_stage(fgpu, oracle_lib, gfrag_index, golden_dir):
    oix = H.load_index(oracle_lib, gfrag_index)
    n, ncont = PC.check_frag_fm_search(fgpu, golden_dir, oracle_lib, oix, fgpu.seqs)
    assert n == 3000 and ncont >= FC.MINIMA["psearch_continued"]
    fgpu.seed_extend_run(fgpu.seed_params(no_spliced=True))
    got = fgpu.seed_extend_fetch()
    want = PC.oracle_seed_extend_ragged(oracle_lib, oix, fgpu.seqs, 0)
    PC.assert_seed_equal(got, want)
    assert (want["ncoords"] > 0).sum() >= FC.MINIMA["seed_anchored"] and (want["straddled"] > 0).sum() >= FC.MINIMA["seed_straddled"]


def test_ext_search_and_local_index_of(fgpu, golden_dir):
    """local indexes of a few dozen to a few hundred bases: staged in LDS (stage_min = 1: every bucket) == searched from HBM == the reference's classes"""
    L = api.lib()
    lof = lambda t, o: L.h2g_local_index_of(fgpu.ix.h, t, o)   # noqa: E731
    n, nabsent = PC.check_frag_local_index_of(lof, golden_dir)
    assert n > 1000 and nabsent >= FC.MINIMA["localof_absent"]
    stats = {}
    for stage_min in (1, 0):
        def search(qs):
            hits, stats[stage_min] = fgpu.ext_search((api.ExtSearchQuery * len(qs))(*qs), stage_min=stage_min)
            return hits
        n, nel = PC.check_ext_search(search, lof, golden_dir, "probe_gfrag_extsearch.txt.gz")
        assert n == 4500 and nel >= FC.MINIMA["extsearch_with_elements"]
    assert stats[1].n_staged > 0 and stats[0].n_staged == 0 and stats[1].n_local == stats[0].n_local == 3000


# ---------------------------------------------------------------- go() against the live reference
class _Out:
    def __init__(self, r):
        self.overflow, self.depth = int(r["overflow"]), int(r["depth"])


def _backend(base, reads, qnames, refnames, bowtie2_dp=0, quals=None, options=()):
    from test_gpu_align import gpu_align
    res, aln, _ = gpu_align(base, reads, qnames, bowtie2_dp=bowtie2_dp, quals=quals, options=options)
    return [_Out(r) for r in res], SU.render_selected(res, aln, refnames, reads, qnames)


@needs_ref
@pytest.mark.parametrize("case", [
    dict(),
    dict(fastq=True, extra=("--mp", "4,2")),
    dict(extra=("-k", "10")),
    dict(extra=("--no-softclip",)),
    dict(extra=("--bowtie2-dp", "2"), bowtie2_dp=2),
    dict(snps=True),
], ids=["plain", "fastq-mp", "k10", "no-softclip", "bowtie2-dp2", "snp-graph"])
def test_live_reference_fragmented_assembly(case):
    import functools
    import fuzz_align as F
    case = dict(case)
    g, reads, labels, _, _, _ = FC.live_case()
    variants = None
    if case.pop("snps", False):
        g = FC.make_frag_genome(FC.LIVE_SEED, FC.GRAPH_TOTAL)
        variants, alt = FC.make_frag_snps(g, FC.LIVE_SEED + 5)
        reads, labels = FC.make_frag_reads(alt, FC.LIVE_SEED + 6, 3000)
    dp = case.pop("bowtie2_dp", 0)
    info = {}
    bad, _ = F.run_case(FC.LIVE_SEED, genome=(g.records, g.names), reads=reads, variants=variants, info=info, verbose=5,
                        backend=functools.partial(_backend, bowtie2_dp=dp), **case)
    assert bad == 0 and info["overflow"] == 0
    if not case and not variants:
        FC.assert_teeth(FC.read_teeth(info["want"], labels), FC.LIVE_READ_MINIMA)


def _pair_backend(base, m1, m2, q1, q2):
    import fuzz_pairs as F
    c1, o1 = F.flatten(m1)
    c2, o2 = F.flatten(m2)
    ix = api.Index(base, device=0)
    st = api.Stream(ix, max_reads=len(m1), max_bases=max(c1.size, c2.size))
    st.set_reads(c1, o1)
    st.set_read_names(q1)
    st.set_mates(c2, o2, q2)
    st.align_pairs_run(st.align_params())
    res, a1, a2 = st.align_pairs_fetch()
    st.close()
    ix.close()
    return res, a1, a2


@needs_ref
def test_live_reference_fragmented_assembly_pairs():
    import fuzz_pairs as F
    g, _, _, m1, m2, plabels = FC.live_case()
    info = {}
    bad, _ = F.run_case(FC.LIVE_SEED, genome=(g.records, g.names), pairs=(m1, m2), info=info, verbose=5, backend=_pair_backend, stride=api.PAIR_RES_CAP)
    assert bad == 0 and info["overflow"] == 0
    FC.assert_teeth(FC.pair_teeth(info["want"], plabels), FC.LIVE_PAIR_MINIMA)


@needs_ref
@pytest.mark.parametrize("mode", ["unpaired-spliced", "paired"])
def test_command_line(tmp_path, mode):
    """hisat2-align-amd against hisat2-align-s: every body line, the alignment summary, and the header — @SQ lines of the texts only, in text order (the all-N
    records are not in the index).  Unpaired: spliced alignment with --no-temp-splicesite (reads whose halves lie either side of an N run come out spliced)."""
    import fuzz_pairs as FP
    import sam_lines as SL
    from test_sam_lines import diff_lines
    g, reads, _, m1, m2, _ = FC.live_case()
    tmp = str(tmp_path)
    base = FC.build_index(g, tmp, REF)
    if mode == "paired":
        f1, f2 = os.path.join(tmp, "r1.fa"), os.path.join(tmp, "r2.fa")
        FP.write_fasta_reads(f1, m1)
        FP.write_fasta_reads(f2, m2)
        common = ["-f", "--no-spliced-alignment", "-x", base, "-1", f1, "-2", f2]
    else:
        rfa = os.path.join(tmp, "r.fa")
        FC.write_reads(rfa, reads)
        common = ["-f", "--no-temp-splicesite", "-x", base, "-U", rfa]
    ref_sam, amd_sam, ref_err, amd_err = (os.path.join(tmp, x) for x in ("ref.sam", "amd.sam", "ref.err", "amd.err"))
    subprocess.run([os.path.join(REF, "hisat2-align-s"), "-p", "1", "-S", ref_sam] + common, check=True, stdout=subprocess.DEVNULL, stderr=open(ref_err, "w"))
    subprocess.run([CLI, "-p", "4", "--batch", "1000", "-S", amd_sam] + common, check=True, stderr=open(amd_err, "w"))
    want = SL.body_lines(ref_sam)
    assert len(want) >= 3000 and diff_lines(SL.body_lines(amd_sam), want) == 0
    assert open(amd_err).read() == open(ref_err).read()
    hdr = [l for l in open(amd_sam) if l.startswith("@")]
    ref_hdr = [l for l in open(ref_sam) if l.startswith("@")]
    assert hdr[:-1] == ref_hdr[:-1] and len([l for l in hdr if l.startswith("@SQ")]) == len(g.texts)
    assert [l.split("\t")[1][3:] for l in hdr if l.startswith("@SQ")] == g.text_names()
    if mode != "paired":
        assert sum(1 for l in want if "N" in l.split("\t")[5]) >= 22      # half of the 44 spliced lines the reference writes for these reads


@needs_ref
def test_fast_pass_equals_the_machine_on_a_fragmented_assembly():
    """fast_digest.py with the fast pass on and off (separate processes: the switch is read once): 20 000 pairs (P1-P3) and 20 000 reads (A, B, C, F, G) of 101 bases"""
    g = FC.live_case()[0]
    tmp = tempfile.mkdtemp(prefix="h2fpfrag")
    base = FC.build_index(g, tmp, REF)
    n = 20000
    reads, _ = FC.make_frag_reads(g, FC.LIVE_SEED + 11, n, lens=(101,), classes="ABCFG")
    m1, m2, _ = FC.make_frag_pairs(g, FC.LIVE_SEED + 12, n, rdlen=101, classes=("P1", "P2", "P3"), contained=False)
    npz = os.path.join(tmp, "reads.npz")
    np.savez(npz, m1=np.stack(m1), m2=np.stack(m2), reads=np.stack(reads))
    got = {}
    for fast in ("0", "1"):
        env = dict(os.environ, H2G_GO_FAST=fast, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fast_digest.py"), base, npz], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got[fast] = json.loads(r.stdout.strip().splitlines()[-1])
    print(got)
    for k in ("pairs", "reads"):
        assert got["0"][k]["fast"] == 0 and got["1"][k]["fast"] > 0
        assert got["1"][k]["fast"] + got["1"][k]["handed_on"] == n
        assert got["0"][k]["overflow"] == 0 and got["1"][k]["overflow"] == 0
        assert got["0"][k]["aligned"] == got["1"][k]["aligned"]
        assert got["0"][k]["sha"] == got["1"][k]["sha"], k

