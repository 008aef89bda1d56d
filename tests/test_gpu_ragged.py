"""-m gpu: trimmed read sets on the device (tests/ragged_cases.py) — every read length from 0 to 300 in one batch, mates of different lengths, empty reads.  The cases
are the ones tests/test_ragged_cpu.py holds on the host instantiation: go() through the C ABI against oracle/_ref/hisat2-align-s on every record; the cases whose
option is the sink's or whose records leave through the long-edit area (--no-mixed --no-discordant, --bowtie2-dp 2 --score-min L,0,-3, spliced) through the command
line, every SAM line, stderr and header; the committed golden (no reference binary); the fast pass on against off on ragged batches; and batches whose longest read
changes on one stream (the SwAligner pool is sized by the first and grown by the second)."""
import functools
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fast_digest as FD
import ragged_cases as RC
import sam_lines as SL
import test_ragged_cpu as TC
from hisat2_amd import api
from test_sam_lines import diff_lines

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
CLI = os.path.join(ROOT, "hisat2_amd", "hisat2-align-amd")
needs_ref = TC.needs_ref


@pytest.fixture(scope="module")
def live_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("ragged_gpu"))


# ---------------------------------------------------------------- go() through the C ABI against the live reference, every record
READ_CASES = [c for c in TC.READ_CASES if not c.get("bowtie2_dp")]
READ_IDS = [i for i, c in zip(TC.READ_IDS, TC.READ_CASES) if not c.get("bowtie2_dp")]


@needs_ref
@pytest.mark.parametrize("case", READ_CASES, ids=READ_IDS)
def test_live_reference_ragged_reads(live_dir, case):
    """4000 reads of 0 to 300 bases in one batch"""
    from test_gpu_frag import _backend
    bad, info, reads, labels = TC.run_reads(live_dir, case, backend=_backend)
    TC.check_reads(bad, info, reads, labels, RC.READ_MINIMA["snps" if case.get("snps") else "plain"])


@needs_ref
@pytest.mark.parametrize("case", TC.PAIR_CASES, ids=["plain", "snp-graph"])
def test_live_reference_ragged_pairs(live_dir, case):
    """4000 pairs R1-R6; the stream is sized by the larger mate set (the second mates are the longer set in about half of the pairs)"""
    from test_gpu_frag import _pair_backend
    bad, info, lc = TC.run_pairs(live_dir, case, backend=_pair_backend, npairs=4000, stride=api.PAIR_RES_CAP)
    TC.check_pairs(bad, info, lc, RC.PAIR_MINIMA["snps" if case.get("snps") else "plain"])


# ---------------------------------------------------------------- the command line against the reference's: body, stderr, header
def cli_vs_ref(tmp, base, common, cli=("-p", "4", "--batch", "700")):
    """hisat2-align-amd against hisat2-align-s -p 1 on the same arguments -> (the reference's body lines, its stderr)"""
    ref_sam, amd_sam, ref_err, amd_err = (os.path.join(str(tmp), x) for x in ("ref.sam", "amd.sam", "ref.err", "amd.err"))
    common = ["-x", base] + list(common)
    subprocess.run([os.path.join(REF, "hisat2-align-s"), "-p", "1", "-S", ref_sam] + common, check=True, stdout=subprocess.DEVNULL, stderr=open(ref_err, "w"))
    subprocess.run([CLI] + list(cli) + ["-S", amd_sam] + common, check=True, stderr=open(amd_err, "w"), timeout=300)
    want = SL.body_lines(ref_sam)
    assert diff_lines(SL.body_lines(amd_sam), want) == 0
    assert open(amd_err).read() == open(ref_err).read()
    hdr, ref_hdr = ([l for l in open(f) if l.startswith("@")] for f in (amd_sam, ref_sam))
    assert hdr[:-1] == ref_hdr[:-1] and len(hdr) == len(ref_hdr)         # (the last line is @PG: the program's own)
    return want, open(ref_err).read()


def warnings_of(err):
    return [l for l in err.splitlines(keepends=True) if l.startswith("Warning: skipping ")]


@needs_ref
def test_command_line_bowtie2_dp_cell_widths_and_row_cap(live_dir, tmp_path):
    """--bowtie2-dp 2 --score-min L,0,-3 on classes Z, T, W, L: 8-bit and 16-bit cells (the minimum score passes -254 from 85 bases on) and the 255 / 256-row
    edge in one batch.  A read of 256 bases may take 128 mismatches: the records beyond 32 edits leave through the long-edit area, so the case runs here."""
    lc = RC.live_case(REF, live_dir, classes="ZTWL")
    rfa = str(tmp_path / "r.fa")
    RC.write_reads(rfa, lc["reads"])
    want, err = cli_vs_ref(tmp_path, lc["base"], ["-f", "--no-spliced-alignment", "--bowtie2-dp", "2", "--score-min", "L,0,-3", "-U", rfa])
    assert len(warnings_of(err)) == 2 * RC.n_length_filtered(lc["reads"]) > 0
    want = {l.split("\t")[0]: [(int(l.split("\t")[1]),)] for l in reversed(want)}
    RC.assert_teeth(RC.read_teeth(want, lc["labels"]), RC.READ_MINIMA["dp"])


@needs_ref
def test_command_line_ragged_reads_spliced(tmp_path):
    """--no-temp-splicesite: anchors of every length either side of an intron"""
    from hisat2_amd import synth
    contigs, reads = TC.spliced_case()
    fa = str(tmp_path / "g.fa")
    synth.write_fasta(fa, contigs, names=["chr1"])
    base = str(tmp_path / "g")
    subprocess.run([os.path.join(REF, "hisat2-build-s"), "-q", fa, base], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    rfa = str(tmp_path / "r.fa")
    RC.write_reads(rfa, reads)
    want, err = cli_vs_ref(tmp_path, base, ["-f", "--no-temp-splicesite", "-U", rfa])
    assert len(warnings_of(err)) == 2 * RC.n_length_filtered(reads) > 0
    assert sum(1 for l in want if l.split("\t")[1] in ("0", "16") and "N" in l.split("\t")[5]) >= RC.SPLICED_MINIMUM


def write_live_fastq(lc, tmp, npairs, nreads):
    """the live case's pairs and reads as FASTQ files with seeded qualities -> (arguments, number of length-filtered reads and mates)"""
    m1, m2, reads = lc["m1"][:npairs], lc["m2"][:npairs], lc["reads"][:nreads]
    f1, f2, fu = (os.path.join(str(tmp), x) for x in ("r1.fq", "r2.fq", "u.fq"))
    RC.write_reads(f1, m1, RC.seeded_quals(m1, RC.LIVE_SEED + 51), [f"p{i}" for i in range(npairs)])
    RC.write_reads(f2, m2, RC.seeded_quals(m2, RC.LIVE_SEED + 52), [f"p{i}" for i in range(npairs)])
    RC.write_reads(fu, reads, RC.seeded_quals(reads, RC.LIVE_SEED + 53), [f"r{i}" for i in range(nreads)])
    return ["-1", f1, "-2", f2, "-U", fu], (m1, m2, reads)


@needs_ref
@pytest.mark.parametrize("extra", [(), ("-5", "3", "-3", "40"), ("--no-mixed", "--no-discordant")], ids=["plain", "trim5-3-trim3-40", "no-mixed-no-discordant"])
def test_command_line_ragged_pairs_and_reads(live_dir, tmp_path, extra):
    """file -> SAM: 2500 ragged FASTQ pairs (R1-R6) plus 2500 -U reads with records of 0 and 1 bases, -p 4 --batch 700: the SAM body, stderr (the length-filter
    warnings in record order, once each across batches and threads, then the summary) and the header, byte for byte.  -5 3 -3 40 cuts every record of up to 44
    bases down to under 2: the warnings then show the trimmed length."""
    lc = RC.live_case(REF, live_dir)
    files, (m1, m2, reads) = write_live_fastq(lc, tmp_path, 2500, 2500)
    want, err = cli_vs_ref(tmp_path, lc["base"], ["-q", "--no-spliced-alignment"] + files + list(extra))
    cut = 43 if "-5" in extra else 0                     # a record of n bases keeps max(0, n - 43) of them
    nshort = sum(1 for rs in (m1, m2, reads) for r in rs if len(r) - cut < 2)
    assert len(warnings_of(err)) == 2 * nshort and nshort >= 300
    assert sum(1 for l in want if l.endswith("YF:Z:LN")) == nshort
    assert sum(1 for l in want if l.split("\t")[9:11] == ["*", "*"]) == sum(1 for rs in (m1, m2, reads) for r in rs if len(r) - cut <= 0) > 0
    # measured from the reference: 1373 length-filtered reads and mates (683 without bases) and 2928 lines of concordant pairs; with -5 3 -3 40: 3007 (all of
    # them without bases) and 1560.  Half of the concordant lines is asserted.
    assert sum(1 for l in want if int(l.split("\t")[1]) & 2) >= (780 if cut else 1464)


# ---------------------------------------------------------------- the committed golden: no reference binary
def test_golden_ragged(g1_index, golden_dir, tmp_path):
    """tests/golden/ragged_*: 2000 ragged reads and 1500 ragged pairs (FASTQ) on the committed index g1 through the command line: the reference's SAM body and
    its stderr, byte for byte"""
    TC.check_golden_inputs(TC.golden_ragged(golden_dir))
    for tag, inputs in (("se", ("-U", "ragged_se.fq")), ("pe", ("-1", "ragged_pe_1.fq", "-2", "ragged_pe_2.fq"))):
        args = []
        for a in inputs:
            if a.endswith(".fq"):
                with open(tmp_path / a, "wb") as f:
                    f.write(gzip.open(os.path.join(golden_dir, a + ".gz")).read())
                a = str(tmp_path / a)
            args.append(a)
        sam, err = str(tmp_path / (tag + ".sam")), str(tmp_path / (tag + ".err"))
        subprocess.run([CLI, "-q", "-p", "3", "--batch", "600", "--no-spliced-alignment", "-x", g1_index, "-S", sam] + args, check=True, stderr=open(err, "w"), timeout=300)
        want = TC.golden_text(golden_dir, f"ragged_{tag}.sam.gz").splitlines()
        assert sum(1 for l in want if not int(l.split("\t")[1]) & 256) == (RC.GOLDEN_NREADS if tag == "se" else 2 * RC.GOLDEN_NPAIRS)
        assert diff_lines(SL.body_lines(sam), want) == 0
        assert open(err).read() == TC.golden_text(golden_dir, f"ragged_{tag}.err.gz")


# ---------------------------------------------------------------- the fast pass on against off
FAST_N = 20000
_DIGESTS = {}


def digest(base, npz, fast, env=()):
    """fast_digest.py in a process of its own (H2G_GO_FAST is read once); the run with the pass off is made once per index"""
    key = (base, fast, tuple(env))
    if key not in _DIGESTS:
        e = dict(os.environ, H2G_GO_FAST=fast, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"), **dict(env))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fast_digest.py"), base, npz], env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        _DIGESTS[key] = json.loads(r.stdout.strip().splitlines()[-1])
    return _DIGESTS[key]


@needs_ref
@pytest.mark.parametrize("snps,env", [
    (False, ()),
    (True, ()),                                                                   # h2g_k_go_fast_graph.hip
    (False, (("H2G_FAST_AM", "1"),)),                                             # alignMate in the pass
    (False, (("H2G_FAST_ORPHAN", "64"), ("H2G_DRAIN_GRID", "8"))),                # the end of the batch through the drain launch
    (False, (("H2G_FAST_MATE_HANDOVER", "1"),)),                                  # the pairs that need alignMate parked for it
], ids=["plain", "snp-graph", "fast-am", "drain", "mate-handover"])
def test_fast_pass_equals_the_machine_on_ragged_batches(live_dir, snps, env):
    """20 000 ragged pairs (R1-R6) and 20 000 ragged reads, runs queued back to back: a lane that finishes a read takes one of another length; a pair with a mate
    outside 32..128 bases (or with an N) is handed on whole; the packed form ends in a partial word at every length that is no multiple of 16.  The same bytes
    with the pass on and off, and the pass is the path of at least half of the units that can enter it."""
    lc = RC.live_case(REF, live_dir, snps=snps, nreads=FAST_N, npairs=FAST_N)
    npz = os.path.join(live_dir, "ragged_g.npz" if snps else "ragged.npz")
    if not os.path.exists(npz):
        FD.save_ragged(npz, lc["m1"], lc["m2"], lc["reads"])
    off, on = digest(lc["base"], npz, "0"), digest(lc["base"], npz, "1", env)
    print(off, on)
    nin = {"pairs": int(RC.fast_ineligible(lc["m1"], lc["m2"]).sum()), "reads": int(RC.fast_ineligible(lc["reads"]).sum())}
    for k in ("pairs", "reads"):
        assert 0 < nin[k] < FAST_N
        assert off[k]["fast"] == 0
        assert on[k]["fast"] + on[k]["handed_on"] == FAST_N
        assert on[k]["handed_on"] >= nin[k], (on[k], nin[k])
        assert on[k]["fast"] >= 0.5 * (FAST_N - nin[k]), (on[k], nin[k])
        assert off[k]["overflow"] == 0 and on[k]["overflow"] == 0
        assert off[k]["aligned"] == on[k]["aligned"] > 0
        assert off[k]["sha"] == on[k]["sha"], k


# ---------------------------------------------------------------- batches whose longest read changes, on one stream
def _dense(st):
    res, aln, offs = st.align_fetch_dense()
    return res.tobytes() + offs.tobytes() + FD.aln_bytes(aln, int(offs[st.n_reads]))


def _load(st, reads, names):
    lst = [np.ascontiguousarray(r, dtype=np.uint8) for r in reads]
    st.set_reads(np.concatenate(lst), np.concatenate([[0], np.cumsum([len(r) for r in lst])]).astype(np.uint32))
    st.set_read_names(names)


def test_batches_of_changing_read_length_on_one_stream(g1_index, golden_dir):
    """--bowtie2-dp 2, three resident batches queued back to back without a sync: the longest read is 64 bases in batch A, 250 in B, 64 again in C.  The SwAligner
    pool is sized by the longest read of the batch that runs first and allocated again for the second.  Every batch's bytes equal those of a stream that only
    ever held that batch.  (The golden reads on g1: no reference binary.)"""
    g = TC.golden_ragged(golden_dir)
    short = [(n, r) for n, r in zip(g["rnames"], g["reads"]) if len(r) <= 64]
    mid = [(n, r) for n, r in zip(g["rnames"], g["reads"]) if 64 < len(r) <= 200]
    long_ = [(n, r[:250]) for n, r in zip(g["rnames"], g["reads"]) if len(r) in (255, 256)]
    sets = [short[:300], mid[:200] + long_[:100] + short[600:650], short[300:600]]
    assert [max(len(r) for _, r in s) for s in sets] == [64, 250, 64] and [len(s) for s in sets] == [300, 350, 300]
    assert all(any(len(r) < 2 for _, r in s) for s in sets)
    ix = api.Index(g1_index, device=0)
    cap = max(sum(len(r) for _, r in s) for s in sets) + 64

    def params(st):
        p = st.align_params()
        p.no_spliced_alignment = 1
        p.bowtie2_dp = 2
        return p
    want = []
    for s in sets:
        st = api.Stream(ix, max_reads=len(s), max_bases=cap)
        _load(st, [r for _, r in s], [n for n, _ in s])
        st.align_run(params(st))
        want.append(_dense(st))
        assert int(st.counters().n_aligned) >= len(s) // 3
        st.close()
    assert want[0] != want[2]
    st = api.Stream(ix, max_reads=max(len(s) for s in sets), max_bases=cap)
    for k, s in enumerate(sets):
        st.select_batch(k)
        _load(st, [r for _, r in s], [n for n, _ in s])
    p = params(st)
    for k in range(len(sets)):
        st.select_batch(k)
        st.align_run(p)
    st.sync()
    for k in (2, 0, 1):
        st.select_batch(k)
        assert _dense(st) == want[k], "batch %d" % k
    st.close()
    ix.close()
