"""Trimmed read sets on the host (tests/ragged_cases.py): every read length from 0 to 300 in one batch, mates of different lengths, empty reads — the go() state
machine (tests/emul) against oracle/_ref/hisat2-align-s on every record, the fast path against the machine, the C++ sink's text against the reference's, and the
committed golden (tests/golden/ragged_*), which needs no reference binary."""
import gzip
import os

import numpy as np
import pytest

import ragged_cases as RC
import sam_lines as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
needs_ref = pytest.mark.skipif(not os.path.exists(os.path.join(REF, "hisat2-align-s")), reason="needs oracle/_ref")


@pytest.fixture(scope="module")
def live_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("ragged"))


READ_CASES = [
    dict(),
    dict(fastq=True, extra=("--mp", "4,2")),
    dict(snps=True),
    # both the 8 / 16-bit cell switch of the SwAligner pass (--score-min below -254 from 85 bases on) and its 255 / 256-row edge in one batch; class X stays out:
    # beyond 256 rows a read is flagged by design
    dict(extra=("--bowtie2-dp", "2", "--score-min", "L,0,-3"), bowtie2_dp=2, classes="ZTWL"),
    dict(extra=("-k", "10")),
    dict(extra=("--no-softclip",)),
]
READ_IDS = ["plain", "fastq-mp", "snp-graph", "bowtie2-dp2", "k10", "no-softclip"]


def run_reads(live_dir, case, backend=None, nreads=4000):
    """one unpaired case through fuzz_align.run_case -> (bad, info, reads, labels)"""
    import fuzz_align as F
    case = dict(case)
    lc = RC.live_case(REF, live_dir, snps=case.pop("snps", False), nreads=nreads, classes=case.pop("classes", RC.READ_CLASSES))
    info = {}
    kw = dict(backend=backend) if backend else {}
    bad, _ = F.run_case(RC.LIVE_SEED, genome=RC.genome_arg(lc["contigs"]), reads=lc["reads"], variants=lc["variants"], info=info, verbose=5, **kw, **case)
    return bad, info, lc["reads"], lc["labels"]


def second_pass_on_the_host(info, reads, opts, bowtie2_dp):
    """What the device does with a read its default workspace flags (n_second_pass): the read runs again with the large workspace (160 edits per working hit,
    records beyond 32 edits through the long-edit area).  Here: the flagged reads through the host instantiation of that configuration (tests/emul/libh2gemu_long.so)
    and the sink, every line against the reference's -> the number of reads still flagged after it."""
    from test_long_edits_cpu import _align_long
    ids = info["flagged"]
    want = {}
    for l in SL.body_lines(os.path.join(info["tmp"], "ref.sam")):
        want.setdefault(l.split("\t")[0], []).append(l)
    # Only a read whose minimum score admits 33 edits can need the large workspace.  The cheapest 33 edits are k Ns (1 each, k <= 0.15 L by --n-ceil) and one gap
    # of 33 - k positions (5 + 3 each): 104 - 2 k <= 3 L gives L >= 32.  A default workspace that starts to flag shorter reads is not absorbed by the second pass.
    print("flagged reads and their lengths:", {i: len(reads[i]) for i in ids})
    assert all(len(reads[i]) >= 32 for i in ids)
    got, nlong, still = _align_long(info["base"], [reads[i] for i in ids], list(opts), bowtie2_dp=bowtie2_dp, names=[str(i) for i in ids])
    assert got == sum((want[str(i)] for i in ids), []), "the second pass differs from the reference"
    print(f"second pass: {len(ids)} reads flagged by the default workspace, {nlong} records beyond 32 edits, {still} still flagged")
    return still


def check_reads(bad, info, reads, labels, minima, overflow=None):
    assert bad == 0 and (info["overflow"] if overflow is None else overflow) == 0
    assert RC.ln_lines(os.path.join(info["tmp"], "ref.sam")) == RC.n_length_filtered(reads) > 0
    RC.assert_teeth(RC.read_teeth(info["want"], labels), minima)


@needs_ref
@pytest.mark.parametrize("case", READ_CASES, ids=READ_IDS)
def test_live_reference_ragged_reads(live_dir, case):
    """4000 reads of 0 to 300 bases in one batch (class X left out of the SwAligner case), every record against the reference's"""
    bad, info, reads, labels = run_reads(live_dir, case)
    overflow = None
    if case.get("bowtie2_dp"):
        # --score-min L,0,-3 lets a read of 256 bases take 128 mismatches: for a dozen of the 4000 reads (81 to 256 bases) a candidate of the search holds more
        # than the 32 edits of the default workspace's records, and the read is flagged by design (bit 1; bit 256: the same in the SwAligner's result) although
        # no line the reference prints for it is that long.  Their overflow is what is left after the second pass.
        overflow = second_pass_on_the_host(info, reads, case["extra"], case["bowtie2_dp"])
    check_reads(bad, info, reads, labels, RC.READ_MINIMA["snps" if case.get("snps") else "dp" if case.get("bowtie2_dp") else "plain"], overflow)


def spliced_case(n=3000):
    """reads of 150 bases over planted introns (fuzz_spliced.make_case), each cut to a drawn length -> (contigs, reads)"""
    import fuzz_spliced as FS
    contigs, reads, _ = FS.make_case(RC.LIVE_SEED + 30, n, rdlen=150, sub=0.005)
    lens = [1, 2, 3, 5, 8, 10, 11, 15, 16, 17, 18, 19, 20, 24, 31, 32, 33, 47, 48, 49, 63, 64, 65, 96, 97, 127, 128, 129, 150]
    return contigs, RC.trim_reads(list(reads), RC.LIVE_SEED + 31, lens)[0]


@needs_ref
def test_live_reference_ragged_reads_spliced():
    """--no-temp-splicesite: anchors of every length either side of an intron, down to reads shorter than the minimum anchor"""
    import fuzz_align as F
    contigs, reads = spliced_case()
    info = {}
    bad, _ = F.run_case(RC.LIVE_SEED, genome=(contigs, ["chr1"]), reads=reads, info=info, verbose=5, spliced=True)
    assert bad == 0 and info["overflow"] == 0
    nspl = sum(1 for q in info["want"] if any("N" in r[3] for r in info["want"][q]))
    print("spliced in the reference:", nspl)
    assert nspl >= RC.SPLICED_MINIMUM


PAIR_CASES = [dict(), dict(snps=True)]


def run_pairs(live_dir, case, backend=None, npairs=3000, stride=16):
    import fuzz_pairs as F
    lc = RC.live_case(REF, live_dir, snps=case.get("snps", False), npairs=npairs)
    info = {}
    kw = dict(backend=backend, stride=stride) if backend else {}
    bad, _ = F.run_case(RC.LIVE_SEED, genome=RC.genome_arg(lc["contigs"]), pairs=(lc["m1"], lc["m2"]), variants=lc["variants"], info=info, verbose=5, **kw)
    return bad, info, lc


def check_pairs(bad, info, lc, minima):
    assert bad == 0 and info["overflow"] == 0
    assert RC.ln_lines(os.path.join(info["tmp"], "ref.sam")) == RC.n_length_filtered(lc["m1"], lc["m2"]) > 0
    RC.assert_teeth(RC.pair_teeth(info["want"], lc["plabels"]), minima)


@needs_ref
@pytest.mark.parametrize("case", PAIR_CASES, ids=["plain", "snp-graph"])
def test_live_reference_ragged_pairs(live_dir, case):
    """3000 pairs R1-R6: mates of different lengths, one mate outside the fast pass's range, one or both mates filtered by length"""
    bad, info, lc = run_pairs(live_dir, case)
    check_pairs(bad, info, lc, RC.PAIR_MINIMA["snps" if case.get("snps") else "plain"])


def ref_run(tmp, base, files, extra=()):
    """hisat2-align-s -p 1 -> (body lines, header lines, stderr text)"""
    import subprocess
    sam, err = os.path.join(tmp, "ref.sam"), os.path.join(tmp, "ref.err")
    subprocess.run([os.path.join(REF, "hisat2-align-s"), "-p", "1", "-x", base, "-S", sam] + list(files) + list(extra), check=True, stdout=subprocess.DEVNULL, stderr=open(err, "w"))
    return SL.body_lines(sam), [l for l in open(sam) if l.startswith("@")], open(err).read()


def expected_warnings(names1, reads1, names2=None, reads2=None):
    """the reference's stderr ahead of its summary (ragged_cases.length_warnings), from the inputs"""
    units = [[(names1[i], len(reads1[i]))] + ([(names2[i], len(reads2[i]))] if reads2 is not None else []) for i in range(len(reads1))]
    return "".join(l + "\n" for l in RC.length_warnings(units))


def split_stderr(text):
    """(the warnings, the summary)"""
    lines = text.splitlines(keepends=True)
    k = next(i for i, l in enumerate(lines) if not l.startswith("Warning: skipping "))
    assert not any(l.startswith("Warning") for l in lines[k:])
    return "".join(lines[:k]), "".join(lines[k:])


@needs_ref
@pytest.mark.parametrize("omit", [False, True], ids=["plain", "omit-sec-seq"])
def test_unpaired_lines_identical_fastq_with_empty_reads(live_dir, tmp_path, omit):
    """every SAM line and the summary of 3000 ragged FASTQ reads, empty reads in the middle of the file: SEQ and QUAL of a read without bases are '*'
    (aln_sink.h:3194, :3209), with and without --omit-sec-seq (-k 10: secondary lines).  The reference's stderr is the warnings expected_warnings() computes, then
    the summary."""
    from h2gemu_align import emu_align
    from test_sam_lines import diff_lines
    lc = RC.live_case(REF, live_dir)
    reads = lc["reads"][:3000]
    names = [f"r{i}" for i in range(len(reads))]
    quals = RC.seeded_quals(reads, RC.LIVE_SEED + 40)
    fq = str(tmp_path / "r.fq")
    RC.write_reads(fq, reads, quals, names)
    opts = ("-k", "10", "--omit-sec-seq") if omit else ()
    want, _, err = ref_run(str(tmp_path), lc["base"], ["-q", "--no-spliced-alignment", "-U", fq], opts)
    outs, recs = emu_align(lc["base"], reads, names, quals=quals, options=opts)
    res, aln = SL.emu_to_abi(outs, recs)
    got = SL.format_unpaired(SL.load_sam_lib(), lc["base"], reads, names, res, aln, quals=quals, options=opts)
    nempty = sum(1 for r in reads if len(r) == 0)
    assert nempty >= 40 and sum(1 for l in want if l.split("\t")[9:11] == ["*", "*"] and l.endswith("YF:Z:LN")) == nempty
    assert diff_lines(got, want) == 0
    warn, summary = split_stderr(err)
    assert warn == expected_warnings(names, reads) and SL.LAST_SUMMARY == summary


@needs_ref
@pytest.mark.parametrize("opts", [(), ("--no-mixed", "--no-discordant")], ids=["plain", "no-mixed-no-discordant"])
def test_paired_lines_identical_fastq_with_empty_mates(live_dir, tmp_path, monkeypatch, opts):
    """every SAM line and the summary of 3000 ragged FASTQ pairs (R1-R6); --no-mixed --no-discordant is the sink's (ReportingParams), so it is checked here, on
    lines, and not on records"""
    import fuzz_pairs as F
    from test_sam_lines import diff_lines, paired_lines
    monkeypatch.setattr(F, "OPTS", opts)
    lc = RC.live_case(REF, live_dir)
    m1, m2 = lc["m1"], lc["m2"]
    names = [f"p{i}" for i in range(len(m1))]
    q1, q2 = RC.seeded_quals(m1, RC.LIVE_SEED + 41), RC.seeded_quals(m2, RC.LIVE_SEED + 42)
    f1, f2 = str(tmp_path / "r1.fq"), str(tmp_path / "r2.fq")
    RC.write_reads(f1, m1, q1, names)
    RC.write_reads(f2, m2, q2, names)
    want, _, err = ref_run(str(tmp_path), lc["base"], ["-q", "--no-spliced-alignment", "-1", f1, "-2", f2], opts)
    got = paired_lines(lc["base"], m1, m2, names, names, opts, quals=(q1, q2))
    nempty = sum(1 for r in m1 + m2 if len(r) == 0)
    assert nempty >= 100 and sum(1 for l in want if l.split("\t")[9:11] == ["*", "*"]) == nempty
    assert diff_lines(got, want) == 0
    warn, summary = split_stderr(err)
    assert warn == expected_warnings(names, m1, names, m2) and SL.LAST_SUMMARY == summary


# ---------------------------------------------------------------- the fast path against the machine
def check_fast(r, ineligible):
    nin = int(ineligible.sum())
    assert r["mismatching"] == 0, r
    assert r["bails"].get("input", 0) == nin, (r["bails"], nin)
    assert r["completed"] >= 0.5 * (r["n"] - nin), (r, nin)        # the floor of test_fast_path_cpu, on the units that can enter
    assert not r["done"][ineligible].any()


@needs_ref
@pytest.mark.parametrize("variant", ["", "am", "g"])
def test_fast_path_equals_the_machine_on_ragged_batches(live_dir, variant):
    """fast_check: a read keeps its lane's state while the next read of the lane has another length; a pair with one mate inside 32..128 and one outside is
    handed on whole (FB_INPUT counts exactly the units that cannot enter: a mate outside the range or with an N); the packed form's partial last word at
    every length mod 16.  "am": alignMate in the fast path; "g": the graph configuration on the SNP-graph index."""
    import fast_check as FC
    lc = RC.live_case(REF, live_dir, snps=variant == "g")
    r = FC.fast_check(lc["base"], lc["reads"], variant=variant)
    print("reads:", {k: v for k, v in r.items() if k != "done"})
    check_fast(r, RC.fast_ineligible(lc["reads"]))
    r = FC.fast_check(lc["base"], lc["m1"], lc["m2"], variant=variant)
    print("pairs:", {k: v for k, v in r.items() if k != "done"})
    bad = RC.fast_ineligible(lc["m1"], lc["m2"])
    check_fast(r, bad)
    lab = np.array(lc["plabels"])
    assert bad[np.isin(lab, ["R2", "R3", "R4", "R5"])].all() and r["done"][lab == "R1"].sum() >= 0.5 * (~bad[lab == "R1"]).sum()


# ---------------------------------------------------------------- the committed golden: no reference binary needed
def golden_ragged(golden_dir):
    """-> dict(reads, rnames, rquals, m1, m2, pnames, q1, q2) of tests/golden/ragged_*.fq.gz"""
    def fq(fn):
        lines = gzip.open(os.path.join(golden_dir, fn), "rt").read().split("\n")
        code = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
        names = [l[1:] for l in lines[0:-1:4]]
        reads = [np.array([code[c] for c in l], dtype=np.uint8) for l in lines[1::4]]
        quals = np.frombuffer("".join(lines[3::4]).encode(), dtype=np.uint8)
        return names, reads, quals
    rn, rd, rq = fq("ragged_se.fq.gz")
    n1, m1, q1 = fq("ragged_pe_1.fq.gz")
    _, m2, q2 = fq("ragged_pe_2.fq.gz")
    return dict(reads=rd, rnames=rn, rquals=rq, m1=m1, m2=m2, pnames=n1, q1=q1, q2=q2)


def golden_text(golden_dir, fn):
    return gzip.open(os.path.join(golden_dir, fn), "rt").read()


def check_golden_inputs(g):
    assert len(g["reads"]) == RC.GOLDEN_NREADS and len(g["m1"]) == len(g["m2"]) == RC.GOLDEN_NPAIRS
    lens = {len(r) for r in g["reads"]}
    assert {0, 1, 2, 8, 31, 32, 128, 129, 256, 257, 300} <= lens
    assert any(len(a) != len(b) for a, b in zip(g["m1"], g["m2"])) and any(len(a) == 0 for a in g["m1"]) and any(len(b) == 0 for b in g["m2"])


def test_golden_ragged(g1_index, golden_dir, monkeypatch):
    """2000 ragged reads and 1500 ragged pairs (FASTQ) on the committed index g1: the host instantiation plus the sink write the reference's SAM body, and the
    reference's stderr is the length-filter warnings followed by the sink's summary"""
    import fuzz_pairs as F
    from h2gemu_align import emu_align
    from test_sam_lines import diff_lines, paired_lines
    monkeypatch.setattr(F, "OPTS", ())
    g = golden_ragged(golden_dir)
    check_golden_inputs(g)
    outs, recs = emu_align(g1_index, g["reads"], g["rnames"], quals=g["rquals"])
    assert not any(o.overflow for o in outs)
    res, aln = SL.emu_to_abi(outs, recs)
    got = SL.format_unpaired(SL.load_sam_lib(), g1_index, g["reads"], g["rnames"], res, aln, quals=g["rquals"])
    want = golden_text(golden_dir, "ragged_se.sam.gz").splitlines()
    assert diff_lines(got, want) == 0
    warn, summary = split_stderr(golden_text(golden_dir, "ragged_se.err.gz"))
    assert warn == expected_warnings(g["rnames"], g["reads"]) and SL.LAST_SUMMARY == summary
    assert sum(1 for l in want if l.endswith("YF:Z:LN")) == RC.n_length_filtered(g["reads"])
    assert sum(1 for l in want if l.split("\t")[1] != "4") >= RC.GOLDEN_MINIMA["aligned_reads"]
    got = paired_lines(g1_index, g["m1"], g["m2"], g["pnames"], g["pnames"], quals=(g["q1"], g["q2"]))
    want = golden_text(golden_dir, "ragged_pe.sam.gz").splitlines()
    assert diff_lines(got, want) == 0
    warn, summary = split_stderr(golden_text(golden_dir, "ragged_pe.err.gz"))
    assert warn == expected_warnings(g["pnames"], g["m1"], g["pnames"], g["m2"]) and SL.LAST_SUMMARY == summary
    assert sum(1 for l in want if l.endswith("YF:Z:LN")) == RC.n_length_filtered(g["m1"], g["m2"])
    assert sum(1 for l in want if int(l.split("\t")[1]) & 2) // 2 >= RC.GOLDEN_MINIMA["concordant_pairs"]
