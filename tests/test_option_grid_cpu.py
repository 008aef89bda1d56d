"""The option grid (tests/option_cases.py) on the host, no GPU: go() under the scoring options' edges — the 16-bit score range of the fast pass, every --score-min
function, mismatch / N / gap penalties from 1 to 40 with qualities over 2 .. 40, soft clipping, -X, -k / --max-seeds.

1. the general machine (hisat2_amd/csrc/h2g_machine.h, host instantiation: the default configuration, what it flags once more through the large-workspace one, as
   go_run's two passes do) against the live reference binary, every case, reads and pairs, a linear index and — one case
   of each group — a SNP graph: every SAM line (FLAG, RNAME, POS, CIGAR, AS:i, in order) and the counts of the stderr summary.  The fast pass against the machine proves
   nothing unless the machine is pinned under the same options.
2. the fast pass (h2g_fast.h) against the machine through fast_check, every case, in the shipped configuration, with alignMate in the pass ("am") and over the graph
   ("g"): nothing it completes may differ; a `bails_whole` case hands every unit on for the named reason, a `takes` case completes at least the table's floor.

Mutants these tests were shown to catch, one at a time on a scratch copy (the failing test in brackets):
  `-30000` in FPC_GO_INIT changed to `-40000`                              [test_fast_pass_equals_the_machine: c30001, c31000 no longer hand on whole]
  mm_penalty(sc, q) replaced by sc.mmpMax in the fast path's scoring       [test_fast_pass_equals_the_machine: mp40-0-fastq and the other FASTQ cases mismatch]
  the `> 0 ? 0` clamp removed from min_score_for                           [test_machine_equals_the_reference: c40000-clamped differs from the reference]
  max_frag_len ignored in the fast path's pairing                          [test_fast_pass_equals_the_machine: x120 mismatches]
"""
import os
import re
import subprocess
import tempfile

import pytest

import option_cases as OC
import sam_util as SU
from hisat2_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(REF, "hisat2-align-s")), reason="needs oracle/_ref")
REF_TIMEOUT = 300          # seconds a reference run may take before the case counts as one the reference hangs on
IDS = [c.name for c in OC.CASES]


def _build(contigs, variants=None):
    tmp = tempfile.mkdtemp(prefix="h2optg")
    fa, base = os.path.join(tmp, "g.fa"), os.path.join(tmp, "g")
    synth.write_fasta(fa, contigs)
    snp = []
    if variants:
        synth.write_snps(os.path.join(tmp, "g.snp"), variants)
        snp = ["--snp", os.path.join(tmp, "g.snp")]
    subprocess.run([os.path.join(REF, "hisat2-build-s"), "-q"] + snp + [fa, base], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return base


@pytest.fixture(scope="module")
def linear():
    """(index base, contigs the reads are drawn from, records of the FASTA file, variants)"""
    contigs = OC.make_genome(OC.HOST_GENOME)
    return _build(contigs), contigs, contigs, None


@pytest.fixture(scope="module")
def graph():
    contigs, var, alt = OC.make_graph(OC.HOST_GRAPH)
    return _build(contigs, var), alt, contigs, var


def test_the_table_holds_what_it_must():
    """every group, the guard's exact edge on both sides, FASTQ cases, one ragged set, a graph case per group, and no penalty below 1 (those are refused, never run)"""
    assert {c.group for c in OC.CASES} == set(OC.GROUPS) and {OC.BY_NAME[n].group for n in OC.GRAPH_CASES} == set(OC.GROUPS)
    assert OC.BY_NAME["c30000"].expect == "takes" and OC.BY_NAME["c30001"].expect == "bails_whole" and OC.BY_NAME["c31000"].reason == "input"
    assert sum(c.fastq for c in OC.CASES) >= 4 and sum(c.ragged for c in OC.CASES) == 1
    assert OC.BY_NAME[OC.DEVICE_EXTRA_CASES[0]].fastq and OC.BY_NAME[OC.DEVICE_EXTRA_CASES[1]].group == "score16" and OC.BY_NAME[OC.DEVICE_EXTRA_CASES[2]].longdel
    for c in OC.CASES:
        for o, v in zip(c.opts, c.opts[1:]):
            if o in ("--mp", "--sp", "--np", "--rdg", "--rfg"):
                nums = [int(x) for x in v.split(",")]
                assert (nums[0] >= 1 and nums[-1] >= 1) or (o == "--mp" and nums == [nums[0], 0] and nums[0] >= 1), c      # (--mp MX,0: the minimum is no divisor)
        assert c.expect in ("takes", "bails_whole") and (c.reason is not None) == (c.expect == "bails_whole")
        for f, m in zip(c.floors, c.measured):
            assert abs(f - OC.floor_of(m, OC.N_HOST)) < 1e-9, c             # the floor is half of what was measured, never set by hand


def _summary_numbers(err):
    """the counts of the reference's stderr summary, line by line: [(count, what), ...]"""
    return [(int(m.group(1)), m.group(2)) for m in re.finditer(r"^\s*(\d+) (?:\([^)]*\) )?(.*)$", err, re.M)]


def _read_summary(recs, n):
    """the unpaired summary's counts from SAM records (aln_sink.h printUnpairedSummary): reads; unpaired; aligned 0 / exactly 1 / > 1 times"""
    k = [sum(1 for f in v if not f[0] & 4) for v in recs.values()]
    return [n, n, sum(1 for x in k if x == 0), sum(1 for x in k if x == 1), sum(1 for x in k if x > 1)]


def _pair_summary(recs, n):
    """the leading counts of the paired summary: reads; paired; concordantly 0 / exactly 1 / > 1 times (lines of mate 1 with the proper-pair bit)"""
    k = [sum(1 for f in v if f[0] & 0x40 and f[0] & 2) for v in recs.values()]
    return [n, n, sum(1 for x in k if x == 0), sum(1 for x in k if x == 1), sum(1 for x in k if x > 1)]


def _against_the_reference(c, idx, kind):
    import fuzz_align as FA
    import fuzz_pairs as FP
    base, src, records, variants = idx
    s = OC.read_set(c, src, OC.N_HOST, OC.HOST_GENOME["seed"])
    info = {}
    genome = (records, None)
    if kind == "reads":
        bad, _ = FA.run_case(7, genome=genome, reads=s["reads"], variants=variants, quals=s["qr"], extra=c.opts, verbose=3, info=info, ref_timeout=REF_TIMEOUT, base=base,
                             backend=OC.host_reads_backend)
        got_summary = _read_summary(info["got"], OC.N_HOST)
    else:
        bad, _ = FP.run_case(7, genome=genome, pairs=(s["m1"], s["m2"]), variants=variants, quals=None if s["q1"] is None else (s["q1"], s["q2"]), extra=c.opts,
                             verbose=3, info=info, ref_timeout=REF_TIMEOUT, base=base, backend=OC.host_pairs_backend, stride=SU.AL_MAX_RESULTS)
        got_summary = _pair_summary(info["got"], OC.N_HOST)
    assert bad == 0, (c.name, kind)
    left = (OC.host_reads_backend if kind == "reads" else OC.host_pairs_backend).left()
    print(c.name, kind, "second pass:", (OC.host_reads_backend if kind == "reads" else OC.host_pairs_backend).second_pass, "flagged after it:", info["overflow"], left)
    assert all(b & ~c.flags == 0 for b in left), (c.name, kind, left)      # what may stay flagged is named in the table
    # the summary the reference printed is the summary of these lines (equal lines, equal counts: the count lines say which classes the case exercised)
    nums = [x for x, _ in _summary_numbers(info["ref_err"])]
    assert nums[:5] == got_summary, (c.name, kind, info["ref_err"])
    return nums


@pytest.mark.parametrize("kind", ["reads", "pairs"])
@pytest.mark.parametrize("c", [c for c in OC.CASES if c.reference == "equal"], ids=[c.name for c in OC.CASES if c.reference == "equal"])
def test_machine_equals_the_reference(linear, c, kind):
    nums = _against_the_reference(c, linear, kind)
    if c.name in ("c0", "c40000-clamped") and kind == "reads":
        assert 0 < nums[3] + nums[4] < OC.N_HOST // 4       # exact matches only: at a substitution rate of 0.03 a read of 101 bases is clean about one time in 20


@pytest.mark.parametrize("kind", ["reads", "pairs"])
@pytest.mark.parametrize("name", OC.GRAPH_CASES)
def test_machine_equals_the_reference_on_a_graph(graph, name, kind):
    _against_the_reference(OC.BY_NAME[name], graph, kind)


def _fast_check(c, idx, kind, variant):
    import fast_check as FC
    base, src, _, _ = idx
    s = OC.read_set(c, src, OC.N_HOST, OC.HOST_GENOME["seed"])
    if kind == "pairs":
        r = FC.fast_check(base, s["m1"], s["m2"], quals=s["q1"], quals2=s["q2"], options=c.opts, variant=variant)
    else:
        r = FC.fast_check(base, s["reads"], quals=s["qr"], options=c.opts, variant=variant)
    r.pop("done")
    print(c.name, kind, repr(variant), r)
    assert r["mismatching"] == 0, (c.name, kind, variant, r)
    if c.expect == "bails_whole":
        assert r["completed"] == 0 and r["bails"] == {c.reason: OC.N_HOST}, (c.name, kind, variant, r)
    else:
        assert r["completed"] >= c.floors[0 if kind == "pairs" else 1] * OC.N_HOST, (c.name, kind, variant, r)
    return r


@pytest.mark.parametrize("kind", ["reads", "pairs"])
@pytest.mark.parametrize("variant", ["", "am"])
@pytest.mark.parametrize("c", OC.CASES, ids=IDS)
def test_fast_pass_equals_the_machine(linear, c, variant, kind):
    _fast_check(c, linear, kind, variant)


@pytest.mark.parametrize("kind", ["reads", "pairs"])
@pytest.mark.parametrize("c", OC.CASES, ids=IDS)
def test_fast_pass_equals_the_machine_on_a_graph(graph, c, kind):
    """variant "g" (the configuration of h2g_k_go_fast_graph.hip) over the SNP graph, reads from the alternate haplotype"""
    _fast_check(c, graph, kind, "g")
