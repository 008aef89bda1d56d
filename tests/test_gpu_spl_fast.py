"""The fast pass of SPLICED runs on the device (h2g_k_go_fast_spl.hip: h2g_fast.h with FG_SPLICED = 1) against the spliced general machine on the device: the
batch of tests/spl_fast_cases.py — reads inside exons, reads across planted junctions, reads inside decoy exons of the known-sites file — with the pass on and
with H2G_GO_FAST=0 (separate processes: the switches are read once; the pass is switched on by name, H2G_FAST_SPLICED=1: it ships off) must give byte-identical results, for pairs and for single reads, with runs queued back to
back; the pass must take the reads inside exons, and the reads it hands on must come back spliced from the spliced units.  Then the temporary-splice-site mode
through the command line: the pass on == H2G_FAST_SPLICED=0 == `hisat2-align-s -p 2 --reorder`.

The floor on `fast`: tests/test_spl_fast_cpu.py, case gpu_layout (the first 5 000 reads / 4 000 pairs of this very batch through the host instantiation),
measured the share of class (a) that completes: 0.9150 of the reads and 0.8571 of the pairs without a database, the same with the known-sites file loaded
(a class-(a) read lies in an exon without decoys, 20 bases or more from any listed junction).  The floor is that share minus 0.1 absolute — the reads a
workgroup hands on at the end of a batch (FastArgs::tail, FB_TAIL) complete on the host and not here — times the number of class-(a) reads of the batch:
(0.9150 - 0.1) x n_a reads, (0.8571 - 0.1) x n_a pairs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sam_lines as SL
import spl_fast_cases as SC
from hisat2_amd import synth
from test_sam_lines import diff_lines

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
BUILD = os.path.join(REF, "hisat2-build-s")
CLI = os.path.join(ROOT, "hisat2_amd", "hisat2-align-amd")
needs_ref = pytest.mark.skipif(not os.path.exists(os.path.join(REF, "hisat2-align-s")), reason="needs oracle/_ref")

GENOME_SEED, READ_SEED, N = 31, 20261018, 40000          # (test_spl_fast_cpu.py: GENOME_SEED, GPU_LAYOUT)
SHARE_A = {"reads": 0.9150, "pairs": 0.8571}              # measured on the host (see above)


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("splgpu"))
    c = SC.make(READ_SEED, N, N, sub=0.005, genome_seed=GENOME_SEED)
    fa = os.path.join(tmp, "g.fa")
    synth.write_fasta(fa, [c.g], names=["chr1"])
    base = os.path.join(tmp, "g")
    subprocess.run([BUILD, "-q", "-p", "8", fa, base], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    npz = os.path.join(tmp, "reads.npz")
    np.savez(npz, m1=c.m1, m2=c.m2, reads=c.reads)
    ss = os.path.join(tmp, "ss.txt")
    SC.write_sites(ss, c.sites)
    return dict(tmp=tmp, base=base, npz=npz, ss=ss, case=c, ref={})


def digest(b, args, env):
    e = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"), **env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "spl_fast_digest.py"), b["base"], b["npz"]] + list(args), env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@needs_ref
@pytest.mark.parametrize("name,args,env,adopted", [
    ("nodb", (), {}, False),
    ("known", ("--sites", "SS"), {}, False),
    ("dta", ("--dta",), {}, False),
    ("drain", (), {"H2G_FAST_ORPHAN": "64", "H2G_DRAIN_GRID": "8"}, True),          # the end of the batch through k_go_fast_spl_drain
])
def test_spliced_fast_pass_equals_the_machine(batch, name, args, env, adopted):
    args = [batch["ss"] if a == "SS" else a for a in args]
    key = tuple(args)
    if key not in batch["ref"]:                          # the machine alone: once per option set, shared
        batch["ref"][key] = digest(batch, args, {"H2G_GO_FAST": "0"})
    off, on = batch["ref"][key], digest(batch, args, dict(env, H2G_FAST_SPLICED="1"))      # (switched on by name: the test holds whatever the default is)
    print(name, {"off": off, "on": on})
    c = batch["case"]
    for k, lab in (("pairs", c.plabel), ("reads", c.rlabel)):
        n_a = int((lab == SC.A).sum())
        print("%s %s: fast %d of %d (class (a): %d, floor %.0f), handed on %d, records with a splice edit %d" % (name, k, on[k]["fast"], N, n_a, (SHARE_A[k] - 0.1) * n_a, on[k]["handed_on"], on[k]["spliced_records"]))
        assert on[k]["sha"] == off[k]["sha"], k
        assert on[k]["aligned"] == off[k]["aligned"]
        assert on[k]["overflow"] == 0 and off[k]["overflow"] == 0
        assert off[k]["fast"] == 0
        assert on[k]["fast"] + on[k]["handed_on"] == N
        assert on[k]["spliced_records"] > 0                  # the hand-on into the spliced units was exercised
        assert on[k]["fast"] >= (SHARE_A[k] - 0.1) * n_a, (on[k], n_a)
        if adopted:
            assert on[k]["adopted"] > 0, on[k]


@needs_ref
def test_temporary_splice_sites_command_line(batch):
    """the reference's default mode (junctions of earlier reads help later ones) in waves of 1000 x -p pairs: every wave's run goes through the pass with that
    wave's database, and the SAM is the machine's and the reference's"""
    c, t = batch["case"], batch["tmp"]
    n = 6000
    f1, f2 = os.path.join(t, "r1.fa"), os.path.join(t, "r2.fa")
    synth.write_reads_fasta(f1, c.m1[:n])
    synth.write_reads_fasta(f2, c.m2[:n])
    common = ["-f", "-p", "2", "-x", batch["base"], "-1", f1, "-2", f2]
    subprocess.run([os.path.join(REF, "hisat2-align-s"), "--reorder", "-S", os.path.join(t, "ref.sam")] + common, check=True, stdout=subprocess.DEVNULL, stderr=open(os.path.join(t, "ref.err"), "w"))
    stats = os.path.join(t, "stats.json")
    subprocess.run([CLI, "--h2g-stats", stats, "-S", os.path.join(t, "on.sam")] + common, check=True, stderr=open(os.path.join(t, "on.err"), "w"), timeout=600,
                   env=dict(os.environ, H2G_FAST_SPLICED="1"))
    subprocess.run([CLI, "--h2g-stats", stats + "0", "-S", os.path.join(t, "off.sam")] + common, check=True, stderr=open(os.path.join(t, "off.err"), "w"), timeout=600,
                   env=dict(os.environ, H2G_FAST_SPLICED="0"))
    want, on, off = SL.body_lines(os.path.join(t, "ref.sam")), SL.body_lines(os.path.join(t, "on.sam")), SL.body_lines(os.path.join(t, "off.sam"))
    assert on == off
    assert diff_lines(on, want) == 0 and diff_lines(off, want) == 0
    assert open(os.path.join(t, "on.err")).read() == open(os.path.join(t, "ref.err")).read()
    s1, s0 = json.load(open(stats)), json.load(open(stats + "0"))
    print("temporary splice sites, 6 000 pairs:", s1, s0)
    assert s1["fast"] > 0 and s1["fast"] + s1["handed_on"] == n and s0["fast"] == 0
    assert sum(1 for l in want if "N" in l.split("\t")[5]) > n // 10


def _cli_on(tmp, base, inputs, extra, p="4"):
    """the command line with the pass switched on against `hisat2-align-s -p 1 --no-temp-splicesite`: SAM body and summary byte for byte; -> --h2g-stats"""
    t = str(tmp)
    common = ["-f", "--no-temp-splicesite", "-x", base] + inputs + list(extra)
    subprocess.run([os.path.join(REF, "hisat2-align-s"), "-p", "1", "-S", os.path.join(t, "ref.sam")] + common, check=True, stdout=subprocess.DEVNULL, stderr=open(os.path.join(t, "ref.err"), "w"))
    subprocess.run([CLI, "-p", p, "--batch", "3000", "--h2g-stats", os.path.join(t, "st.json"), "-S", os.path.join(t, "amd.sam")] + common, check=True, stderr=open(os.path.join(t, "amd.err"), "w"),
                   env=dict(os.environ, H2G_FAST_SPLICED="1"), timeout=600)
    assert diff_lines(SL.body_lines(os.path.join(t, "amd.sam")), SL.body_lines(os.path.join(t, "ref.sam"))) == 0
    assert open(os.path.join(t, "amd.err")).read() == open(os.path.join(t, "ref.err")).read()
    return json.load(open(os.path.join(t, "st.json")))


@needs_ref
@pytest.mark.parametrize("kind", ("unpaired", "paired", "known", "one_read_waves"))
def test_existing_spliced_cases_through_the_pass(tmp_path, kind):
    """cases of tests/test_gpu_zy_spliced.py (its generators, smaller) with H2G_FAST_SPLICED=1: the pass ships switched off, so those suites run the machine alone;
    here the same inputs go through k_go_fast_spl and its hand-on into the spliced units, against the reference binary"""
    import fuzz_spliced as F
    t = str(tmp_path)
    if kind == "one_read_waves":                         # a bare `-p 1` run: temporary splice sites with window 0, waves of one read, each a run of its own through the pass
        import gzip
        gold = os.path.join(ROOT, "tests", "golden")
        for k in range(1, 9):
            open(os.path.join(t, f"g1.{k}.ht2"), "wb").write(gzip.open(os.path.join(gold, f"g1.{k}.ht2.gz")).read())
        rfa = os.path.join(t, "r.fa")
        open(rfa, "wb").write(gzip.open(os.path.join(gold, "reads_se.fa.gz")).read())
        subprocess.run([CLI, "-f", "-x", os.path.join(t, "g1"), "-U", rfa, "--h2g-stats", os.path.join(t, "st.json"), "-S", os.path.join(t, "amd.sam")], check=True,
                       stderr=open(os.path.join(t, "amd.err"), "w"), env=dict(os.environ, H2G_FAST_SPLICED="1"), timeout=600)
        got = [l for l in open(os.path.join(t, "amd.sam")).read().splitlines() if not l.startswith("@")]
        want = [l for l in gzip.open(os.path.join(gold, "ref_se_spliced.sam.gz"), "rt").read().splitlines() if not l.startswith("@")]
        st = json.load(open(os.path.join(t, "st.json")))
        assert len(want) > 100 and got == want
    elif kind == "paired":
        import fuzz_spliced_pairs as FP
        contigs, m1, m2, _ = FP.make_case(352, 4000, sub=0.02)
        fa = os.path.join(t, "g.fa")
        synth.write_fasta(fa, contigs)
        subprocess.run([BUILD, "-q", fa, os.path.join(t, "g")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        f1, f2 = os.path.join(t, "r1.fa"), os.path.join(t, "r2.fa")
        synth.write_reads_fasta(f1, m1)
        synth.write_reads_fasta(f2, m2)
        st = _cli_on(tmp_path, os.path.join(t, "g"), ["-1", f1, "-2", f2], ())
    else:
        contigs, reads, introns = F.make_case(361 if kind == "known" else 342, 6000, sub=0.01 if kind == "known" else 0.02)
        fa = os.path.join(t, "g.fa")
        synth.write_fasta(fa, contigs)
        subprocess.run([BUILD, "-q", fa, os.path.join(t, "g")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        rfa = os.path.join(t, "r.fa")
        synth.write_reads_fasta(rfa, reads)
        extra = ()
        if kind == "known":
            ss = os.path.join(t, "ss.txt")
            with open(ss, "w") as f:
                for _, l, r, d in F.known_sites(introns, 361, 0.7):
                    f.write("chr1\t%d\t%d\t%s\n" % (l, r, d))
            extra = ("--known-splicesite-infile", ss)
        st = _cli_on(tmp_path, os.path.join(t, "g"), ["-U", rfa], extra)
    print(kind, st)
    assert st["fast"] > 0 and st["fast"] + st["handed_on"] == st["reads"]      # every run went through the pass
