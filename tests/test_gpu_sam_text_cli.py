"""hisat2-align-amd --h2g-device-sam (the SAM text written on the device from a host-made line plan) against the same command without the option:
the SAM file, stderr and the --novel-splicesite-outfile / --un-conc files must be the same bytes, in every mode the formatter stage serves — paired, unpaired, a
--tab6 mix, the temporary-splice-site waves, records beyond 32 edits, the read files of the front end — at --batch 1000, so that several items pass."""
import json
import os
import subprocess

import numpy as np
import pytest

import readsets_util as RU
from hisat2_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
CLI = os.path.join(ROOT, "hisat2_amd", "hisat2-align-amd")
FRONT = os.path.join(ROOT, "hisat2_amd", "hisat2-amd")
needs_ref = pytest.mark.skipif(not os.path.exists(os.path.join(REF, "hisat2-align-s")), reason="needs oracle/_ref")


def both_ways(tmp, args, files=(), exe=CLI):
    """runs `exe args` without and with --h2g-device-sam; `files`: option names whose argument is an output file -> (SAM body lines, stats) of the device run"""
    out = {}
    for tag, extra in (("host", []), ("dev", ["--h2g-device-sam"])):
        d = tmp / tag
        d.mkdir()
        a = list(args) + extra + ["--batch", "1000", "--h2g-stats", str(d / "stats.json"), "-S", str(d / "out.sam")]
        for f in files:
            a += [f, str(d / f.strip("-"))]
        r = subprocess.run([exe] + a, stderr=open(d / "err", "w"), cwd=str(d))
        assert r.returncode == 0, open(d / "err").read()[-1500:]
        out[tag] = d
    h, v = out["host"], out["dev"]
    sam_h = open(h / "out.sam", "rb").read().replace(b" --h2g-device-sam", b"").replace(str(h).encode(), b"@").replace(str(v).encode(), b"@")
    sam_v = open(v / "out.sam", "rb").read().replace(b" --h2g-device-sam", b"").replace(str(h).encode(), b"@").replace(str(v).encode(), b"@")
    hl, vl = sam_h.split(b"\n"), sam_v.split(b"\n")
    assert len(hl) == len(vl) and not [(x, y) for x, y in zip(hl, vl) if x != y][:2]
    assert open(h / "err", "rb").read() == open(v / "err", "rb").read()
    for f in files:
        names = sorted(p.name for p in h.iterdir() if p.name.startswith(f.strip("-")))
        assert names and names == sorted(p.name for p in v.iterdir() if p.name.startswith(f.strip("-")))
        for nm in names:
            assert open(h / nm, "rb").read() == open(v / nm, "rb").read(), nm
    sh, sv = json.load(open(h / "stats.json")), json.load(open(v / "stats.json"))
    body = [l for l in vl if l and not l.startswith(b"@")]
    assert sh["device_sam_lines"] == 0 and sv["device_sam_lines"] >= len(body) > 0
    assert all(sh[k] == sv[k] for k in ("reads", "overflow"))           # (how many reads the fast pass hands on varies from run to run: not compared)
    return body, sv


def build(tmp, contigs, names=None):
    fa, base = str(tmp / "g.fa"), str(tmp / "g")
    synth.write_fasta(fa, contigs, names=names)
    subprocess.run([os.path.join(REF, "hisat2-build-s"), "-q", fa, base], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return base


@needs_ref
def test_unpaired_spliced(tmp_path):
    import fuzz_spliced as FS
    contigs, reads, _ = FS.make_case(341, 3000, sub=0.005)
    base = build(tmp_path, contigs, FS.contig_names(contigs))
    synth.write_reads_fasta(str(tmp_path / "r.fa"), reads)
    novel = ["--novel-splicesite-outfile"]
    body, st = both_ways(tmp_path, ["-f", "-p", "4", "--no-temp-splicesite", "-x", base, "-U", str(tmp_path / "r.fa")], files=novel)
    assert sum(1 for l in body if b"N" in l.split(b"\t")[5]) > len(body) // 5          # the pool path (CIGAR / MD:Z from the host) is exercised
    assert st["whole_lines"] == 0


@needs_ref
def test_paired_spliced_temporary_splice_sites(tmp_path):
    import fuzz_spliced as FS
    import fuzz_spliced_pairs as FP
    contigs, m1, m2, _ = FP.make_case(351, 3000)
    base = build(tmp_path, contigs, FS.contig_names(contigs))
    synth.write_reads_fasta(str(tmp_path / "1.fa"), m1); synth.write_reads_fasta(str(tmp_path / "2.fa"), m2)
    body, st = both_ways(tmp_path, ["-f", "-p", "2", "-x", base, "-1", str(tmp_path / "1.fa"), "-2", str(tmp_path / "2.fa")], files=["--novel-splicesite-outfile"])
    assert any(b"N" in l.split(b"\t")[5] for l in body)


def _golden_pair_files(tmp, golden_dir):
    import gzip
    import shutil
    for m in (1, 2):
        with gzip.open(os.path.join(golden_dir, "reads_pe_%d.fa.gz" % m), "rb") as f, open(tmp / ("%d.fa" % m), "wb") as o:
            shutil.copyfileobj(f, o)
    return ["-1", str(tmp / "1.fa"), "-2", str(tmp / "2.fa")]


def test_golden_pairs_with_the_options_that_reach_the_tables(tmp_path, g1_index, golden_dir):
    rd = _golden_pair_files(tmp_path, golden_dir)
    body, st = both_ways(tmp_path, ["-f", "-p", "4", "--no-spliced-alignment", "-x", g1_index] + rd +
                         ["-k", "5", "--secondary", "--omit-sec-seq", "--no-unal", "--rna-strandness", "FR", "--rg-id", "g", "--rg", "SM:x", "--remove-chrname"])
    assert all(b"\tRG:Z:g" in l and b"\tXS:A:" in l for l in body) and not any(l.split(b"\t")[2].startswith(b"chr") for l in body)
    assert not any(int(l.split(b"\t")[1]) & 4 for l in body)


def test_tab6_mix(tmp_path, g1_index, golden_dir):
    genome = RU.load_genome(golden_dir)
    recs = RU.make_records(genome, 8301, 2500)
    RU.write_tabbed(str(tmp_path / "mix.tab6"), recs, six=True)
    body, st = both_ways(tmp_path, ["-p", "4", "--no-spliced-alignment", "-x", g1_index, "--tab6", str(tmp_path / "mix.tab6")])
    flags = [int(l.split(b"\t")[1]) for l in body]
    assert any(f & 1 for f in flags) and any(not (f & 1) for f in flags)               # pairs and unpaired reads in one run


def test_un_conc_through_the_front_end(tmp_path, g1_index, golden_dir):
    rd = _golden_pair_files(tmp_path, golden_dir)
    # a few pairs that align nowhere, so that --un-conc has something to hold
    rng = np.random.default_rng(8401)
    for m in (1, 2):
        with open(tmp_path / ("%d.fa" % m), "a") as f:
            for i in range(40):
                f.write(">junk%d\n%s\n" % (i, "".join("ACGT"[x] for x in rng.integers(0, 4, size=101))))
    body, st = both_ways(tmp_path, ["-f", "-p", "4", "--no-spliced-alignment", "-x", g1_index] + rd, files=["--un-conc"], exe=FRONT)
    held = sorted(p for p in (tmp_path / "dev").iterdir() if p.name.startswith("un-conc"))
    assert len(held) == 2 and all(sum(1 for l in open(p)) >= 80 for p in held)


@needs_ref
def test_long_deletions_travel_as_whole_lines(tmp_path):
    from test_long_edits_cpu import deletion_reads
    contigs = synth.make_genome([600000, 200000], 2901, n_gaps=1, gap_len=200, repeats=4, repeat_len=400)
    base = build(tmp_path, contigs)
    reads = deletion_reads(contigs, 2000, 101, 2902, dmin=30, dmax=30, sub=0.03)      # (30 deletion edits + three mismatches and more: beyond the 32 inline entries)
    synth.write_reads_fasta(str(tmp_path / "r.fa"), reads)
    args = ["-f", "--no-spliced-alignment", "-x", base, "-U", str(tmp_path / "r.fa"), "--score-min", "L,0,-2.4"]
    body, st = both_ways(tmp_path, ["-p", "4"] + args)
    assert st["whole_lines"] > 0 and st["whole_lines"] < st["device_sam_lines"] // 2
    # ... and this configuration against the reference binary as well
    subprocess.run([os.path.join(REF, "hisat2-align-s"), "-p", "1"] + args + ["-S", str(tmp_path / "ref.sam")], check=True, stderr=open(tmp_path / "ref.err", "w"))
    want = [l.rstrip(b"\n") for l in open(tmp_path / "ref.sam", "rb") if not l.startswith(b"@")]
    assert body == want
    assert open(tmp_path / "dev" / "err", "rb").read() == open(tmp_path / "ref.err", "rb").read()
