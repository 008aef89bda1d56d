"""hisat2-align-amd --h2g-device-plan (plain reads planned on the device, the host planner over the rest) against --h2g-device-sam and against neither:
the SAM file, stderr and the --un-conc / --al-conc / --novel-splicesite-outfile files must be the same bytes three ways — paired, unpaired, a --tab6 mix, the
temporary-splice-site waves at -p 2, a known-site database with far-apart mates — on at most 2 000 records at --batch 1000, so that several items pass.  --h2g-stats
must show device_planned > 0 and device_planned + host_planned equal to the records."""
import json
import os
import subprocess

import pytest

import readsets_util as RU
from hisat2_amd import synth
from test_gpu_sam_text_cli import CLI, FRONT, REF, _golden_pair_files, build, needs_ref

pytestmark = pytest.mark.gpu
MODES = (("host", []), ("dev", ["--h2g-device-sam"]), ("plan", ["--h2g-device-plan"]))


def three_ways(tmp, args, files=(), exe=CLI):
    """runs `exe args` with neither option, with --h2g-device-sam and with --h2g-device-plan -> (SAM body lines, stats of the planned run)"""
    dirs = {}
    for tag, extra in MODES:
        d = tmp / tag
        d.mkdir()
        a = list(args) + extra + ["--batch", "1000", "--h2g-stats", str(d / "stats.json"), "-S", str(d / "out.sam")]
        for f in files:
            a += [f, str(d / f.strip("-"))]
        r = subprocess.run([exe] + a, stderr=open(d / "err", "w"), cwd=str(d), timeout=300)
        assert r.returncode == 0, open(d / "err").read()[-1500:]
        dirs[tag] = d

    def sam(tag):
        b = open(dirs[tag] / "out.sam", "rb").read().replace(b" --h2g-device-sam", b"").replace(b" --h2g-device-plan", b"")
        for d in dirs.values():
            b = b.replace(str(d).encode(), b"@")
        return b.split(b"\n")
    want = sam("host")
    for tag in ("dev", "plan"):
        got = sam(tag)
        assert len(got) == len(want) and not [(x, y) for x, y in zip(got, want) if x != y][:2], tag
        assert open(dirs[tag] / "err", "rb").read() == open(dirs["host"] / "err", "rb").read(), tag
        for f in files:
            names = sorted(p.name for p in dirs["host"].iterdir() if p.name.startswith(f.strip("-")))
            assert names and names == sorted(p.name for p in dirs[tag].iterdir() if p.name.startswith(f.strip("-")))
            for nm in names:
                assert open(dirs["host"] / nm, "rb").read() == open(dirs[tag] / nm, "rb").read(), (tag, nm)
    st = {tag: json.load(open(dirs[tag] / "stats.json")) for tag in dirs}
    body = [l for l in want if l and not l.startswith(b"@")]
    sp = st["plan"]
    print("--h2g-device-plan:", sp)
    assert st["host"]["device_planned"] == 0 and st["dev"]["device_planned"] == 0 and st["dev"]["host_planned"] == 0
    assert sp["device_planned"] > 0 and sp["device_planned"] + sp["host_planned"] == sp["reads"] == st["host"]["reads"]
    assert sp["device_sam_lines"] == st["dev"]["device_sam_lines"] >= len(body) > 0
    return body, sp


def test_paired(tmp_path, g1_index, golden_dir):
    rd = _golden_pair_files(tmp_path, golden_dir)
    body, st = three_ways(tmp_path, ["-f", "-p", "4", "--no-spliced-alignment", "-x", g1_index] + rd, files=["--un-conc", "--al-conc"], exe=FRONT)
    assert st["device_planned"] > st["reads"] // 2


def test_paired_options_through_the_front_end(tmp_path, g1_index, golden_dir):
    rd = _golden_pair_files(tmp_path, golden_dir)
    body, st = three_ways(tmp_path, ["-f", "-p", "4", "--no-spliced-alignment", "-x", g1_index] + rd +
                          ["-k", "5", "--no-unal", "--no-mixed", "--rna-strandness", "RF", "--rg-id", "g", "--rg", "SM:x"], exe=FRONT)
    assert all(b"\tRG:Z:g" in l and b"\tXS:A:" in l for l in body) and not any(int(l.split(b"\t")[1]) & 4 for l in body)


def test_unpaired(tmp_path, g1_index, golden_dir):
    import gzip
    open(tmp_path / "r.fa", "wb").write(gzip.open(os.path.join(golden_dir, "reads_se.fa.gz")).read())
    body, st = three_ways(tmp_path, ["-f", "-p", "4", "--no-spliced-alignment", "-x", g1_index, "-U", str(tmp_path / "r.fa")], files=["--un", "--al"], exe=FRONT)
    assert st["device_planned"] > st["reads"] // 2


def test_tab6_mix(tmp_path, g1_index, golden_dir):
    genome = RU.load_genome(golden_dir)
    recs = RU.make_records(genome, 8301, 2000)
    RU.write_tabbed(str(tmp_path / "mix.tab6"), recs, six=True)
    body, st = three_ways(tmp_path, ["-p", "4", "--no-spliced-alignment", "-x", g1_index, "--tab6", str(tmp_path / "mix.tab6")])
    flags = [int(l.split(b"\t")[1]) for l in body]
    assert any(f & 1 for f in flags) and any(not (f & 1) for f in flags)               # pairs and unpaired reads in one run


@needs_ref
def test_paired_spliced_temporary_splice_sites(tmp_path):
    """the default mode at -p 2: waves of 2 000 pairs, each wave's junctions merged before the next; junction reads are handed on and their sites collected"""
    import fuzz_spliced as FS
    import fuzz_spliced_pairs as FP
    contigs, m1, m2, _ = FP.make_case(351, 2000)
    base = build(tmp_path, contigs, FS.contig_names(contigs))
    synth.write_reads_fasta(str(tmp_path / "1.fa"), m1); synth.write_reads_fasta(str(tmp_path / "2.fa"), m2)
    body, st = three_ways(tmp_path, ["-f", "-p", "2", "-x", base, "-1", str(tmp_path / "1.fa"), "-2", str(tmp_path / "2.fa")], files=["--novel-splicesite-outfile"])
    assert any(b"N" in l.split(b"\t")[5] for l in body) and st["host_planned"] > 0


@needs_ref
def test_known_sites_and_template_length_adjustment(tmp_path):
    """a known-site database with template-length adjustment on: concordant mates on either side of an intron get their TLEN from the database, on the host"""
    import fuzz_spliced as FS
    import fuzz_spliced_pairs as FP
    contigs, m1, m2, introns = FP.make_case(371, 2000, sub=0.01)
    base = build(tmp_path, contigs, FS.contig_names(contigs))
    synth.write_reads_fasta(str(tmp_path / "1.fa"), m1); synth.write_reads_fasta(str(tmp_path / "2.fa"), m2)
    with open(tmp_path / "ss.txt", "w") as f:
        for t, l, r, d in FS.known_sites(introns, 371, 0.8):
            f.write("chr1\t%d\t%d\t%s\n" % (l, r, d))
    args = ["-f", "-p", "4", "--no-temp-splicesite", "-x", base, "-1", str(tmp_path / "1.fa"), "-2", str(tmp_path / "2.fa"), "--known-splicesite-infile", str(tmp_path / "ss.txt")]
    body, st = three_ways(tmp_path, args)
    assert st["host_planned"] > 0
    # the database matters for TLEN on this input: without the adjustment some lines differ
    d = tmp_path / "noadj"
    d.mkdir()
    subprocess.run([CLI] + args + ["--no-templatelen-adjustment", "--batch", "1000", "-S", str(d / "out.sam")], check=True, stderr=open(d / "err", "w"), timeout=300)
    other = [l.rstrip(b"\n") for l in open(d / "out.sam", "rb") if not l.startswith(b"@")]
    assert len(other) == len(body) and sum(1 for x, y in zip(other, body) if x.split(b"\t")[8] != y.split(b"\t")[8]) > 0
