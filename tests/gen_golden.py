#!/usr/bin/env python3
"""Regenerate tests/golden/ from the REAL reference (run in the build container only).

Needs oracle/_ref/{hisat2-build-s,hisat2-align-s,ref_probe} (make -C oracle ref).  Produces,
for a small seeded genome ("g1"):
  g1.fa.gz, g1.{1..8}.ht2.gz      genome + index written by the reference's hisat2-build-s
  reads_se.fa.gz                  400 x 101 bp reads (subs, a few Ns and indels)
  probe_{rank,ftab,offset,stretch,psearch,coords,extend}.txt.gz
                                  outputs of the reference classes via oracle/ref_probe.cpp
  ref_se_nospliced.sam.gz         hisat2-align-s -f -p 1 --no-spliced-alignment (minus @PG)
  ref_se_spliced.sam.gz           hisat2-align-s -f -p 1 (default), minus @PG
  reads_pe_{1,2}.fa.gz, ref_pe_nospliced.sam.gz   300 pairs and their -1/-2 --no-spliced-alignment SAM
`gen_golden.py sw` adds reads_sw.fa.gz + probe_sw.txt.gz (SwAligner call-site vectors), `gen_golden.py sw16` reads_sw16.fa.gz + probe_sw16.txt.gz (its 16-bit path); `gen_golden.py graph` adds the GRAPH index fixtures without touching the above:
  g1s.snp.gz, g1s.{1..8}.ht2.gz   ~500 seeded variants of g1 and the hisat2-build-s --snp graph index
  reads_snp.fa.gz                 300 reads drawn from the alternate haplotype (all variants applied)
  probe_g1s_{params,rank,glf,glf1,psearch,psearch_spliced,coords,coords_short,extend,adjust,adjust_short,lglf}.txt.gz   reference GFM graph-LF / group-walk outputs
`gen_golden.py frag` adds the FRAGMENTED assembly fixture (tests/frag_cases.py: ~217 texts, ~330 fragments, all-N records, N runs at record ends):
  gfrag.fa.gz, gfrag.{1..8}.ht2.gz, reads_gfrag.fa.gz (1500 reads, classes A-G, 36-150 bases)
  probe_gfrag_{params,offset,stretch,psearch,coords,extend,extend_fq,extsearch,localof}.txt.gz
                                  coords: getGenomeCoords with rejectStraddle 0 and 1; extend: max_leftext / max_rightext unbounded, 0, 1, 7, 33
                                  (_fq: the same reads as FASTQ with seeded qualities); localof: HGFM::getLocalGFM at and past every text's end
`gen_golden.py ragged` adds the TRIMMED read sets (tests/ragged_cases.py) on the index g1, without touching the above:
  ragged_se.fq.gz, ragged_pe_{1,2}.fq.gz   2000 reads / 1500 pairs of 0-300 bases, mates of different lengths, empty records
  ragged_{se,pe}.sam.gz, ragged_{se,pe}.err.gz   hisat2-align-s -q -p 1 --no-spliced-alignment: the SAM body, and stderr (length-filter warnings + summary)
`gen_golden.py dense` adds the IN-EDGE-RICH graph fixture (tests/dense_cases.py: families of repeat copies with SNPs at the same element offsets):
  gdense.fa.gz, gdense.snp.gz, gdense.{1..8}.ht2.gz, reads_gdense_kmers.fa.gz (3000 k-mers of 10-24 bases from the alternate haplotype)
  probe_gdense_{psearch,coords,extend,adjust}.txt.gz   ranges of up to 64 rows (ref_probe ... maxrows=64): in-edge lists and node ranges of up to 64
  reads_gdense_{se,pe_1,pe_2}.fa.gz, ref_gdense_{se,pe}.sam.gz   2000 reads / 1000 pairs of 101 bases and their --no-spliced-alignment SAM bodies
Everything is deterministic (seeds below); the fixtures are committed.
"""
import gzip
import os
import shutil
import subprocess
import sys
import tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from hisat2_amd import synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
GOLD = os.path.join(HERE, "golden")
SEED = 20260925


def run(cmd, **kw):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, **kw)


def gz_write(path, data: bytes):
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(data)


def main():
    os.makedirs(GOLD, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="h2gold")
    contigs = synth.make_genome([60000, 45000, 30000], SEED, n_gaps=1, gap_len=500, repeats=2, repeat_len=400)
    fa = os.path.join(tmp, "g1.fa")
    synth.write_fasta(fa, contigs)
    base = os.path.join(tmp, "g1")
    run([os.path.join(REF, "hisat2-build-s"), "-q", fa, base])
    gz_write(os.path.join(GOLD, "g1.fa.gz"), open(fa, "rb").read())
    for k in range(1, 9):
        gz_write(os.path.join(GOLD, f"g1.{k}.ht2.gz"), open(f"{base}.{k}.ht2", "rb").read())
    reads, _ = synth.make_reads(contigs, 400, 101, SEED + 1, sub_rate=0.01, indel_rate=0.0005, n_rate=0.0005)
    rfa = os.path.join(tmp, "reads_se.fa")
    synth.write_reads_fasta(rfa, reads)
    gz_write(os.path.join(GOLD, "reads_se.fa.gz"), open(rfa, "rb").read())
    probe = os.path.join(REF, "ref_probe")
    for cmd, args in [("params", []), ("rank", ["4000", "11"]), ("ftab", ["3000", "12"]), ("offset", ["2000", "13"]),
                      ("stretch", ["1500", "14"]), ("psearch", [rfa, "1"]), ("coords", [rfa, "1"]),
                      ("extend", [rfa, "1"])]:
        out = run([probe, cmd, base] + args).stdout
        gz_write(os.path.join(GOLD, f"probe_{cmd}.txt.gz"), out)
        print(cmd, len(out.splitlines()), "lines")
    # spliced-mode partial search (pseudogeneStop on linear indexes)
    out = run([probe, "psearch", base, rfa, "0"]).stdout
    gz_write(os.path.join(GOLD, "probe_psearch_spliced.txt.gz"), out)
    for name, extra in [("ref_se_nospliced", ["--no-spliced-alignment"]), ("ref_se_spliced", [])]:
        sam = os.path.join(tmp, name + ".sam")
        run([os.path.join(REF, "hisat2-align-s"), "-f", "-p", "1", "-x", base, "-U", rfa, "-S", sam] + extra)
        lines = [l for l in open(sam, "rb").read().splitlines(True) if not l.startswith(b"@PG")]
        gz_write(os.path.join(GOLD, name + ".sam.gz"), b"".join(lines))
    # paired-end: 300 pairs, some with a mate that fails / contains Ns
    m1, m2 = synth.make_pairs(contigs, 300, 101, SEED + 7, frag_mean=320, frag_sd=120, sub_rate=0.015)
    f1, f2 = os.path.join(tmp, "reads_pe_1.fa"), os.path.join(tmp, "reads_pe_2.fa")
    synth.write_reads_fasta(f1, m1)
    synth.write_reads_fasta(f2, m2)
    gz_write(os.path.join(GOLD, "reads_pe_1.fa.gz"), open(f1, "rb").read())
    gz_write(os.path.join(GOLD, "reads_pe_2.fa.gz"), open(f2, "rb").read())
    sam = os.path.join(tmp, "pe.sam")
    run([os.path.join(REF, "hisat2-align-s"), "-f", "-p", "1", "--no-spliced-alignment", "-x", base, "-1", f1, "-2", f2, "-S", sam])
    lines = [l for l in open(sam, "rb").read().splitlines(True) if not l.startswith(b"@PG")]
    gz_write(os.path.join(GOLD, "ref_pe_nospliced.sam.gz"), b"".join(lines))
    shutil.rmtree(tmp)
    tot = sum(os.path.getsize(os.path.join(GOLD, f)) for f in os.listdir(GOLD))
    print("golden bytes:", tot)


def main_graph():
    import numpy as np
    tmp = tempfile.mkdtemp(prefix="h2goldg")
    fa = os.path.join(tmp, "g1.fa")
    open(fa, "wb").write(gzip.open(os.path.join(GOLD, "g1.fa.gz")).read())
    contigs = synth.make_genome([60000, 45000, 30000], SEED, n_gaps=1, gap_len=500, repeats=2, repeat_len=400)
    snps = synth.make_snps(contigs, SEED + 11)
    snpf = os.path.join(tmp, "g1s.snp")
    synth.write_snps(snpf, snps)
    gz_write(os.path.join(GOLD, "g1s.snp.gz"), open(snpf, "rb").read())
    base = os.path.join(tmp, "g1s")
    run([os.path.join(REF, "hisat2-build-s"), "-q", "--snp", snpf, fa, base])
    for k in range(1, 9):
        gz_write(os.path.join(GOLD, f"g1s.{k}.ht2.gz"), open(f"{base}.{k}.ht2", "rb").read())
    alt = synth.apply_snps(contigs, snps)
    reads, _ = synth.make_reads(alt, 300, 101, SEED + 12, sub_rate=0.004)
    rfa = os.path.join(tmp, "reads_snp.fa")
    synth.write_reads_fasta(rfa, reads)
    gz_write(os.path.join(GOLD, "reads_snp.fa.gz"), open(rfa, "rb").read())
    short, _ = synth.make_reads(alt, 3000, 18, SEED + 13, sub_rate=0.0)   # 18-mers: many two-node (ref/alt) ranges
    sfa = os.path.join(tmp, "reads_snp_short.fa")
    synth.write_reads_fasta(sfa, short)
    gz_write(os.path.join(GOLD, "reads_snp_short.fa.gz"), open(sfa, "rb").read())
    probe = os.path.join(REF, "ref_probe")
    for name, cmd, args in [("coords", "coords", [rfa, "1"]), ("coords_short", "coords", [sfa, "1"]), ("extend", "extend", [rfa, "1"]),
                            ("lglf", "lglf", ["6000", "24"]), ("adjust", "adjust", [rfa, "1"]), ("adjust_short", "adjust", [sfa, "1"]),
                            ("params", "params", []), ("rank", "rank", ["3000", "21"]), ("glf", "glf", ["12000", "22"]),
                            ("glf1", "glf1", ["6000", "23"]), ("psearch", "psearch", [rfa, "1"]),
                            ("psearch_spliced", "psearch", [rfa, "0"])]:
        out = run([probe, cmd, base] + args).stdout
        gz_write(os.path.join(GOLD, f"probe_g1s_{name}.txt.gz"), out)
        print(name, len(out.splitlines()), "lines")
    shutil.rmtree(tmp)
    tot = sum(os.path.getsize(os.path.join(GOLD, f)) for f in os.listdir(GOLD))
    print("golden bytes:", tot)


def main_sw():
    """reads_sw.fa.gz (indel-rich reads of g1) + probe_sw.txt.gz: the reference SwAligner run exactly as hybridSearch
    calls it (frame, 8-bit end-to-end fill, gather, first nextAlignment) around every seed-hit coordinate"""
    tmp = tempfile.mkdtemp(prefix="h2goldsw")
    base = os.path.join(tmp, "g1")
    for k in range(1, 9):
        open(f"{base}.{k}.ht2", "wb").write(gzip.open(os.path.join(GOLD, f"g1.{k}.ht2.gz")).read())
    contigs = synth.make_genome([60000, 45000, 30000], SEED, n_gaps=1, gap_len=500, repeats=2, repeat_len=400)
    reads, _ = synth.make_reads(contigs, 400, 101, SEED + 21, sub_rate=0.02, indel_rate=0.01, n_rate=0.001)
    rfa = os.path.join(tmp, "reads_sw.fa")
    synth.write_reads_fasta(rfa, reads)
    gz_write(os.path.join(GOLD, "reads_sw.fa.gz"), open(rfa, "rb").read())
    out = run([os.path.join(REF, "ref_probe"), "sw", base, rfa, "1"]).stdout
    gz_write(os.path.join(GOLD, "probe_sw.txt.gz"), out)
    print("sw", len(out.splitlines()), "lines")
    shutil.rmtree(tmp)


def main_extsearch():
    """probe_extsearch.txt.gz / probe_g1s_extsearch.txt.gz: globalGFMSearch (hi_aligner.h:6606) and localGFMSearch (:6751) of the REAL
    classes as hybridSearch_recur calls them — on the local index under the read's true origin and its neighbours, from several read
    offsets, with and without uniqueStop / a hit-length limit.  Line: read fw rdoff kind tidx toff maxHitLen uniqueStop nelt hitlen top bot uniqueStopOut"""
    import numpy as np
    tmp = tempfile.mkdtemp(prefix="h2goldx")
    probe = os.path.join(REF, "ref_probe")
    contigs = synth.make_genome([60000, 45000, 30000], SEED, n_gaps=1, gap_len=500, repeats=2, repeat_len=400)
    snps = synth.make_snps(contigs, SEED + 11)
    alt = synth.apply_snps(contigs, snps)
    for tag, idx, src, rseed, nreads, rate, rname in (("", "g1", contigs, SEED + 1, 400, dict(sub_rate=0.01, indel_rate=0.0005, n_rate=0.0005), "reads_se.fa.gz"),
                                                      ("g1s_", "g1s", alt, SEED + 12, 300, dict(sub_rate=0.004), "reads_snp.fa.gz")):
        base = os.path.join(tmp, idx)
        for k in range(1, 9):
            open(f"{base}.{k}.ht2", "wb").write(gzip.open(os.path.join(GOLD, f"{idx}.{k}.ht2.gz")).read())
        reads, truth = synth.make_reads(src, nreads, 101, rseed, **rate)          # the committed reads, with their origins
        rfa = os.path.join(tmp, idx + "_reads.fa")
        open(rfa, "wb").write(gzip.open(os.path.join(GOLD, rname)).read())
        rng = np.random.default_rng(SEED + 77)
        q = []
        for i, (ci, pos, fw) in enumerate(truth):
            ci, pos, fw = int(ci), int(pos), int(fw)
            n = len(reads[i])
            for rdoff in (n - 1, int(rng.integers(30, n - 1))):
                q.append((i, fw, rdoff, 0, 0, 0, 0xffffffff, 1))
            for _ in range(4):
                rdoff = int(rng.integers(8, n))
                shift = int(rng.choice([0, 0, -56320, 56320]))
                toff = min(max(0, pos + shift), len(src[ci]) - 1)
                q.append((i, fw if rng.integers(0, 8) else 1 - fw, rdoff, 1, ci, toff, 0xffff if rng.integers(0, 2) else int(rng.integers(8, 40)), int(rng.integers(0, 2))))
        qf = os.path.join(tmp, "q.txt")
        open(qf, "w").write("".join(" ".join(map(str, x)) + "\n" for x in q))
        out = run([probe, "extsearch", base, rfa, qf]).stdout.decode().splitlines()
        assert len(out) == len(q), (len(out), len(q))
        body = "".join(" ".join(map(str, x)) + " " + o + "\n" for x, o in zip(q, out))
        gz_write(os.path.join(GOLD, f"probe_{tag}extsearch.txt.gz"), body.encode())
        print(tag + "extsearch", len(out), "lines,", sum(1 for o in out if not o.startswith("0 ")), "with elements")
    shutil.rmtree(tmp)


def main_sw16():
    """reads_sw16.fa.gz (150-base reads of g1 at 2 / 7 / 18 / 30 % substitutions, an indel each) + probe_sw16.txt.gz: the same call site with
    --score-min below -254, where SwAligner::align takes its 16-bit path (aligner_sw.cpp:496: alignNucleotidesEnd2EndSseI16 + the I16
    gather / backtrace).  Two runs of the probe: minsc -450, and minsc -900 with every seed coordinate also tried 777 bases to the right (unrelated placements:
    deep scores, many equal choices in the backtrace).  Alignments with more than H2G_MAX_EDITS edits are part of the vectors (score and
    offset are checked; the records flag the overflow)."""
    tmp = tempfile.mkdtemp(prefix="h2goldsw16")
    base = os.path.join(tmp, "g1")
    for k in range(1, 9):
        open(f"{base}.{k}.ht2", "wb").write(gzip.open(os.path.join(GOLD, f"g1.{k}.ht2.gz")).read())
    contigs = synth.make_genome([60000, 45000, 30000], SEED, n_gaps=1, gap_len=500, repeats=2, repeat_len=400)
    reads = np.concatenate([synth.make_reads(contigs, 150, 150, SEED + 31 + g, sub_rate=r, indel_rate=0.01, n_rate=0.002)[0] for g, r in enumerate((0.02, 0.07, 0.18, 0.30))])
    rfa = os.path.join(tmp, "reads_sw16.fa")
    synth.write_reads_fasta(rfa, reads)
    gz_write(os.path.join(GOLD, "reads_sw16.fa.gz"), open(rfa, "rb").read())
    out = b"".join(run([os.path.join(REF, "ref_probe"), "sw", base, rfa, "1", str(m), str(sh)]).stdout for m, sh in ((-450, 0), (-900, 777)))
    gz_write(os.path.join(GOLD, "probe_sw16.txt.gz"), out)
    print("sw16", len(out.splitlines()), "lines")
    shutil.rmtree(tmp)


def combine_reads(contigs, n, seed, rdlen=101):
    """reads made of two exact anchors of the genome with something for GenomeHit::combineWith to place between them: nothing (a plain join), mismatches,
    an insertion, a deletion, an intron (a jump of 20 ... 3000 reference bases).  Names = "id|fw|tidx|rdoffA|lenA|toffA|rdoffB|lenB|toffB" in the coordinates of
    the aligned strand.  -> (names, read arrays)"""
    rng = np.random.default_rng(seed)
    names, reads = [], []
    k = 0
    while k < n:
        tidx = int(rng.integers(0, len(contigs)))
        c = contigs[tidx]
        kind = int(rng.integers(0, 6))                       # 0 join, 1 mismatches, 2 insertion, 3 deletion, 4 intron, 5 deletion + mismatches
        lenA = int(rng.integers(18, 45)); lenB = int(rng.integers(18, 45))
        mid = rdlen - lenA - lenB                            # bases of the read between the anchors
        ins = int(rng.integers(1, 4)) if kind == 2 else 0
        skip = int(rng.integers(1, 16)) if kind in (3, 5) else int(rng.integers(20, 3000)) if kind == 4 else 0
        cut = int(rng.integers(1, mid)) if mid > 1 else 0   # where in the middle the event sits
        span = rdlen - ins + skip
        s0 = int(rng.integers(0, len(c) - span - 1))
        ref = c[s0:s0 + span]
        if (ref > 3).any():
            continue
        left = ref[:lenA + cut]
        right = ref[lenA + cut + skip:]
        strand = np.concatenate([left, rng.integers(0, 4, size=ins).astype(np.uint8), right])[:rdlen]
        if len(strand) != rdlen:
            continue
        if kind in (1, 5) and mid > 4:                       # substitutions strictly between the anchors
            for pos in rng.choice(np.arange(lenA + 1, lenA + mid - 1), size=min(2, mid - 2), replace=False):
                strand[pos] = (strand[pos] + int(rng.integers(1, 4))) & 3
        toA = s0
        roB = rdlen - lenB
        toB = s0 + span - lenB
        if not (np.array_equal(strand[:lenA], c[toA:toA + lenA]) and np.array_equal(strand[roB:], c[toB:toB + lenB])):
            continue
        fw = int(rng.integers(0, 2))
        rd = strand if fw else (3 - strand[::-1]).astype(np.uint8)
        names.append("%d|%d|%d|%d|%d|%d|%d|%d|%d" % (k, fw, tidx, 0, lenA, toA, roB, lenB, toB))
        reads.append(rd.astype(np.uint8))
        k += 1
    return names, reads


def main_combine():
    """probe_combine{,_spliced}.txt.gz + reads_combine.fa.gz: GenomeHit::combineWith of the reference on the g1 index"""
    import parity_cases as PC
    tmp = tempfile.mkdtemp(prefix="h2goldc")
    for k in range(1, 9):
        with gzip.open(os.path.join(GOLD, f"g1.{k}.ht2.gz"), "rb") as f, open(os.path.join(tmp, f"g1.{k}.ht2"), "wb") as o:
            shutil.copyfileobj(f, o)
    contigs = PC.load_contigs(GOLD)
    names, reads = combine_reads(contigs, 1500, SEED + 77)
    rfa = os.path.join(tmp, "reads_combine.fa")
    with open(rfa, "wb") as f:
        for nm, r in zip(names, reads):
            f.write(b">" + nm.encode() + b"\n" + synth._ALPHA[r].tobytes() + b"\n")
    gz_write(os.path.join(GOLD, "reads_combine.fa.gz"), open(rfa, "rb").read())
    for nosp, out in ((1, "probe_combine.txt.gz"), (0, "probe_combine_spliced.txt.gz")):
        txt = run([os.path.join(REF, "ref_probe"), "combine", os.path.join(tmp, "g1"), rfa, str(nosp)]).stdout
        gz_write(os.path.join(GOLD, out), txt)
        ok = sum(1 for l in txt.splitlines() if b"-> 1" in l)
        print(out, len(txt.splitlines()), "lines,", ok, "combined")
    shutil.rmtree(tmp)


def main_frag():
    sys.path.insert(0, HERE)
    import frag_cases as FC
    tmp = tempfile.mkdtemp(prefix="h2goldf")
    g = FC.make_frag_genome(FC.GFRAG_SEED, FC.GFRAG_TOTAL)
    base = FC.build_index(g, tmp, REF)
    os.rename(os.path.join(tmp, "g.fa"), os.path.join(tmp, "gfrag.fa"))
    gz_write(os.path.join(GOLD, "gfrag.fa.gz"), open(os.path.join(tmp, "gfrag.fa"), "rb").read())
    for k in range(1, 9):
        gz_write(os.path.join(GOLD, f"gfrag.{k}.ht2.gz"), open(f"{base}.{k}.ht2", "rb").read())
    reads, labels, origin = FC.make_frag_reads(g, FC.GFRAG_SEED + 1, FC.GFRAG_NREADS, with_origin=True)
    rfa, rfq = os.path.join(tmp, "reads_gfrag.fa"), os.path.join(tmp, "reads_gfrag.fq")
    FC.write_reads(rfa, reads)
    FC.write_reads(rfq, reads, FC.seeded_quals(reads, FC.GFRAG_SEED + 2))
    gz_write(os.path.join(GOLD, "reads_gfrag.fa.gz"), open(rfa, "rb").read())
    # the extension vectors: the classes whose exact-match cores end at a contig end / an N run / a repeat copy (B, D, F, G)
    keep = [i for i, c in enumerate(labels) if c in "BDFG"]
    xfa, xfq = os.path.join(tmp, "x.fa"), os.path.join(tmp, "x.fq")
    xr = [reads[i] for i in keep]
    FC.write_reads(xfa, xr)
    q = FC.seeded_quals(reads, FC.GFRAG_SEED + 2)
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    FC.write_reads(xfq, xr, np.concatenate([q[offs[i]:offs[i + 1]] for i in keep]))
    probe = os.path.join(REF, "ref_probe")
    for name, cmd, args in [("params", "params", []), ("offset", "offset", ["3000", "13"]), ("stretch", "stretch", ["3000", "14"]),
                            ("psearch", "psearch", [rfa, "1"]), ("localof", "localof", [])]:
        out = run([probe, cmd, base] + args).stdout
        gz_write(os.path.join(GOLD, f"probe_gfrag_{name}.txt.gz"), out)
        print(name, len(out.splitlines()), "lines")
    out = run([probe, "coords", base, rfa, "1", "0"]).stdout + run([probe, "coords", base, rfa, "1", "1"]).stdout
    gz_write(os.path.join(GOLD, "probe_gfrag_coords.txt.gz"), out)
    print("coords", len(out.splitlines()), "lines")
    for name, f in (("extend", xfa), ("extend_fq", xfq)):
        lines = run([probe, "extend", base, f, "1", "bounds"]).stdout.splitlines(True)
        # read ids of the subset -> ids of reads_gfrag; the FASTQ run keeps every third hit (the qualities only change scores)
        lines = [b"%d " % keep[int(l.split(b" ", 1)[0])] + l.split(b" ", 1)[1] for l in lines]
        if name == "extend_fq":
            lines = lines[::3]
        gz_write(os.path.join(GOLD, f"probe_gfrag_{name}.txt.gz"), b"".join(lines))
        print(name, len(lines), "lines")
    # extsearch: the local index under every read's origin (most texts here have ONE local index of a few dozen to a few hundred bases) and the
    # global index; offsets at and past the text's end go through localof
    text_of = {r: t for t, r in enumerate(g.texts)}
    rng = np.random.default_rng(FC.GFRAG_SEED + 77)
    qs = []
    for i, (rec, pos, fw) in enumerate(origin):
        n = len(reads[i])
        t = text_of[rec]
        tl = len(g.records[rec])
        qs.append((i, int(fw), n - 1, 0, 0, 0, 0xffffffff, 1))
        for _ in range(2):
            rdoff = int(rng.integers(8, n))
            toff = min(max(0, pos + int(rng.integers(0, n))), tl - 1)
            qs.append((i, int(fw) if rng.integers(0, 8) else 1 - int(fw), rdoff, 1, t, toff, 0xffff if rng.integers(0, 2) else int(rng.integers(8, 40)), int(rng.integers(0, 2))))
    qf = os.path.join(tmp, "q.txt")
    open(qf, "w").write("".join(" ".join(map(str, x)) + "\n" for x in qs))
    out = run([probe, "extsearch", base, rfa, qf]).stdout.decode().splitlines()
    assert len(out) == len(qs), (len(out), len(qs))
    gz_write(os.path.join(GOLD, "probe_gfrag_extsearch.txt.gz"), "".join(" ".join(map(str, x)) + " " + o + "\n" for x, o in zip(qs, out)).encode())
    print("extsearch", len(out), "lines,", sum(1 for o in out if not o.startswith("0 ")), "with elements")
    shutil.rmtree(tmp)
    for f in sorted(os.listdir(GOLD)):
        if "gfrag" in f:
            print(f, os.path.getsize(os.path.join(GOLD, f)))


def main_ragged():
    """tests/ragged_cases.py on the committed index g1: 2000 ragged reads and 1500 ragged pairs as FASTQ, the reference's SAM body and its stderr (the
    length-filter warnings, then the summary)"""
    sys.path.insert(0, HERE)
    import ragged_cases as RC
    tmp = tempfile.mkdtemp(prefix="h2goldr")
    for k in range(1, 9):
        open(os.path.join(tmp, f"g1.{k}.ht2"), "wb").write(gzip.open(os.path.join(GOLD, f"g1.{k}.ht2.gz")).read())
    base = os.path.join(tmp, "g1")
    contigs = synth.make_genome([60000, 45000, 30000], SEED, n_gaps=1, gap_len=500, repeats=2, repeat_len=400)
    minK, ftab = RC.index_params(base)
    reads, labels = RC.make_ragged_reads(contigs, RC.GOLDEN_SEED, RC.GOLDEN_NREADS, minK, ftab)
    m1, m2, plabels = RC.make_ragged_pairs(contigs, RC.GOLDEN_SEED + 1, RC.GOLDEN_NPAIRS, minK, ftab)
    files = {}
    for tag, rs, seed, pre in (("se", reads, 2, "r"), ("pe_1", m1, 3, "p"), ("pe_2", m2, 4, "p")):
        files[tag] = os.path.join(tmp, f"ragged_{tag}.fq")
        RC.write_reads(files[tag], rs, RC.seeded_quals(rs, RC.GOLDEN_SEED + seed), [f"{pre}{i}" for i in range(len(rs))])
        gz_write(os.path.join(GOLD, f"ragged_{tag}.fq.gz"), open(files[tag], "rb").read())
    for tag, inputs in (("se", ["-U", files["se"]]), ("pe", ["-1", files["pe_1"], "-2", files["pe_2"]])):
        sam = os.path.join(tmp, tag + ".sam")
        err = run([os.path.join(REF, "hisat2-align-s"), "-q", "-p", "1", "--no-spliced-alignment", "-x", base, "-S", sam] + inputs).stderr
        body = [l for l in open(sam, "rb") if not l.startswith(b"@")]
        gz_write(os.path.join(GOLD, f"ragged_{tag}.sam.gz"), b"".join(body))
        gz_write(os.path.join(GOLD, f"ragged_{tag}.err.gz"), err)
        ln = sum(1 for l in body if l.rstrip().endswith(b"YF:Z:LN"))
        if tag == "se":
            print("reads:", len(reads), "aligned", sum(1 for l in body if l.split(b"\t")[1] != b"4"), "YF:Z:LN lines", ln,
                  {c: sum(1 for x in labels if x == c) for c in RC.READ_CLASSES})
        else:
            print("pairs:", len(m1), "concordant", sum(1 for l in body if int(l.split(b"\t")[1]) & 2) // 2, "YF:Z:LN lines", ln,
                  {c: sum(1 for x in plabels if x == c) for c in RC.PAIR_CLASSES})
    shutil.rmtree(tmp)
    for f in sorted(os.listdir(GOLD)):
        if f.startswith("ragged_"):
            print(f, os.path.getsize(os.path.join(GOLD, f)))


def main_dense():
    """tests/dense_cases.py: the in-edge-rich graph fixture gdense (families of diverged repeat copies that carry SNPs at the same element offsets), its k-mers of
    10-24 bases from the alternate haplotype, the reference's vectors over them (ranges of up to DC.MAXROWS rows: `maxrows=`), the 2000 reads and 1000 pairs of
    101 bases from the alternate haplotype and the reference's SAM for them"""
    sys.path.insert(0, HERE)
    import dense_cases as DC
    tmp = tempfile.mkdtemp(prefix="h2goldd")
    g, where = DC.make_dense_genome()
    snps = DC.make_dense_snps(g, where)
    fa, snpf, base = os.path.join(tmp, "gdense.fa"), os.path.join(tmp, "gdense.snp"), os.path.join(tmp, "gdense")
    synth.write_fasta(fa, [g], names=[DC.NAME])
    synth.write_snps(snpf, snps)
    run([os.path.join(REF, "hisat2-build-s"), "-q", "--snp", snpf, fa, base])
    gz_write(os.path.join(GOLD, "gdense.fa.gz"), open(fa, "rb").read())
    gz_write(os.path.join(GOLD, "gdense.snp.gz"), open(snpf, "rb").read())
    for k in range(1, 9):
        gz_write(os.path.join(GOLD, f"gdense.{k}.ht2.gz"), open(f"{base}.{k}.ht2", "rb").read())
    kfa = os.path.join(tmp, "kmers.fa")
    DC.write_ragged_fasta(kfa, DC.make_kmers(g, where, snps))
    gz_write(os.path.join(GOLD, "reads_gdense_kmers.fa.gz"), open(kfa, "rb").read())
    probe = os.path.join(REF, "ref_probe")
    for name in ("psearch", "coords", "extend", "adjust"):
        out = run([probe, name, base, kfa, "1", f"maxrows={DC.MAXROWS}"]).stdout
        if name in ("extend", "adjust"):                       # one line per coordinate (and mismatch budget): every DC.THIN-th keeps the files small
            out = b"".join(out.splitlines(True)[::DC.THIN])
        gz_write(os.path.join(GOLD, f"probe_gdense_{name}.txt.gz"), out)
        print(name, len(out.splitlines()), "lines")
    reads, m1, m2 = DC.make_reads(g, snps)
    files = {}
    for tag, rs in (("se", reads), ("pe_1", m1), ("pe_2", m2)):
        files[tag] = os.path.join(tmp, f"reads_gdense_{tag}.fa")
        synth.write_reads_fasta(files[tag], rs)
        gz_write(os.path.join(GOLD, f"reads_gdense_{tag}.fa.gz"), open(files[tag], "rb").read())
    for tag, inputs in (("se", ["-U", files["se"]]), ("pe", ["-1", files["pe_1"], "-2", files["pe_2"]])):
        sam = os.path.join(tmp, tag + ".sam")
        run([os.path.join(REF, "hisat2-align-s"), "-f", "-p", "1", "--no-spliced-alignment", "-x", base, "-S", sam] + inputs)
        body = [l for l in open(sam, "rb") if not l.startswith(b"@")]
        gz_write(os.path.join(GOLD, f"ref_gdense_{tag}.sam.gz"), b"".join(body))
    shutil.rmtree(tmp)
    for f in sorted(os.listdir(GOLD)):
        if "gdense" in f:
            print(f, os.path.getsize(os.path.join(GOLD, f)))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "frag":
        main_frag()
    elif len(sys.argv) > 1 and sys.argv[1] == "dense":
        main_dense()
    elif len(sys.argv) > 1 and sys.argv[1] == "ragged":
        main_ragged()
    elif len(sys.argv) > 1 and sys.argv[1] == "combine":
        sys.path.insert(0, HERE)
        main_combine()
    elif len(sys.argv) > 1 and sys.argv[1] == "extsearch":
        main_extsearch()
    elif len(sys.argv) > 1 and sys.argv[1] == "graph":
        main_graph()
    elif len(sys.argv) > 1 and sys.argv[1] == "sw":
        main_sw()
    elif len(sys.argv) > 1 and sys.argv[1] == "sw16":
        main_sw16()
    else:
        main()
