"""GPU: the rest of the transcriptome policy through the command line — --avoid-pseudogene, --tmo, --no-anchorstop, --pen-conflictsplice —
against the reference binary: every SAM body line and the alignment summary byte-identical.  The genome carries multi-exon genes (GT..AG
introns) and processed pseudogenes (a gene's exons joined, more than 20 kbp from any splice site; identical, or about one mismatch in
200 bp); the reads come from the spliced transcripts, so an exonic read aligns as well to its gene as to the gene's processed copy.  Every
case also checks that the option changes the reference's own output on its fixture, by at least a stated number of lines."""
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import sam_lines as SL
from hisat2_amd import synth
from test_sam_lines import diff_lines

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "hisat2_amd", "hisat2-align-amd")
REF = os.path.join(ROOT, "oracle", "_ref")
needs_ref = pytest.mark.skipif(not os.path.exists(os.path.join(REF, "hisat2-align-s")), reason="needs oracle/_ref")
GAP = 22000            # random sequence between two genes / pseudogenes: every processed copy lies > 20 kbp from any splice site


def _revcomp(r):
    return np.where(r > 3, 4, 3 - r)[::-1].astype(np.uint8)


def make_genome(seed, ngenes=24, div=0.0, repeats=False):
    """chr1: genes of 3-4 exons (150-600 bp) with GT..AG introns (250-3000 bp), then one processed pseudogene per gene (every other one
    reverse-complemented; `div` = substitution rate of the copies); chr2: more processed copies.  repeats: copies of a few 300 bp elements
    scattered through the gaps (the anchor-stop rule of the partial search then matters).  Returns (contigs, genes = [(exons)], introns)."""
    rng = np.random.default_rng(seed)
    elements = [rng.integers(0, 4, size=300, dtype=np.uint8) for _ in range(4)]

    def gap(n):
        g = rng.integers(0, 4, size=n, dtype=np.uint8)
        if repeats:
            for _ in range(n // 2500):
                e = elements[int(rng.integers(0, len(elements)))].copy()
                m = rng.random(len(e)) < 0.02
                e[m] = (e[m] + rng.integers(1, 4, size=int(m.sum()))) % 4
                p = int(rng.integers(0, n - len(e)))
                g[p:p + len(e)] = e
        return g

    parts, pos, genes, introns = [], 0, [], []
    for _ in range(ngenes):
        parts.append(gap(GAP)); pos += GAP
        ex = []
        for k in range(int(rng.integers(3, 5))):
            if k:
                L = int(rng.integers(250, 3000))
                intr = rng.integers(0, 4, size=L, dtype=np.uint8)
                intr[:2] = [2, 3]; intr[-2:] = [0, 2]              # GT .. AG
                introns.append((pos, pos + L))
                parts.append(intr); pos += L
            L = int(rng.integers(150, 600))
            parts.append(rng.integers(0, 4, size=L, dtype=np.uint8))
            ex.append((pos, pos + L)); pos += L
        genes.append(ex)
    chr1 = np.concatenate(parts)
    copies = []
    for i, ex in enumerate(genes):
        c = np.concatenate([chr1[a:b] for a, b in ex]).copy()
        if div > 0:
            m = rng.random(len(c)) < div
            c[m] = (c[m] + rng.integers(1, 4, size=int(m.sum()))) % 4
        copies.append(_revcomp(c) if i % 2 else c)
    tail = []
    for c in copies[: ngenes // 2 + 1]:
        tail += [gap(GAP), c]
    tail.append(gap(GAP))
    chr1 = np.concatenate([chr1] + tail)
    chr2 = []
    for c in copies[ngenes // 2 + 1:]:
        chr2 += [gap(GAP), c]
    chr2.append(gap(GAP))
    return [chr1, np.concatenate(chr2)], genes, introns


def _transcript(chr1, ex):
    return np.concatenate([chr1[a:b] for a, b in ex])


def make_reads(contigs, genes, n, seed, rdlen=101, sub=0.004):
    rng = np.random.default_rng(seed)
    reads = np.empty((n, rdlen), dtype=np.uint8)
    for i in range(n):
        t = _transcript(contigs[0], genes[int(rng.integers(0, len(genes)))])
        s = int(rng.integers(0, len(t) - rdlen + 1))
        r = t[s:s + rdlen].copy()
        m = rng.random(rdlen) < sub
        r[m] = (r[m] + rng.integers(1, 4, size=int(m.sum()))) % 4
        reads[i] = _revcomp(r) if rng.random() < 0.5 else r
    return reads


def make_pairs(contigs, genes, n, seed, rdlen=101, sub=0.004):
    rng = np.random.default_rng(seed)
    m1, m2 = np.empty((n, rdlen), dtype=np.uint8), np.empty((n, rdlen), dtype=np.uint8)
    for i in range(n):
        t = _transcript(contigs[0], genes[int(rng.integers(0, len(genes)))])
        f = min(len(t), int(rng.integers(220, 380)))
        s = int(rng.integers(0, len(t) - f + 1))
        a, b = t[s:s + rdlen].copy(), _revcomp(t[s + f - rdlen:s + f])
        for r in (a, b):
            m = rng.random(rdlen) < sub
            r[m] = (r[m] + rng.integers(1, 4, size=int(m.sum()))) % 4
        if rng.random() < 0.5:
            a, b = b, a
        m1[i], m2[i] = a, b
    return m1, m2


def write_annotation(tmp, genes, introns):
    ss, ex = os.path.join(tmp, "ss.txt"), os.path.join(tmp, "exon.txt")
    with open(ss, "w") as f:
        for a, b in introns:
            f.write("chr1\t%d\t%d\t+\n" % (a - 1, b))
    with open(ex, "w") as f:
        for g in genes:
            for a, b in g:
                f.write("chr1\t%d\t%d\t+\n" % (a, b - 1))
    return ss, ex


def build(tmp, contigs, tran=None, snp_seed=None):
    fa, base = os.path.join(tmp, "g.fa"), os.path.join(tmp, "g")
    synth.write_fasta(fa, contigs)
    cmd = [os.path.join(REF, "hisat2-build-s"), "-q"]
    if tran:
        cmd += ["--ss", tran[0], "--exon", tran[1]]
    if snp_seed is not None:
        snp = os.path.join(tmp, "g.snp")
        synth.write_snps(snp, synth.make_snps(contigs, snp_seed, every=400))
        cmd += ["--snp", snp]
    subprocess.run(cmd + [fa, base], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return base


def ref_run(tmp, tag, base, inputs, opts, p=1):
    sam, err = os.path.join(tmp, tag + ".ref.sam"), os.path.join(tmp, tag + ".ref.err")
    subprocess.run([os.path.join(REF, "hisat2-align-s"), "-f", "-p", str(p), "--reorder", "-x", base, "-S", sam] + inputs + list(opts),
                   check=True, stdout=subprocess.DEVNULL, stderr=open(err, "w"), timeout=900)
    return sam, err


def amd_run(tmp, tag, base, inputs, opts, p=4, batch=3000):
    sam, err = os.path.join(tmp, tag + ".amd.sam"), os.path.join(tmp, tag + ".amd.err")
    subprocess.run([CLI, "-f", "-p", str(p), "--batch", str(batch), "-x", base, "-S", sam] + inputs + list(opts),
                   check=True, stderr=open(err, "w"), timeout=900)
    return sam, err


def both(tmp, tag, base, inputs, opts, amd_p=4):
    """the command line against the reference (-p 1) with `opts`: returns the reference's body lines"""
    rs, re_ = ref_run(tmp, tag, base, inputs, opts)
    as_, ae = amd_run(tmp, tag, base, inputs, opts, p=amd_p)
    want = SL.body_lines(rs)
    assert diff_lines(SL.body_lines(as_), want) == 0
    assert open(ae).read() == open(re_).read()
    return want


def differs(tmp, tag, base, inputs, with_opt, without, want_min):
    """the reference's own output with and without the option under test: at least `want_min` lines of the first are not in the second"""
    ws, _ = ref_run(tmp, tag + ".without", base, inputs, without)
    n = sum((Counter(with_opt) - Counter(SL.body_lines(ws))).values())
    assert n >= want_min, n


@pytest.fixture(scope="module")
def linear_case(tmp_path_factory):
    t = str(tmp_path_factory.mktemp("tp_lin"))
    contigs, genes, introns = make_genome(501, div=0.0)
    base = build(t, contigs)
    ss, _ = write_annotation(t, genes, introns)
    rfa, f1, f2 = os.path.join(t, "r.fa"), os.path.join(t, "r1.fa"), os.path.join(t, "r2.fa")
    synth.write_reads_fasta(rfa, make_reads(contigs, genes, 6000, 502))
    m1, m2 = make_pairs(contigs, genes, 4000, 503)
    synth.write_reads_fasta(f1, m1)
    synth.write_reads_fasta(f2, m2)
    return t, base, ss, rfa, f1, f2


@needs_ref
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("k", [(), ("-k", "1")])
def test_avoid_pseudogene_linear_known_sites(linear_case, paired, k):
    t, base, ss, rfa, f1, f2 = linear_case
    inputs = ["-1", f1, "-2", f2] if paired else ["-U", rfa]
    common = ["--no-temp-splicesite", "--known-splicesite-infile", ss] + list(k)
    tag = "lin%d%s" % (int(paired), "k1" if k else "")
    want = both(t, tag, base, inputs, common + ["--avoid-pseudogene"])
    differs(t, tag, base, inputs, want, common, 2000)


@pytest.fixture(scope="module", params=["tran", "tran_snp"])
def tran_case(request, tmp_path_factory):
    t = str(tmp_path_factory.mktemp("tp_" + request.param))
    contigs, genes, introns = make_genome(511 if request.param == "tran" else 521, div=0.0 if request.param == "tran" else 0.005)
    ss, ex = write_annotation(t, genes, introns)
    base = build(t, contigs, tran=(ss, ex), snp_seed=523 if request.param == "tran_snp" else None)
    rfa = os.path.join(t, "r.fa")
    synth.write_reads_fasta(rfa, make_reads(contigs, genes, 5000, 512))
    return t, base, rfa


@needs_ref
@pytest.mark.parametrize("opts,want_min", [(("--avoid-pseudogene",), 1000), (("--tmo",), 2000), (("--avoid-pseudogene", "--tmo"), 1500)])
def test_tran_index_policy(tran_case, opts, want_min):
    t, base, rfa = tran_case
    tag = "tran" + "".join(o.strip("-")[:3] for o in opts)
    common = ["--no-temp-splicesite"]
    want = both(t, tag, base, ["-U", rfa], common + list(opts))
    differs(t, tag, base, ["-U", rfa], want, common, want_min)


@needs_ref
def test_avoid_pseudogene_temporary_splice_sites_p1(tmp_path):
    """the default mode at -p 1: a read sees the junctions of every read before it, and the unfiltered query of --avoid-pseudogene every site
    of the database when its wave starts — here the reference's own -p 1 chain"""
    t = str(tmp_path)
    contigs, genes, _ = make_genome(531)
    base = build(t, contigs)
    rfa = os.path.join(t, "r.fa")
    synth.write_reads_fasta(rfa, make_reads(contigs, genes, 2500, 532))
    rs, re_ = ref_run(t, "tmp", base, ["-U", rfa], ["--avoid-pseudogene"])
    as_, ae = amd_run(t, "tmp", base, ["-U", rfa], ["--avoid-pseudogene"], p=1)
    want = SL.body_lines(rs)
    assert diff_lines(SL.body_lines(as_), want) == 0
    assert open(ae).read() == open(re_).read()
    differs(t, "tmp", base, ["-U", rfa], want, [], 800)


@needs_ref
def test_avoid_pseudogene_temporary_splice_sites_deterministic(tmp_path):
    """-p 4 in the default mode: the database a wave queries is the sites of the earlier waves, whatever --batch says"""
    t = str(tmp_path)
    contigs, genes, _ = make_genome(541)
    base = build(t, contigs)
    rfa = os.path.join(t, "r.fa")
    synth.write_reads_fasta(rfa, make_reads(contigs, genes, 12000, 542))
    a, _ = amd_run(t, "b3k", base, ["-U", rfa], ["--avoid-pseudogene"], p=4, batch=3000)
    b, _ = amd_run(t, "b50k", base, ["-U", rfa], ["--avoid-pseudogene"], p=4, batch=50000)
    la, lb = SL.body_lines(a), SL.body_lines(b)
    assert len(la) > 12000 and la == lb


@needs_ref
def test_tmo_without_spliced_alignment(linear_case):
    """--tmo under --no-spliced-alignment: no alignment is spliced through known sites, so every read ends up unaligned"""
    t, base, ss, rfa, f1, f2 = linear_case
    want = both(t, "tmons", base, ["-U", rfa], ["--no-spliced-alignment", "--tmo"])
    assert all(int(l.split("\t")[1]) & 4 for l in want)
    differs(t, "tmons", base, ["-U", rfa], want, ["--no-spliced-alignment"], 3000)


@pytest.fixture(scope="module")
def repeat_case(tmp_path_factory):
    t = str(tmp_path_factory.mktemp("tp_rep"))
    contigs, genes, _ = make_genome(551, div=0.01, repeats=True)
    base = build(t, contigs)
    rfa = os.path.join(t, "r.fa")
    reads = make_reads(contigs, genes, 3000, 552)
    rep = synth.make_reads(contigs, 3000, 101, 553, sub_rate=0.01)[0]          # reads from anywhere: many touch a repeat element
    synth.write_reads_fasta(rfa, np.concatenate([reads, rep]))
    return t, base, rfa


@needs_ref
@pytest.mark.parametrize("mode", [("--no-spliced-alignment",), ("--no-temp-splicesite",)])
def test_no_anchorstop(repeat_case, mode):
    t, base, rfa = repeat_case
    tag = "nas" + mode[0][5:8]
    want = both(t, tag, base, ["-U", rfa], list(mode) + ["--no-anchorstop"])
    differs(t, tag, base, ["-U", rfa], want, list(mode), 200)


@needs_ref
@pytest.mark.parametrize("pen,want_min", [("0", 700), ("12", 700)])
def test_pen_conflictsplice(tmp_path, pen, want_min):
    """reads across two junctions of opposite direction (a GT..AG intron next to a CT..AC one): the conflict penalty decides them"""
    t = str(tmp_path)
    rng = np.random.default_rng(561)
    parts, pos, ex = [], 0, []
    for _ in range(40):
        parts.append(rng.integers(0, 4, size=3000, dtype=np.uint8)); pos += 3000
        gene = []
        for k in range(3):
            if k:
                L = int(rng.integers(300, 1500))
                intr = rng.integers(0, 4, size=L, dtype=np.uint8)
                if k == 1:
                    intr[:2] = [2, 3]; intr[-2:] = [0, 2]         # GT .. AG (forward)
                else:
                    intr[:2] = [1, 3]; intr[-2:] = [0, 1]         # CT .. AC (reverse strand)
                parts.append(intr); pos += L
            L = int(rng.integers(30, 60)) if k == 1 else 200
            parts.append(rng.integers(0, 4, size=L, dtype=np.uint8))
            gene.append((pos, pos + L)); pos += L
        ex.append(gene)
    parts.append(rng.integers(0, 4, size=3000, dtype=np.uint8))
    contigs = [np.concatenate(parts)]
    base = build(t, contigs)
    reads = []
    for i in range(3000):
        g = ex[i % len(ex)]
        tr = _transcript(contigs[0], g)
        s = int(rng.integers(max(0, g[0][1] - g[0][0] - 80), g[0][1] - g[0][0] - 15))
        r = tr[s:s + 101]
        if len(r) == 101:
            reads.append(_revcomp(r) if i % 2 else r)
    rfa = os.path.join(t, "r.fa")
    synth.write_reads_fasta(rfa, np.array(reads))
    common = ["--no-temp-splicesite"]
    want = both(t, "csp" + pen, base, ["-U", rfa], common + ["--pen-conflictsplice", pen])
    differs(t, "csp" + pen, base, ["-U", rfa], want, common, want_min)
