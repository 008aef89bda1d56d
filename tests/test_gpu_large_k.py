"""GPU: -k up to 128 and --max-seeds up to 256 through the command line (the extra-large go() units, h2g_go_xl.h) against the reference
binary: every SAM body line and the alignment summary byte-identical, and no read flagged.  The genome carries families of about 200
near-identical copies (0-1 % divergence, both strands) of a few 0.5-3 kbp elements, and the reads come from the copies, so a read has far
more than 32 equally good placements and a pair more than 32 concordant pairings.  Every case also checks that the reference's own output
at its -k differs from its -k 30 output by a stated number of lines, and every case above -k 32 that the reference prints an NH:i above 32."""
import json
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
# lines by which the reference's output on the small family's reads differs from its -k 30 output (at least; measured well above)
SMALL_MIN = {"u50": 5000, "p64": 20000, "ptmp": 20000, "g100": 20000, "p33": 5000}
needs_ref = pytest.mark.skipif(not os.path.exists(os.path.join(REF, "hisat2-align-s")), reason="needs oracle/_ref")


def _revcomp(r):
    return np.where(r > 3, 4, 3 - r)[::-1].astype(np.uint8)


def make_genome(seed, length=3_000_000, elements=(700, 1300, 2400), copies=(150, 250), small=(900, 40)):
    """two contigs of random sequence with families of near-identical copies of `elements`, and one family of small[1] copies of a small[0] bp
    element; returns (contigs, [(contig, start, end, family)] of copies).  The large families are for the unspliced cases.  Spliced pairing joins
    every two copies within --max-intronlen (500 kbp): the spliced, graph and --secondary cases read the small family, whose lists the
    extra-large units hold (a 200-copy family makes lists of thousands there).  -k 31 reads it too: the large units hold its lists."""
    rng = np.random.default_rng(seed)
    contigs = [rng.integers(0, 4, size=length * 2 // 3, dtype=np.uint8), rng.integers(0, 4, size=length - length * 2 // 3, dtype=np.uint8)]
    spots = []
    for f, (L, nc) in enumerate([(L, int(rng.integers(copies[0], copies[1] + 1))) for L in elements] + [small]):
        e = rng.integers(0, 4, size=L, dtype=np.uint8)
        for _ in range(nc):
            c = e.copy()
            m = rng.random(L) < rng.random() * 0.01
            c[m] = (c[m] + rng.integers(1, 4, size=int(m.sum()))) % 4
            if rng.random() < 0.5:
                c = _revcomp(c)
            spots.append((int(rng.integers(0, 2)), c, f))
    placed, used = [], [[] for _ in contigs]
    for t, c, f in spots:
        for _ in range(100):
            p = int(rng.integers(0, len(contigs[t]) - len(c)))
            if all(p + len(c) + 200 < a or p > b + 200 for a, b in used[t]):
                contigs[t][p:p + len(c)] = c
                used[t].append((p, p + len(c)))
                placed.append((t, p, p + len(c), f))
                break
    return contigs, placed


def _mutate(rng, r, sub):
    m = rng.random(len(r)) < sub
    r[m] = (r[m] + rng.integers(1, 4, size=int(m.sum()))) % 4
    return r


def make_reads(contigs, copies, n, seed, rdlen=101, sub=0.005):
    rng = np.random.default_rng(seed)
    reads = np.empty((n, rdlen), dtype=np.uint8)
    for i in range(n):
        t, a, b, _ = copies[int(rng.integers(0, len(copies)))]
        s = int(rng.integers(a, b - rdlen + 1))
        r = _mutate(rng, contigs[t][s:s + rdlen].copy(), sub)
        reads[i] = _revcomp(r) if rng.random() < 0.5 else r
    return reads


def make_pairs(contigs, copies, n, seed, rdlen=101, sub=0.005):
    rng = np.random.default_rng(seed)
    m1, m2 = np.empty((n, rdlen), dtype=np.uint8), np.empty((n, rdlen), dtype=np.uint8)
    long_ = [c for c in copies if c[2] - c[1] >= 400]
    for i in range(n):
        t, a, b, _ = long_[int(rng.integers(0, len(long_)))]
        f = int(rng.integers(250, 401))
        s = int(rng.integers(a, b - f + 1))
        x = _mutate(rng, contigs[t][s:s + rdlen].copy(), sub)
        y = _mutate(rng, _revcomp(contigs[t][s + f - rdlen:s + f]), sub)
        if rng.random() < 0.5:
            x, y = y, x
        m1[i], m2[i] = x, y
    return m1, m2


def build(tmp, contigs, snp_seed=None):
    fa, base = os.path.join(tmp, "g.fa"), os.path.join(tmp, "g")
    synth.write_fasta(fa, contigs)
    cmd = [os.path.join(REF, "hisat2-build-s"), "-q"]
    if snp_seed is not None:       # a variant every ~400 bp: about a third of them fall inside the copies
        snp = os.path.join(tmp, "g.snp")
        synth.write_snps(snp, synth.make_snps(contigs, snp_seed, every=400))
        cmd += ["--snp", snp]
    subprocess.run(cmd + [fa, base], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return base


def ref_run(tmp, tag, base, inputs, opts, p=4):
    sam, err = os.path.join(tmp, tag + ".ref.sam"), os.path.join(tmp, tag + ".ref.err")
    subprocess.run([os.path.join(REF, "hisat2-align-s"), "-f", "-p", str(p), "--reorder", "-x", base, "-S", sam] + inputs + list(opts),
                   check=True, stdout=subprocess.DEVNULL, stderr=open(err, "w"), timeout=1200)
    return sam, err


def amd_run(tmp, tag, base, inputs, opts, p=4):
    sam, err, st = (os.path.join(tmp, tag + x) for x in (".amd.sam", ".amd.err", ".amd.json"))
    subprocess.run([CLI, "-f", "-p", str(p), "-x", base, "-S", sam, "--h2g-stats", st] + inputs + list(opts),
                   check=True, stderr=open(err, "w"), timeout=1200)
    return sam, err, json.load(open(st))


def both(tmp, tag, base, inputs, opts):
    """the command line against the reference (-p 4 --reorder) with `opts`: returns the reference's body lines"""
    rs, re_ = ref_run(tmp, tag, base, inputs, opts)
    as_, ae, st = amd_run(tmp, tag, base, inputs, opts)
    want = SL.body_lines(rs)
    assert diff_lines(SL.body_lines(as_), want) == 0
    assert open(ae).read() == open(re_).read()
    assert st["overflow"] == 0, st
    return want


def exercised(tmp, tag, base, inputs, want, opts_k30, want_min, k):
    """the reference at -k 30 differs from its output at `k` by at least want_min lines; above -k 32 it prints an NH:i above 32"""
    ws, _ = ref_run(tmp, tag + ".k30", base, inputs, opts_k30)
    n = sum((Counter(want) - Counter(SL.body_lines(ws))).values())
    assert n >= want_min, n
    if k > 32:
        nh = max((int(f[5:]) for l in want for f in l.split("\t")[11:] if f.startswith("NH:i:")), default=0)
        assert nh > 32, nh


def max_concordant(want):
    """the most concordant pairings the output prints for one pair (FLAG 0x2 lines of mate 1)"""
    c = Counter(l.split("\t")[0] for l in want if int(l.split("\t")[1]) & 0x42 == 0x42)
    return max(c.values(), default=0)


@pytest.fixture(scope="module")
def fam(tmp_path_factory):
    t = str(tmp_path_factory.mktemp("largek"))
    contigs, copies = make_genome(901)
    base = build(t, contigs)
    rfa, f1, f2 = os.path.join(t, "r.fa"), os.path.join(t, "r1.fa"), os.path.join(t, "r2.fa")
    big, small = [c for c in copies if c[3] < 3], [c for c in copies if c[3] == 3]
    synth.write_reads_fasta(rfa, make_reads(contigs, big, 2000, 902))
    synth.write_reads_fasta(os.path.join(t, "rs.fa"), make_reads(contigs, small, 1500, 904))
    s1, s2 = make_pairs(contigs, small, 1500, 905)
    synth.write_reads_fasta(os.path.join(t, "s1.fa"), s1)
    synth.write_reads_fasta(os.path.join(t, "s2.fa"), s2)
    m1, m2 = make_pairs(contigs, big, 1500, 903)
    synth.write_reads_fasta(f1, m1)
    synth.write_reads_fasta(f2, m2)
    return t, base, rfa, f1, f2, contigs, copies


@needs_ref
@pytest.mark.parametrize("opts,k,want_min,small", [
    (("--no-spliced-alignment", "-k", "100"), 100, 20000, False),
    (("-k", "50", "--max-seeds", "150", "--secondary", "--no-temp-splicesite"), 50, SMALL_MIN["u50"], True),
    # unspliced on an SNP-graph index: the extra-large graph unit WITHOUT the splice-site joins, which no other case runs (the small family's reads, as -k 31 below:
    # at least 200 lines beyond -k 30)
    (("--no-spliced-alignment", "-k", "100"), 100, 200, "graph"),
])
def test_unpaired_large_k(fam, tmp_path, opts, k, want_min, small):
    t, base, rfa = fam[:3]
    if small:
        rfa = os.path.join(t, "rs.fa")
    if small == "graph":
        t = str(tmp_path)
        base = build(t, fam[5], snp_seed=911)
    tag = "u" + "".join(o.strip("-")[:3] for o in opts)
    want = both(t, tag, base, ["-U", rfa], opts)
    k30 = [o if o != str(k) else "30" for o in opts]
    if "--max-seeds" in k30:
        k30[k30.index("--max-seeds") + 1] = "60"
    exercised(t, tag, base, ["-U", rfa], want, k30, want_min, k)


@needs_ref
def test_paired_unspliced_k100(fam):
    t, base, _, f1, f2 = fam[:5]
    inputs = ["-1", f1, "-2", f2]
    opts = ["--no-spliced-alignment", "-k", "100"]
    want = both(t, "pns100", base, inputs, opts)
    assert max_concordant(want) > 32
    exercised(t, "pns100", base, inputs, want, ["--no-spliced-alignment", "-k", "30"], 20000, 100)


@needs_ref
def test_paired_spliced_k64(fam):
    t, base = fam[:2]
    inputs = ["-1", os.path.join(t, "s1.fa"), "-2", os.path.join(t, "s2.fa")]
    want = both(t, "pspl64", base, inputs, ["--no-temp-splicesite", "-k", "64"])
    exercised(t, "pspl64", base, inputs, want, ["--no-temp-splicesite", "-k", "30"], SMALL_MIN["p64"], 64)


@needs_ref
def test_paired_temporary_splice_sites_p4(fam):
    """the default mode: the command line at -p 4 against the reference's -p 4 --reorder"""
    t, base = fam[:2]
    inputs = ["-1", os.path.join(t, "s1.fa"), "-2", os.path.join(t, "s2.fa")]
    want = both(t, "ptmp100", base, inputs, ["-k", "100"])
    exercised(t, "ptmp100", base, inputs, want, ["-k", "30"], SMALL_MIN["ptmp"], 100)


@needs_ref
def test_graph_index_paired_k100(fam, tmp_path):
    t0, contigs = fam[0], fam[5]
    t = str(tmp_path)
    base = build(t, contigs, snp_seed=911)
    inputs = ["-1", os.path.join(t0, "s1.fa"), "-2", os.path.join(t0, "s2.fa")]
    want = both(t, "g100", base, inputs, ["--no-temp-splicesite", "-k", "100"])
    exercised(t, "g100", base, inputs, want, ["--no-temp-splicesite", "-k", "30"], SMALL_MIN["g100"], 100)


@needs_ref
def test_edge_k31_large_units(fam):
    """-k 31, which the command line refused before: the large units run it, as the library always did.  Reads of the 40-copy family (more than
    30 placements each, within what the large units hold)"""
    t, base = fam[:2]
    inputs = ["-U", os.path.join(t, "rs.fa")]
    want = both(t, "e31", base, inputs, ["--no-spliced-alignment", "-k", "31"])
    exercised(t, "e31", base, inputs, want, ["--no-spliced-alignment", "-k", "30"], 200, 31)


@needs_ref
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("opts,k,want_min", [
    (("-k", "33"), 33, 10000),                         # the smallest XL run (--max-seeds 66)
    (("-k", "128", "--max-seeds", "256"), 128, 20000),
])
def test_edges(fam, paired, opts, k, want_min):
    t, base, rfa, f1, f2 = fam[:5]
    common = ["--no-spliced-alignment"]
    if paired and k == 33:
        # -k 33 with its 66 seeds makes report lists of more than 1024 on the large families: the small family's pairs, spliced (which pairs its
        # copies with each other: more than 32 placements per pair)
        f1, f2, want_min, common = os.path.join(t, "s1.fa"), os.path.join(t, "s2.fa"), SMALL_MIN["p33"], ["--no-temp-splicesite"]
    inputs = ["-1", f1, "-2", f2] if paired else ["-U", rfa]
    tag = "e%d%s" % (int(paired), "".join(opts))
    want = both(t, tag, base, inputs, common + list(opts))
    exercised(t, tag, base, inputs, want, common + ["-k", "30"], want_min, k)


@pytest.mark.parametrize("opts", [("-k", "129"), ("-k", "10", "--max-seeds", "257")])
def test_refused_beyond_range(tmp_path, opts):
    """outside 1 <= -k <= 128, -k <= --max-seeds <= 256: refused by name, no SAM body"""
    t = str(tmp_path)
    rng = np.random.default_rng(921)
    contigs = [rng.integers(0, 4, size=20000, dtype=np.uint8)]
    fa, base = os.path.join(t, "g.fa"), os.path.join(t, "g")
    synth.write_fasta(fa, contigs)
    if not os.path.exists(os.path.join(REF, "hisat2-build-s")):
        pytest.skip("needs oracle/_ref")
    subprocess.run([os.path.join(REF, "hisat2-build-s"), "-q", fa, base], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    rfa = os.path.join(t, "r.fa")
    synth.write_reads_fasta(rfa, synth.make_reads(contigs, 50, 101, 922)[0])
    sam = os.path.join(t, "o.sam")
    r = subprocess.run([CLI, "-f", "-x", base, "-U", rfa, "-S", sam] + list(opts), stderr=subprocess.PIPE, timeout=300)
    assert r.returncode != 0
    msg = r.stderr.decode()
    assert "1 <= -k <= 128" in msg and "--max-seeds <= 256" in msg, msg
    assert not os.path.exists(sam) or not SL.body_lines(sam)
