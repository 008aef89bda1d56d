"""Seeded TRIMMED read sets (tests only): every length from 0 to 300 in one batch, mates of different lengths, empty reads.

Every other case of the suite fixes one read length per batch (the fragmented-assembly set mixes six, unpaired), and no pair has mates of two lengths.  Adapter- and
quality-trimmed input is the opposite, and a uniform batch cannot reach what it reaches: a fast-pass lane that takes a read of another length next, the entry range of
fast_begin (32..128 bases per mate, both mates), the partial last word of the packed form (16 bases per word), the read-length thresholds of the machine (minK,
minK + 2, minK_local = 8, ftabChars, len < 2), the 256-row cap of the SwAligner path, and the batch-level sizes taken from the longest read of a batch.

Reads and pairs are drawn at 150 bases (300 for lengths above 150) with synth.make_reads / make_pairs and each read or mate is cut on its own to a drawn length;
80 % of the cuts keep the 5' end, 20 % the 3' end.  Length classes (length_classes(); minK and ftabChars come from the index, index_params()):

  Z  0, 1                     filtered by length (YF:Z:LN)
  T  2, 3, 7, 8, 9, ftabChars - 1 .. ftabChars + 1, minK - 1 .. minK + 3, 20, 24
  W  31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 111, 112, 113, 127, 128      the fast pass's range and the packed form's word edges
  L  129, 150, 200, 255, 256
  X  257, 300                 beyond the 256 rows of the SwAligner path: kept out of every --bowtie2-dp case (such a read is flagged by design)

Pair classes: R1 both mates in 32..128, unequal | R2 one mate <= 128 (class W), the other >= 129 | R3 one mate < 32 (class T) | R4 one mate in Z | R5 both mates in Z |
R6 equal lengths (control).  Which mate is the longer one is a coin flip.

The last read / pair of a set is never empty: the reference's FASTA parser drops an empty LAST record (and then aborts on -1/-2 with "fewer reads in file specified
with -1"); its FASTQ parser takes empty records anywhere.  Everything is a pure function of the seeds.

Measured from the reference's own output (hisat2-align-s -p 1 --no-spliced-alignment) on live_case(): genome make_genome(LIVE_SEED), 4000 reads, 3000 pairs.  The tests
assert at least half of each count (READ_MINIMA / PAIR_MINIMA / GOLDEN_MINIMA below) and the exact number of length-filtered lines, which follows from the inputs:

  live case, reads (4000)                       class:     Z      T      W      L      X     YF:Z:LN lines
    the reference aligns, linear index                       0    232   1674    718    322     236   (= reads under 2 bases; generated: Z 236, T 935, W 1775, L 729, X 325)
    ... SNP graph, reads from the alternate haplotype        0    234   1658    715    322
    ... --bowtie2-dp 2 --score-min L,0,-3 (no class X)       0    274   1956    775
    asserted (linear / graph / --bowtie2-dp 2)                    116 / 117 / 137   837 / 829 / 978   359 / 357 / 387   161 / 161
  live case, pairs (3000)                       class:    R1     R2     R3     R4     R5     R6     YF:Z:LN lines
    concordant in the reference, linear index              467    439    292      0      0    433    1484   (= mates under 2 bases; generated: 500, 533, 500, 508, 488, 471)
    ... SNP graph                                          465    440    285      0      0    430
    pairs with an aligned mate, linear / graph                                 364 / 361   0
    asserted: concordant (linear / graph)            233 / 232   219 / 220   146 / 142                216 / 215
    asserted: R4 with an aligned mate (linear / graph)                        182 / 180
    (R5: both mates are filtered by length; its tooth is the YF:Z:LN count)
  spliced case (fuzz_spliced.make_case at 150 bases, every read cut; --no-temp-splicesite), 3000 reads: 478 spliced in the reference (asserted 239)
  golden (tests/golden/ragged_*, index g1): 2000 reads, 1570 aligned (asserted 785), 101 YF:Z:LN lines; 1500 pairs, 843 concordant (asserted 421), 734 YF:Z:LN lines
"""
import os
import subprocess

import numpy as np

from hisat2_amd import synth

LIVE_SEED = 20261101
LIVE_LENS = (300000, 120000, 60000)
GOLDEN_SEED, GOLDEN_NREADS, GOLDEN_NPAIRS = 20261102, 2000, 1500
READ_CLASSES = "ZTWLX"
PAIR_CLASSES = ("R1", "R2", "R3", "R4", "R5", "R6")
FAST_MIN, FAST_MAX = 32, 128        # what fast_begin admits per mate (h2g_fast.h)


def index_params(base):
    """(minK, ftabChars) of a built index, read by the C oracle's loader (no device)"""
    import h2o_py as H
    ix = H.load_index(H.load(), base).contents
    return int(ix.minK), int(ix.g.p.ftabChars)


def length_classes(minK, ftab_chars, classes=READ_CLASSES):
    c = dict(Z=[0, 1],
             T=sorted({2, 3, 7, 8, 9, 20, 24} | set(range(ftab_chars - 1, ftab_chars + 2)) | set(range(minK - 1, minK + 4))),
             W=[31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 111, 112, 113, 127, 128],
             L=[129, 150, 200, 255, 256],
             X=[257, 300])
    assert all(2 <= x < 31 for x in c["T"]), c["T"]
    return {k: c[k] for k in classes}


def make_genome(seed, lens=LIVE_LENS):
    return synth.make_genome(list(lens), seed, n_gaps=2, gap_len=300, repeats=6, repeat_len=500)


def build_index(contigs, tmp, ref_dir, variants=None, name="g"):
    fa = os.path.join(tmp, name + ".fa")
    synth.write_fasta(fa, contigs)
    base = os.path.join(tmp, name)
    snp = []
    if variants:
        synth.write_snps(os.path.join(tmp, name + ".snp"), variants)
        snp = ["--snp", os.path.join(tmp, name + ".snp")]
    subprocess.run([os.path.join(ref_dir, "hisat2-build-s"), "-q"] + snp + [fa, base], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return base


def cut(rng, r, length):
    """80 %: the first `length` bases (3' trimming); 20 %: the last ones"""
    r = r[:length] if rng.random() < 0.8 else r[len(r) - length:]
    return np.ascontiguousarray(r, dtype=np.uint8)


_READ_WEIGHTS = dict(Z=0.06, T=0.24, W=0.45, L=0.17, X=0.08)


def make_ragged_reads(contigs, seed, n, minK, ftab_chars, classes=READ_CLASSES, sub=0.01, indel=0.001, nrate=0.0005):
    """-> (reads: list of uint8 arrays, labels: one class letter per read)"""
    rng = np.random.default_rng(seed)
    lc = length_classes(minK, ftab_chars, classes)
    w = np.array([_READ_WEIGHTS[c] for c in classes])
    short, _ = synth.make_reads(contigs, n, 150, seed + 1, sub_rate=sub, indel_rate=indel, n_rate=nrate)
    long_, _ = synth.make_reads(contigs, n, 300, seed + 2, sub_rate=sub, indel_rate=indel, n_rate=nrate)
    reads, labels = [], []
    for i in range(n):
        cl = classes[int(rng.choice(len(classes), p=w / w.sum()))]
        if i == n - 1 and cl == "Z":
            cl = "W"                                 # (an empty last FASTA record is dropped by the reference's parser)
        length = int(rng.choice(lc[cl]))
        reads.append(cut(rng, long_[i] if length > 150 else short[i], length))
        labels.append(cl)
    return reads, labels


def make_ragged_pairs(contigs, seed, n, minK, ftab_chars, classes=PAIR_CLASSES, sub=0.01):
    """-> (mate 1 list, mate 2 list, labels)"""
    rng = np.random.default_rng(seed)
    lc = length_classes(minK, ftab_chars)
    s1, s2 = synth.make_pairs(contigs, n, 150, seed + 1, frag_mean=300, frag_sd=40, sub_rate=sub)
    l1, l2 = synth.make_pairs(contigs, n, 300, seed + 2, frag_mean=420, frag_sd=50, sub_rate=sub)
    pick = lambda cls: int(rng.choice(sum((lc[c] for c in cls), [])))       # noqa: E731
    w32 = [x for x in lc["W"] if x >= FAST_MIN]
    m1, m2, labels = [], [], []
    for i in range(n):
        cl = classes[int(rng.integers(0, len(classes)))]
        if i == n - 1 and cl in ("R4", "R5"):
            cl = "R1"
        if cl == "R1":
            a, b = (int(x) for x in rng.choice(w32, size=2, replace=False))
        elif cl == "R2":
            a, b = int(rng.choice(w32)), pick("LX")
        elif cl == "R3":
            a, b = pick("T"), pick("WL")
        elif cl == "R4":
            a, b = pick("Z"), pick("TWL")
        elif cl == "R5":
            a, b = pick("Z"), pick("Z")
        else:
            a = b = int(rng.choice(lc["W"] + [150]))
        if rng.random() < 0.5:
            a, b = b, a
        big = max(a, b) > 150
        m1.append(cut(rng, (l1 if big else s1)[i], a))
        m2.append(cut(rng, (l2 if big else s2)[i], b))
        labels.append(cl)
    return m1, m2, labels


def trim_reads(reads, seed, lengths):
    """every read of a uniform set cut to a length drawn from `lengths` (those that fit), the last one never to fewer than 2 bases -> (list, lengths drawn)"""
    rng = np.random.default_rng(seed)
    out = []
    for i, r in enumerate(reads):
        fit = [x for x in lengths if x <= len(r) and (i < len(reads) - 1 or x >= 2)]
        out.append(cut(rng, np.asarray(r), int(rng.choice(fit))))
    return out, [len(r) for r in out]


def seeded_quals(reads, seed):
    """flat phred+33 bytes over the reads' offsets"""
    rng = np.random.default_rng(seed)
    n = sum(len(r) for r in reads)
    return (33 + rng.choice(np.array([2, 8, 15, 20, 25, 30, 37, 40], dtype=np.uint8), size=n)).astype(np.uint8)


def write_reads(path, reads, quals=None, names=None):
    """FASTA, or FASTQ when `quals` (flat phred+33 bytes, same offsets) is given; names 0, 1, 2 ... unless given.  An empty last record has no place in a FASTA file
    (the reference's parser drops it): the generators never make one, and this refuses to write one."""
    assert quals is not None or len(reads[-1]) > 0, "an empty last FASTA record"
    with open(path, "wb") as f:
        off = 0
        for i, r in enumerate(reads):
            s = synth._ALPHA[r].tobytes()
            nm = names[i].encode() if names else b"%d" % i
            if quals is None:
                f.write(b">" + nm + b"\n" + s + b"\n")
            else:
                f.write(b"@" + nm + b"\n" + s + b"\n+\n" + quals[off:off + len(s)].tobytes() + b"\n")
            off += len(s)


def n_length_filtered(*read_lists):
    """reads / mates of fewer than 2 bases: each is one YF:Z:LN line and two warnings on stderr"""
    return sum(1 for reads in read_lists for r in reads if len(r) < 2)


def length_warnings(units):
    """the reference's stderr lines ahead of its summary (hisat2.cpp:3017-3052, :3417-3432): two warnings per read or mate of fewer than 2 bases, the first
    message for every such mate of a record and then the second.  units: per record [(name, length)] for an unpaired read, [(name 1, length 1), (name 2,
    length 2)] for a pair -> the lines, without their newlines"""
    out = []
    for mates in units:
        who = lambda k, nm: f"mate #{k + 1} of read '{nm}'" if len(mates) == 2 else f"read '{nm}'"      # noqa: E731
        short = [(k, nm, ln) for k, (nm, ln) in enumerate(mates) if ln < 2]
        out += [f"Warning: skipping {who(k, nm)} because length ({ln}) <= # seed mismatches (0)" for k, nm, ln in short]
        out += [f"Warning: skipping {who(k, nm)} because it was < 2 characters long" for k, nm, ln in short]
    return out


def fast_ineligible(reads1, reads2=None):
    """units the fast pass cannot enter by construction: a mate outside 32..128 bases or with an N -> boolean array"""
    def out(r):
        return not (FAST_MIN <= len(r) <= FAST_MAX) or bool((np.asarray(r) > 3).any())
    bad = np.array([out(r) for r in reads1], dtype=bool)
    if reads2 is not None:
        bad |= np.array([out(r) for r in reads2], dtype=bool)
    return bad


def read_teeth(want, labels):
    """from the reference's SAM records: {aligned_X: reads of class X it aligns}"""
    t = {}
    for c in sorted(set(labels)):
        t["aligned_" + c] = sum(1 for i, l in enumerate(labels) if l == c and want[str(i)][0][0] != 4)
    return t


def pair_teeth(want, labels):
    """{concordant_X: pairs of class X reported concordant, aligned_X: pairs of class X with an aligned mate}"""
    t = {}
    for c in sorted(set(labels)):
        idx = [i for i, l in enumerate(labels) if l == c]
        t["concordant_" + c] = sum(1 for i in idx if want[str(i)][0][0] & 2)
        t["aligned_" + c] = sum(1 for i in idx if any(not (r[0] & 4) for r in want[str(i)]))
    return t


def ln_lines(sam_path):
    import gzip
    op = gzip.open if str(sam_path).endswith(".gz") else open
    with op(sam_path, "rt") as f:
        return sum(1 for l in f if not l.startswith("@") and "\tYF:Z:LN" in l)


def assert_teeth(measured, minima):
    print("teeth:", measured)
    for k, v in minima.items():
        assert measured.get(k, 0) >= v, (k, measured.get(k, 0), v)


_LIVE = {}


def live_case(ref_dir, tmp, snps=False, nreads=4000, npairs=3000, classes=READ_CLASSES):
    """-> dict(contigs, variants, base, minK, ftabChars, reads, labels, m1, m2, plabels): the live CPU / GPU case; the index, the reads and the pairs are each made
    once per process.  With snps the index is a SNP graph (a variant about every 200 bases) and the reads come from the alternate haplotype."""
    snps = bool(snps)
    if ("index", snps) not in _LIVE:
        contigs = make_genome(LIVE_SEED + (7 if snps else 0))
        variants = synth.make_snps(contigs, LIVE_SEED + 5, every=200) if snps else None
        base = build_index(contigs, tmp, ref_dir, variants, name="ragged_g" if snps else "ragged")
        minK, ftab = index_params(base)
        _LIVE[("index", snps)] = dict(contigs=contigs, variants=variants, base=base, minK=minK, ftabChars=ftab, src=synth.apply_snps(contigs, variants) if snps else contigs)
    ix = _LIVE[("index", snps)]
    if ("reads", snps, nreads, classes) not in _LIVE:
        _LIVE[("reads", snps, nreads, classes)] = make_ragged_reads(ix["src"], LIVE_SEED + 10, nreads, ix["minK"], ix["ftabChars"], classes=classes)
    if ("pairs", snps, npairs) not in _LIVE:
        _LIVE[("pairs", snps, npairs)] = make_ragged_pairs(ix["src"], LIVE_SEED + 20, npairs, ix["minK"], ix["ftabChars"])
    reads, labels = _LIVE[("reads", snps, nreads, classes)]
    m1, m2, plabels = _LIVE[("pairs", snps, npairs)]
    return dict(ix, reads=reads, labels=labels, m1=m1, m2=m2, plabels=plabels)


def genome_arg(contigs):
    """(records, names) as fuzz_align.run_case / fuzz_pairs.run_case take a prepared genome"""
    return contigs, [f"chr{i + 1}" for i in range(len(contigs))]


# half of what the reference's own output shows (the table in the module docstring)
READ_MINIMA = dict(plain=dict(aligned_T=116, aligned_W=837, aligned_L=359, aligned_X=161),
                    dp=dict(aligned_T=137, aligned_W=978, aligned_L=387),
                    snps=dict(aligned_T=117, aligned_W=829, aligned_L=357, aligned_X=161))
PAIR_MINIMA = dict(plain=dict(concordant_R1=233, concordant_R2=219, concordant_R3=146, aligned_R4=182, concordant_R6=216),
                   snps=dict(concordant_R1=232, concordant_R2=220, concordant_R3=142, aligned_R4=180, concordant_R6=215))
SPLICED_MINIMUM = 239
GOLDEN_MINIMA = dict(aligned_reads=785, concordant_pairs=421)
