"""Seeded FRAGMENTED assemblies and the reads that touch their edges (tests only).

Every other genome of the suite has at most three contigs and a handful of N gaps, and its reads keep clear of every contig
end and of every N.  The generators here make the opposite: hundreds of texts (many shorter than a read, a few shorter than
the ftab window), N runs of every small length (also at the very start and the very end of a record, and two runs 12 bases
apart), all-N records that the reference's builder drops (text ids then shift against record order), one repeat element whose
copies sit exactly at contig starts and ends, and read / pair classes that each aim at one edge:

  reads   A interior (control) | B hang off a contig's first / last base by 1-30 random bases | C straddle two texts that are adjacent
          in the joined string (j = 20-80 bases of the first) | D span an N run (1, 2, 3, 5: random bases over the Ns; 50, 300: the
          run cut out, i.e. two fragments of one text that are adjacent in the joined string) | E a whole contig shorter than the read between random flanks | F zero overhang: starts at offset 0 / ends at the
          last base / abuts an N run | G the repeat element, its copies at contig ends included
  pairs   P1 both mates inside one short contig (overlapping / one containing the other / fragment == contig) | P2 mate 2 hangs off
          the contig end | P3 mates on two texts adjacent in the joined string, joined distance < 1000 | P4 mates either side of a 300-N run

Everything is a pure function of the seeds.  Nothing here changes hisat2_amd/synth.py (bench.py and the goldens are built from it).

The reference's builder and aligner take every ingredient listed above; none had to be dropped.  One read shape was moved: a read with random
bases over a whole 50-N run.  The reference aligns a 150-base read of that kind end to end (a reference N costs it nothing in GenomeHit::extend),
which is 50+ edits in one record — more than the 32 a default record holds, so such a read sets overflow bit 1 by design and is the large
workspace's to take.  The cases here assert overflow == 0, so class D cuts the 50-N runs out like the 300-N ones, and the reads across them
(make_nrun_reads) are a case of their own in tests/test_long_edits_cpu.py.

Measured from the reference's own output (tests/golden/gfrag fixture = make_frag_genome(GFRAG_SEED, GFRAG_TOTAL), 1500 reads of
make_frag_reads(seed GFRAG_SEED + 1); the live CPU case = make_frag_genome(LIVE_SEED, LIVE_TOTAL), 3000 reads / 3000 pairs).  The
tests assert at least half of each count (MINIMA below):

  gfrag (183 texts, 57 under 101 bases, 11 under 36; 315 fragments; 134 N runs)        measured   asserted
    coords vectors with straddled = 1 (of 2720)                                           100        50
    coords vectors rejected with rejectStraddle = 1                                        50        25
    extend vectors that stop at a stretch end, FASTA (of 38 900) / FASTQ (of 12 967)   736 / 247   368 / 123
    getLocalGFM probes without a local index (of 1464)                                     549       274
    extsearch vectors with elements (of 4500)                                             3336      1668
    partialSearch vectors that continue from an offset > 0 (of 3000)                      2798      1399
  live case, reads (3000)            class:    A     B     C     D     E     F     G
    generated                                575   584   373   359   285   440   384
    the reference aligns                     568   142     0   274    28   438   383
    ... with a soft clip                             142                28
    asserted: aligned                        284    71          137    14   219   191
    asserted: soft-clipped                            71                14
    class C left unaligned or clipped: 373 of 373 (asserted 186)
  live case, pairs (3000)            class:   P1    P2    P3    P4
    generated                                778   764   706   752
    the reference reports concordant         540   174     0   751
    asserted                                 270    87          375
    P3 not concordant: 706 of 706 (asserted 353)
  command line, --no-temp-splicesite: 44 reads come out spliced over an N run (asserted 22)
"""
import os
import subprocess

import numpy as np

from hisat2_amd import synth

GFRAG_SEED, GFRAG_TOTAL, GFRAG_NREADS = 20261017, 120000, 1500
LIVE_SEED, LIVE_TOTAL, GRAPH_TOTAL = 20261018, 600000, 300000
N_RUNS = (1, 1, 2, 3, 5, 10, 50, 300)
ELEM_LEN = 300
READ_CLASSES = "ABCDEFG"
PAIR_CLASSES = ("P1", "P2", "P3", "P4")


class FragGenome:
    """records: the FASTA records by index (uint8 codes 0..4, all-N records included); texts: indexes of the records the builder keeps
    (text id -> record); runs: (record, start, length) of every N run; copies: (record, start, fw) of every copy of the element"""

    def __init__(self, records, runs, copies, element):
        self.records, self.runs, self.copies, self.element = records, runs, copies, element
        self.texts = [i for i, r in enumerate(records) if (r < 4).any()]
        self.names = [f"chr{i + 1}" for i in range(len(records))]

    def text_names(self):
        return [self.names[i] for i in self.texts]

    def text_seqs(self):
        return [self.records[i] for i in self.texts]


def make_frag_genome(seed, total=GFRAG_TOTAL):
    """~total bases: short contigs of log-uniform length 25..2000 (about 200 per 120 kbp), a few contigs of 3-12 kbp with the N runs of N_RUNS (several of each),
    two all-N records (length 1 first in the file, length 500 in the middle), 10 copies of one 300-base element."""
    rng = np.random.default_rng(seed)
    scale = total / 120000.0
    nlong = max(5, int(round(5 * scale)))
    longs = [rng.integers(0, 4, size=int(rng.integers(3000, 12001)), dtype=np.uint8) for _ in range(nlong)]
    budget = total - sum(len(x) for x in longs)
    shorts = []
    while sum(len(x) for x in shorts) < budget or len(shorts) < 60:
        shorts.append(rng.integers(0, 4, size=int(round(float(np.exp(rng.uniform(np.log(25), np.log(2000)))))), dtype=np.uint8))
    assert sum(1 for s in shorts if len(s) < 101) >= 40 and sum(1 for s in shorts if len(s) < 36) >= 3
    # the element: at the start of three contigs, at the end of three, interior in four; random strand
    element = rng.integers(0, 4, size=ELEM_LEN, dtype=np.uint8)
    hosts = [i for i, s in enumerate(shorts) if len(s) >= 700]
    pick = [int(x) for x in rng.choice(hosts, size=10, replace=False)]
    short_copies = []
    for k, si in enumerate(pick):
        s = shorts[si]
        at = 0 if k < 3 else len(s) - ELEM_LEN if k < 6 else int(rng.integers(40, len(s) - ELEM_LEN - 40))
        fw = bool(rng.integers(0, 2))
        s[at:at + ELEM_LEN] = element if fw else (3 - element[::-1])
        short_copies.append((si, at, fw))
    # N runs of the long contigs: every length of N_RUNS up to four times in each, at least 110 bases apart; long 0 starts and ends with a run, long 1 has two runs 12 bases apart
    long_runs = []
    for li, g in enumerate(longs):
        taken = []

        def put(at, ln):
            g[at:at + ln] = 4
            taken.append((at, ln))
        if li == 0:
            put(0, 10)
            put(len(g) - 5, 5)
        if li == 1:
            put(1000, 3)
            put(1015, 2)            # 12 unambiguous bases between the two: a fragment shorter than the ftab window
        for ln in N_RUNS * 4:
            for _ in range(100):
                at = int(rng.integers(200, len(g) - 200 - ln))
                if all(at + ln + 110 < a or a + l + 110 < at for a, l in taken):
                    put(at, ln)
                    break
        long_runs.append(sorted(taken))
    # record order: all-N (1) first; shorts with the longs spread among them; all-N (500) in the middle
    order = [("s", i) for i in range(len(shorts))]
    for li in range(nlong):
        order.insert(int(rng.integers(1, len(order))), ("l", li))
    order.insert(len(order) // 2, ("n", 500))
    order.insert(0, ("n", 1))
    records, runs, copies = [], [], []
    where = {}
    for kind, i in order:
        where[(kind, i)] = len(records)
        if kind == "n":
            records.append(np.full(i, 4, dtype=np.uint8))
        else:
            records.append(shorts[i] if kind == "s" else longs[i])
    for li, tk in enumerate(long_runs):
        runs += [(where[("l", li)], a, l) for a, l in tk]
    copies = [(where[("s", si)], at, fw) for si, at, fw in short_copies]
    return FragGenome(records, runs, copies, element)


def write_genome(path, genome):
    synth.write_fasta(path, genome.records, names=genome.names)


def _rc(r):
    return np.where(r[::-1] < 4, 3 - r[::-1], 4).astype(np.uint8)


def _rand(rng, n):
    return rng.integers(0, 4, size=n, dtype=np.uint8)


def _clean(genome):
    """records without any N (the short contigs), as (record index, sequence)"""
    return [(i, r) for i, r in enumerate(genome.records) if len(r) and (r < 4).all()]


def _adjacent(genome):
    """(record t, record u): consecutive TEXTS, both free of N — contiguous in the joined string"""
    tx = genome.texts
    return [(a, b) for a, b in zip(tx[:-1], tx[1:]) if (genome.records[a] < 4).all() and (genome.records[b] < 4).all()]


def make_frag_reads(genome, seed, n, lens=(36, 64, 65, 101, 128, 150), classes=READ_CLASSES, sub_rate=0.005, with_origin=False):
    """-> (reads: list of uint8 arrays, labels: list of one-letter classes).  Class C reads are exact (the string is in the index); the
    other classes carry i.i.d. substitutions at sub_rate.  Strand ~ Bernoulli(1/2).  with_origin: a third list, (record, offset of the read's
    first base in the record — negative when it hangs off the start, forward strand?) per read."""
    rng = np.random.default_rng(seed)
    rec = genome.records
    clean = _clean(genome)
    adj = _adjacent(genome)
    longs = sorted({r for r, _, _ in genome.runs})
    reads, labels, origin = [], [], []
    weights = dict(A=0.2, B=0.2, C=0.12, D=0.12, E=0.1, F=0.14, G=0.12)
    w = np.array([weights[c] for c in classes])
    w = w / w.sum()
    cl = None
    while len(reads) < n:
        if cl is None:                                  # a draw that does not fit is redrawn within its class: the class mix is the weights'
            cl = classes[int(rng.choice(len(classes), p=w))]
        L = int(rng.choice(lens))
        r = None
        if cl == "A":
            i, g = clean[int(rng.integers(0, len(clean)))] if rng.random() < 0.7 else (lambda t: (t, rec[t]))(longs[int(rng.integers(0, len(longs)))])
            if len(g) < L + 17:
                continue
            at = int(rng.integers(8, len(g) - L - 8))
            r = g[at:at + L].copy()
            org = (i, at)
            if (r > 3).any():
                continue
        elif cl == "B":
            i, g = clean[int(rng.integers(0, len(clean)))]
            k = int(rng.integers(1, 31))
            if len(g) < L - k or L - k < 20:
                continue
            left = rng.random() < 0.5
            r = np.concatenate([_rand(rng, k), g[:L - k]]) if left else np.concatenate([g[len(g) - (L - k):], _rand(rng, k)])
            org = (i, -k if left else len(g) - (L - k))
        elif cl == "C":
            a, b = adj[int(rng.integers(0, len(adj)))]
            j = int(rng.integers(20, 81))
            if j >= L - 8 or len(rec[a]) < j or len(rec[b]) < L - j:
                continue
            r = np.concatenate([rec[a][len(rec[a]) - j:], rec[b][:L - j]])
            org = (a, len(rec[a]) - j)
        elif cl == "D":
            t, at, ln = genome.runs[int(rng.integers(0, len(genome.runs)))]
            g = rec[t]
            if ln == 10 or at == 0 or at + ln == len(g):
                continue
            cut = ln >= 50
            if cut:                                     # the two flanks joined: fragments of one text, adjacent in the joined string
                j = int(rng.integers(12, L - 11))
                r = np.concatenate([g[at - j:at], g[at + ln:at + ln + L - j]]).copy()
                org = (t, at - j)
            else:
                if ln + 24 > L:
                    continue
                s0 = int(rng.integers(at + ln + 12 - L, at - 11))
                r = g[s0:s0 + L].copy()
                org = (t, s0)
            if len(r) != L:
                continue
            m = r > 3                                   # random bases over every N of the window (a neighbouring run included)
            r[m] = _rand(rng, int(m.sum()))
        elif cl == "E":
            small = [(i, g) for i, g in clean if len(g) < L]
            i, g = small[int(rng.integers(0, len(small)))]
            k = int(rng.integers(0, L - len(g) + 1))
            r = np.concatenate([_rand(rng, k), g, _rand(rng, L - len(g) - k)])
            org = (i, -k)
        elif cl == "F":
            kind = int(rng.integers(0, 4))
            if kind < 2:
                i, g = clean[int(rng.integers(0, len(clean)))]
                if len(g) < L:
                    continue
                r = g[:L].copy() if kind == 0 else g[len(g) - L:].copy()
                org = (i, 0 if kind == 0 else len(g) - L)
            else:
                t, at, ln = genome.runs[int(rng.integers(0, len(genome.runs)))]
                g = rec[t]
                if kind == 2 and at < L:
                    continue
                r = g[at - L:at].copy() if kind == 2 else g[at + ln:at + ln + L].copy()
                org = (t, at - L if kind == 2 else at + ln)
                if len(r) != L or (r > 3).any():
                    continue
        elif cl == "G":
            t, at, _ = genome.copies[int(rng.integers(0, len(genome.copies)))]
            g = rec[t]
            lo, hi = max(0, at - 20), min(len(g) - L, at + ELEM_LEN - L + 20)
            if hi < lo:
                continue
            s0 = int(rng.integers(lo, hi + 1))
            r = g[s0:s0 + L].copy()
            org = (t, s0)
        if cl != "C":
            m = rng.random(len(r)) < sub_rate
            r = np.where(m, (r + rng.integers(1, 4, size=len(r), dtype=np.uint8)) & 3, r).astype(np.uint8)
        fw = rng.random() >= 0.5
        if not fw:
            r = _rc(r)
        reads.append(np.ascontiguousarray(r, dtype=np.uint8))
        labels.append(cl)
        origin.append((org[0], org[1], bool(fw)))
        cl = None
    return (reads, labels, origin) if with_origin else (reads, labels)


def make_frag_pairs(genome, seed, n, rdlen=101, classes=PAIR_CLASSES, sub_rate=0.005, contained=True):
    """-> (mate 1 list, mate 2 list, labels).  --fr pairs: one mate forward at the fragment's left end, the other reverse-complemented at
    its right end; which of the two is mate 1 is random (both strands).  contained=False leaves out the P1 pairs with a 64-base mate inside the other
    (every mate is then rdlen long)."""
    rng = np.random.default_rng(seed)
    rec = genome.records
    clean = _clean(genome)
    adj = _adjacent(genome)
    runs300 = [x for x in genome.runs if x[2] == 300]
    m1, m2, labels = [], [], []
    cl = None
    while len(m1) < n:
        if cl is None:
            cl = classes[int(rng.integers(0, len(classes)))]
        a = b = None                      # a: left mate (forward strand of the text), b: right mate (forward strand; reverse-complemented below)
        if cl == "P1":
            i, g = clean[int(rng.integers(0, len(clean)))]
            if not (rdlen <= len(g) <= 600):
                continue
            kind = int(rng.integers(0, 3 if contained else 2))
            if kind == 0:                 # fragment == contig
                a, b = g[:rdlen], g[len(g) - rdlen:]
            elif kind == 1:               # overlapping mates somewhere inside
                fl = int(rng.integers(rdlen, min(len(g), 2 * rdlen - 1) + 1))
                s0 = int(rng.integers(0, len(g) - fl + 1))
                a, b = g[s0:s0 + rdlen], g[s0 + fl - rdlen:s0 + fl]
            else:                         # the right mate (64 bases) inside the left one
                s0 = int(rng.integers(0, len(g) - rdlen + 1))
                k = int(rng.integers(0, rdlen - 64 + 1))
                a, b = g[s0:s0 + rdlen], g[s0 + k:s0 + k + 64]
        elif cl == "P2":
            i, g = clean[int(rng.integers(0, len(clean)))]
            if len(g) < 2 * rdlen:
                continue
            k = int(rng.integers(1, 31))
            fl = int(rng.integers(rdlen + 20, min(len(g), 450) + 1))
            if rng.random() < 0.5:        # the right mate hangs off the contig's last base
                a = g[len(g) - fl:len(g) - fl + rdlen]
                b = np.concatenate([g[len(g) - (rdlen - k):], _rand(rng, k)])
            else:                         # the left mate hangs off its first base
                a = np.concatenate([_rand(rng, k), g[:rdlen - k]])
                b = g[fl - rdlen:fl]
        elif cl == "P3":
            t, u = adj[int(rng.integers(0, len(adj)))]
            if len(rec[t]) < rdlen or len(rec[u]) < rdlen:
                continue
            da = int(rng.integers(0, min(len(rec[t]) - rdlen, 350) + 1))     # bases of t right of the left mate
            db = int(rng.integers(0, min(len(rec[u]) - rdlen, 350) + 1))     # bases of u left of the right mate
            a = rec[t][len(rec[t]) - da - rdlen:len(rec[t]) - da]
            b = rec[u][db:db + rdlen]
        elif cl == "P4":
            t, at, ln = runs300[int(rng.integers(0, len(runs300)))]
            g = rec[t]
            da, db = int(rng.integers(0, 60)), int(rng.integers(0, 60))
            a = g[at - da - rdlen:at - da]
            b = g[at + ln + db:at + ln + db + rdlen]
            if len(a) != rdlen or len(b) != rdlen or (a > 3).any() or (b > 3).any():
                continue
        a, b = a.copy(), b.copy()
        for arr in (a, b):
            m = rng.random(len(arr)) < sub_rate
            arr[...] = np.where(m, (arr + rng.integers(1, 4, size=len(arr), dtype=np.uint8)) & 3, arr)
        b = _rc(b)
        if rng.random() < 0.5:
            a, b = b, a
        m1.append(np.ascontiguousarray(a, dtype=np.uint8))
        m2.append(np.ascontiguousarray(b, dtype=np.uint8))
        labels.append(cl)
        cl = None
    return m1, m2, labels


def make_nrun_reads(genome, seed, n, run=50, rdlen=150):
    """reads with random bases where the record has a run of `run` Ns, 12+ record bases either side; either strand.  (The reference aligns such a read
    of 150 bases end to end across a 50-N run, 50+ edits in one record; shorter reads across it stay unaligned.)"""
    rng = np.random.default_rng(seed)
    runs = [r for r in genome.runs if r[2] == run]
    reads = []
    while len(reads) < n:
        t, at, ln = runs[int(rng.integers(0, len(runs)))]
        s0 = int(rng.integers(at + ln + 12 - rdlen, at - 11))
        r = genome.records[t][s0:s0 + rdlen].copy()
        m = r > 3
        r[m] = _rand(rng, int(m.sum()))
        reads.append(np.ascontiguousarray(r if rng.random() < 0.5 else _rc(r), dtype=np.uint8))
    return reads


def write_reads(path, reads, quals=None):
    """FASTA, or FASTQ when `quals` (flat phred+33 bytes, same offsets) is given; names 0, 1, 2 ..."""
    txt = [synth._ALPHA[r].tobytes() for r in reads]
    with open(path, "wb") as f:
        off = 0
        for i, s in enumerate(txt):
            if quals is None:
                f.write(b">%d\n" % i + s + b"\n")
            else:
                f.write(b"@%d\n" % i + s + b"\n+\n" + quals[off:off + len(s)].tobytes() + b"\n")
            off += len(s)


def seeded_quals(reads, seed):
    rng = np.random.default_rng(seed)
    n = sum(len(r) for r in reads)
    return (33 + rng.choice(np.array([2, 8, 15, 20, 25, 30, 37, 40], dtype=np.uint8), size=n)).astype(np.uint8)


def build_index(genome, tmp, ref_dir, snp_file=None):
    """FASTA + the reference builder's index under tmp -> index basename"""
    fa = os.path.join(tmp, "g.fa")
    write_genome(fa, genome)
    base = os.path.join(tmp, "g")
    cmd = [os.path.join(ref_dir, "hisat2-build-s"), "-q"] + (["--snp", snp_file] if snp_file else []) + [fa, base]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return base


# at least half of every count measured from the reference's output (see the table in the module docstring)
MINIMA = dict(
    # gfrag vectors (the reference's classes through oracle/ref_probe.cpp)
    coords_straddled=50, coords_rejected=25, extend_stop_at_stretch_end=368, extend_stop_at_stretch_end_fq=123, localof_absent=274,
    extsearch_with_elements=1668, psearch_continued=1399,
    # the C oracle over every row of gfrag (it is held to the vectors above first): straddling queries, rejected queries; the fused seed stage
    sa_straddled=6486, sa_rejected=3194, seed_anchored=660, seed_straddled=24)


def live_case():
    """the live CPU / GPU case: (genome, reads, read labels, mate 1 list, mate 2 list, pair labels), cached"""
    if not _LIVE:
        g = make_frag_genome(LIVE_SEED, LIVE_TOTAL)
        reads, labels = make_frag_reads(g, LIVE_SEED + 1, 3000)
        m1, m2, plabels = make_frag_pairs(g, LIVE_SEED + 2, 3000)
        _LIVE.append((g, reads, labels, m1, m2, plabels))
    return _LIVE[0]


_LIVE = []


def read_teeth(want, labels):
    """from the reference's SAM records alone: {aligned_X: reads of class X it aligns, clipped_B / clipped_E: aligned reads with a soft clip,
    c_unaligned_or_clipped: class C reads it leaves unaligned or clips}"""
    t = {}
    for c in sorted(set(labels)):
        idx = [i for i, l in enumerate(labels) if l == c]
        al = [i for i in idx if want[str(i)][0][0] != 4]
        t["aligned_" + c] = len(al)
        if c in "BE":
            t["clipped_" + c] = sum(1 for i in al if "S" in want[str(i)][0][3])
        if c == "C":
            t["c_unaligned_or_clipped"] = sum(1 for i in idx if want[str(i)][0][0] == 4 or "S" in want[str(i)][0][3])
    return t


def pair_teeth(want, labels):
    """{concordant_X: pairs of class X the reference reports as concordant, p3_not_concordant}"""
    t = {}
    for c in sorted(set(labels)):
        idx = [i for i, l in enumerate(labels) if l == c]
        t["concordant_" + c] = sum(1 for i in idx if want[str(i)][0][0] & 2)
        if c == "P3":
            t["p3_not_concordant"] = sum(1 for i in idx if not want[str(i)][0][0] & 2)
    return t


def assert_teeth(measured, minima):
    print("teeth:", measured)
    for k, v in minima.items():
        assert measured.get(k, 0) >= v, (k, measured.get(k, 0), v)


# half of what the reference's own output shows on live_case() (the table in the module docstring)
LIVE_READ_MINIMA = dict(aligned_A=284, aligned_B=71, clipped_B=71, c_unaligned_or_clipped=186, aligned_D=137, aligned_E=14, clipped_E=14, aligned_F=219, aligned_G=191)
LIVE_PAIR_MINIMA = dict(concordant_P1=270, concordant_P2=87, p3_not_concordant=353, concordant_P4=375)


def make_frag_snps(genome, seed):
    """-> (variants as synth.write_snps takes them, the alternate-haplotype FragGenome).  synth.make_snps keeps 50 bases clear of every contig end and 6 of
    every N, and skips contigs under 200 bases; these variants do the opposite: single-base variants 0-4 bases from the first and the last base of every
    text of 40+ bases and 1-5 bases from both sides of N runs, plus one in the middle of the text.  Single-base only: the alternate haplotype keeps every
    coordinate, so the read generators work on it unchanged."""
    rng = np.random.default_rng(seed)
    out, alt = [], [r.copy() for r in genome.records]
    runs_of = {}
    for t, at, ln in genome.runs:
        runs_of.setdefault(t, []).append((at, ln))
    for t in genome.texts:
        g = genome.records[t]
        if len(g) < 40:
            continue
        pos = {int(rng.integers(0, 5)), len(g) - 1 - int(rng.integers(0, 5)), len(g) // 2}
        for at, ln in runs_of.get(t, []):
            pos |= {at - 1 - int(rng.integers(0, 5)), at + ln + int(rng.integers(0, 5))}
        last = -100
        for p in sorted(pos):
            if p < 0 or p >= len(g) or g[p] > 3 or p - last < 12:
                continue
            last = p
            a = (int(g[p]) + int(rng.integers(1, 4))) & 3
            out.append((f"rs{len(out) + 1}", "single", genome.names[t], p, "ACGT"[a]))
            alt[t][p] = a
    return out, FragGenome(alt, genome.runs, genome.copies, genome.element)
