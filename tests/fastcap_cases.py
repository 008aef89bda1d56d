"""Planted inputs that drive the fast pass (hisat2_amd/csrc/h2g_fast.h) to every capacity of its compact state: one seeded genome of about 1 Mbp with planted
copies, and reads / pairs over it that each carry a label (family, parameter, variant).  tests/test_fast_caps_cpu.py runs them through tests/emul/h2g_fastcap_check
and asserts which capacity windows they reach; tests/test_gpu_fast_caps.py runs the same units on the device.

The genome is made twice over the same bases: for a linear index, and with a variant set for a SNP-graph index (reads then come from the alternate haplotype).
Inside a planted family the variants are single-base ones at the same offsets of every copy, so that the copies stay copies on either haplotype.

A unit is a dict: label, group ("reads" | "pairs" | "reads_relaxed"), r1, r2 (codes 0..4; r2 None for a read)."""
import numpy as np

from hisat2_amd import synth

SEED = 20261
RDLEN = 101
RELAXED = ("--score-min", "L,0,-0.3")          # 101 bases: -30.3, five mismatches of 6 align, and the pass holds four edits
FULL_C = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 40]
FLANK_C = [2, 3, 4, 5, 6, 7, 8, 9]
LOCAL_C = [2, 3, 4, 5, 6, 7]
TANDEM_C = [2, 3, 4, 5, 6]
CHIMERA_S = [2, 3, 4, 5, 6, 7, 8]
GROUPS = ("reads", "reads_relaxed", "pairs")


def rc(r):
    r = np.asarray(r, dtype=np.uint8)[::-1].copy()
    m = r < 4
    r[m] = 3 - r[m]
    return r


class Genome:
    """ref: the contigs; alt: the alternate haplotype (None on a linear case); pos(ci, p): where reference position p of contig ci lies on the haplotype reads
    are taken from"""
    def __init__(self, ref, snps=None):
        self.ref, self.snps = ref, snps
        self.hap = ref
        self.maps = None
        if snps:
            self.hap = synth.apply_snps(ref, snps)
            self.maps = []
            for ci, g in enumerate(ref):
                shift = np.zeros(len(g) + 1, dtype=np.int64)
                for _, typ, chrom, p, data in snps:
                    if chrom != f"chr{ci + 1}":
                        continue
                    if typ == "deletion":
                        d = int(data)
                        shift[p + 1:p + d] -= np.arange(1, d)       # the deleted bases all land on the base behind them
                        shift[p + d:] -= d
                    elif typ == "insertion":
                        shift[p:] += len(data)
                self.maps.append(np.arange(len(g) + 1) + shift)

    def take(self, ci, p, n):
        q = int(self.maps[ci][p]) if self.maps else p
        r = self.hap[ci][q:q + n]
        assert len(r) == n, (ci, p, n)
        return np.array(r, dtype=np.uint8)


def _plant(rng, g, regions, at, seg):
    g[at:at + len(seg)] = seg
    regions.append((at, at + len(seg)))


def make_genome(graph):
    """-> (Genome, plan): plan[family][parameter] = what the read builders need (positions of the copies)"""
    rng = np.random.default_rng(SEED)
    g = rng.integers(0, 4, size=900000).astype(np.uint8)
    g2 = rng.integers(0, 4, size=100000).astype(np.uint8)
    regions, plan, fam_regions = [], {"full": {}, "flank": {}, "local": {}, "tandem": {}, "micro": []}, []
    cur = 20000
    for c in FULL_C:                                       # a 300-base segment, c copies 4 kb apart
        seg = rng.integers(0, 4, size=300).astype(np.uint8)
        at = [cur + 4000 * k for k in range(c)]
        for a in at:
            _plant(rng, g, regions, a, seg)
        fam_regions.append((at, 300))
        plan["full"][c] = at
        cur = at[-1] + 6000
    for c in FLANK_C:                                      # a 45-base core, c copies 1 kb apart, every copy inside flanks of its own
        core = rng.integers(0, 4, size=45).astype(np.uint8)
        at = [cur + 1000 * k for k in range(c)]
        for a in at:
            _plant(rng, g, regions, a, core)
        fam_regions.append((at, 45))
        plan["flank"][c] = at
        cur = at[-1] + 3000
    for c in LOCAL_C:                                      # a 30-base core, c copies inside 3 kb
        core = rng.integers(0, 4, size=30).astype(np.uint8)
        step = 2600 // c
        at = [cur + step * k for k in range(c)]
        for a in at:
            _plant(rng, g, regions, a, core)
        fam_regions.append((at, 30))
        plan["local"][c] = at
        cur = at[-1] + 5000
    for c in TANDEM_C:                                     # a 120-base segment, c copies 350 apart
        seg = rng.integers(0, 4, size=120).astype(np.uint8)
        at = [cur + 350 * k for k in range(c)]
        for a in at:
            _plant(rng, g, regions, a, seg)
        fam_regions.append((at, 120))
        plan["tandem"][c] = at
        cur = at[-1] + 5000
    plan["duo"] = []
    for inst in range(8):                                  # 30-base cores in two copies 700 apart: long partial hits that are no anchors
        core = rng.integers(0, 4, size=30).astype(np.uint8)
        for a in (cur, cur + 700):
            _plant(rng, g, regions, a, core)
        fam_regions.append(([cur, cur + 700], 30))
        plan["duo"].append(cur)
        cur += 2000
    plan["pairs4"] = []
    for inst in range(4):                                  # two 105-base segments, each twice in tandem 110 apart: 2 x 2 alignments, every combination concordant
        s1, s2 = rng.integers(0, 4, size=105).astype(np.uint8), rng.integers(0, 4, size=105).astype(np.uint8)
        for k, seg in enumerate((s1, s1, s2, s2)):
            _plant(rng, g, regions, cur + 110 * k, seg)
        fam_regions.append(([cur, cur + 110], 105))
        fam_regions.append(([cur + 220, cur + 330], 105))
        plan["pairs4"].append(cur)
        cur += 3000
    for unit in ([0, 1], [0, 2, 3], [0], [1, 3, 3, 2]):    # microsatellites of 400 bases: low-complexity reads
        seg = np.resize(np.array(unit, dtype=np.uint8), 400)
        _plant(rng, g, regions, cur, seg)
        plan["micro"].append(cur)
        cur += 3000
    plan["unique_from"] = cur + 5000                       # chr1 from here on and all of chr2: nothing planted
    g2[50000:50300] = 4                                    # an N run: reads that lie across it, and across the seam of the two contigs, straddle two texts
    plan["ngap"] = (50000, 50300)
    ref = [g, g2]
    snps = None
    if graph:
        inside = np.zeros(len(g), dtype=bool)
        for a, b in regions:
            inside[max(0, a - 20):b + 20] = True
        snps = [s for s in synth.make_snps(ref, SEED + 1, every=200) if not (s[2] == "chr1" and inside[s[3]])]
        sid = 10 ** 6
        for at, n in fam_regions:                           # one single-base variant per 60 bases, at the same offsets of every copy (one per 13 bases in the families of many copies, and the graph builder does not finish)
            for off in range(17, n - 12, 60):
                alt = "ACGT"[(int(g[at[0] + off]) + 1 + off % 3) & 3]
                for a in at:
                    sid += 1
                    snps.append((f"rs{sid}", "single", "chr1", a + off, alt))
        snps.sort(key=lambda s: (s[2], s[3]))
    return Genome(ref, snps), plan


def _subst(rng, r, k, lo=0, hi=None, avoid=()):
    """k substitutions at seeded distinct positions of [lo, hi) outside `avoid` (a set of positions)"""
    r = r.copy()
    hi = len(r) if hi is None else hi
    cand = np.array([p for p in range(lo, hi) if p not in avoid])
    for p in rng.choice(cand, size=k, replace=False):
        r[p] = (int(r[p]) + int(rng.integers(1, 4))) & 3
    return r


def _mirror_subs(r, subs):
    """the substitutions at the same distances from the read's other end"""
    r = r.copy()
    for q in subs:
        q = len(r) - 1 - q
        r[q] = (int(r[q]) + 1 + q % 3) & 3
    return r


def make_units(G, plan):
    """-> list of units; every read in both orientations (variant ends in '+' or '-'), every pair as fr and as its mirror"""
    rng = np.random.default_rng(SEED + 2)
    U = []

    def read(label, r, group="reads"):
        for s, x in (("+", r), ("-", rc(r))):
            U.append(dict(label=(label[0], label[1], label[2] + s), group=group, r1=x, r2=None))

    def pair(label, a, b):
        """a: the upstream mate as it lies on the forward strand, b: the downstream one (forward strand too)"""
        U.append(dict(label=(label[0], label[1], label[2] + "+"), group="pairs", r1=a, r2=rc(b)))
        U.append(dict(label=(label[0], label[1], label[2] + "-"), group="pairs", r1=rc(b), r2=a))

    uq = plan["unique_from"]

    def unique_pos(n=RDLEN, ci=None):
        if ci is None:
            ci = int(rng.integers(0, 2))
        lo = uq if ci == 0 else 500
        while True:
            p = int(rng.integers(lo, len(G.ref[ci]) - n - 2000))
            if ci == 0 or p + n + 600 < plan["ngap"][0] or p > plan["ngap"][1] + 100:      # (clear of the N run, pairs' second mates included)
                return ci, p

    # full copies: windows of the 300-base segment, plain and with substitutions
    for c, at in plan["full"].items():
        offs = list(range(0, 200, 8))
        for o in offs:
            read(("full", c, "s0"), G.take(0, at[o % c] + o, RDLEN))
        if c <= 4:
            for k in (1, 2):
                for o in offs:
                    read(("full", c, f"s{k}"), _subst(rng, G.take(0, at[o % c] + o, RDLEN), k))
        if c in (2, 3, 4):
            for o in offs:                                 # a copy that carries more substitutions than the minimum score allows next to a clean one: searched, not reported
                read(("full", c, "s5"), _subst(rng, G.take(0, at[0] + o, RDLEN), 5, 30, 101))
    # flank-unique cores: the read covers the core and 28 bases of the copy's own flanks
    for c, at in plan["flank"].items():
        for k, a in enumerate(at):
            for sh in (-6, 0, 6):
                r = G.take(0, a - 28 + sh, RDLEN)
                read(("flank", c, "s0"), r)
                read(("flank", c, "s2"), _subst(rng, r, 2, avoid=set(range(28 - sh, 28 - sh + 45))))
                # the substitutions right next to the core: a search that starts inside the core ends there with every copy in its range
                lo = 28 - sh
                read(("flank", c, "adj"), _subst(rng, r, 2, avoid=set(range(RDLEN)) - {lo - 1, lo + 45}))
    # the core of a flank-unique family at the read's end, then bases that match nowhere / a unique segment from elsewhere
    for c, at in plan["flank"].items():
        for rep in range(12 if c in (3, 4) else 6):
            core = G.take(0, at[0], 45)
            read(("corejunk", c, "junk"), np.concatenate([rng.integers(0, 4, size=RDLEN - 45).astype(np.uint8), core]))
            ci, p = unique_pos()
            read(("corejunk", c, "chimera"), np.concatenate([G.take(ci, p, RDLEN - 45), core]))
    # local-window cores
    for c, at in plan["local"].items():
        for k, a in enumerate(at):
            for sh in (-10, -5, 0, 5, 10):
                r = G.take(0, a - 36 + sh, RDLEN)
                read(("local", c, "s0"), r)
                read(("local", c, "s3"), _subst(rng, r, 3, avoid=set(range(36 - sh, 36 - sh + 30))))
    # a remainder that matches twice inside one local-index window: 60 unique bases, then the 30-base core and bases that follow it nowhere
    for c, at in plan["local"].items():
        for a in at[:2]:
            for sh in (0, 5, 10):
                r = np.concatenate([G.take(0, a - 60 + sh, 60 - sh + 30), rng.integers(0, 4, size=RDLEN - 90 + sh).astype(np.uint8)])
                read(("localtwice", c, "s0"), r[:RDLEN])
    # tandem copies, reads and pairs
    for c, at in plan["tandem"].items():
        for o in range(0, 20, 2):
            read(("tandem", c, "s0"), G.take(0, at[o % c] + o, RDLEN))
        for o in range(0, 20, 2):
            a = at[o % c] - 150 - o                            # the first mate on unique sequence in front of the array, the second inside a copy
            pair(("tandempair", c, "s0"), G.take(0, a, RDLEN), G.take(0, at[o % c] + (o % 19), RDLEN))
            pair(("tandemboth", c, "s0"), G.take(0, at[0] + o % 19, RDLEN), G.take(0, at[c - 1] + (o % 19), RDLEN))
    # chimeras of s unique segments
    for s in CHIMERA_S:
        for rep in range(16):
            cuts = np.linspace(0, 128 if s >= 7 else RDLEN, s + 1).astype(int)
            parts = []
            for i in range(s):
                ci, p = unique_pos()
                parts.append(G.take(ci, p, int(cuts[i + 1] - cuts[i])))
            read(("chimera", s, "s0"), np.concatenate(parts))
    for s in (3, 4, 5, 6):                                 # ... of 128 bases, and pairs of chimeras: long partial hits of four strands share the pool
        for rep in range(12):
            cuts = np.linspace(0, 128, s + 1).astype(int)
            read(("chimera128", s, "s0"), np.concatenate([G.take(*unique_pos(), int(cuts[i + 1] - cuts[i])) for i in range(s)]))
    for s in (2, 3):
        for rep in range(12):
            cuts = np.linspace(0, RDLEN, s + 1).astype(int)
            a, b = [np.concatenate([G.take(*unique_pos(), int(cuts[i + 1] - cuts[i])) for i in range(s)]) for _ in range(2)]
            pair(("chimerapair", s, "both"), a, b)
            ci, p = unique_pos(400)
            pair(("chimerapair", s, "one"), a, G.take(ci, p, RDLEN))
    # chains of two-copy cores: every partial search leaves a long hit that is no anchor, on both strands
    def chain(n):
        """n two-copy cores with bases that match nowhere in front of, between and behind them"""
        pick = rng.choice(len(plan["duo"]), size=n, replace=False)
        L = 128 if n == 4 else RDLEN
        gap = (L - 30 * n) // (n + 1)
        r = []
        for k in pick:
            r += [rng.integers(0, 4, size=gap).astype(np.uint8), G.take(0, plan["duo"][int(k)], 30)]
        r.append(rng.integers(0, 4, size=L - 30 * n - gap * n).astype(np.uint8))
        return np.concatenate(r)
    for n in (2, 3, 4):
        for rep in range(16):
            read(("corechain", n, "s0"), chain(n))
    # ... and chains of unique segments too short to stop a strand's search as anchors
    for n, seg in ((3, 17), (3, 20), (4, 17), (3, 15)):
        for rep in range(20):
            gap = (RDLEN - seg * n) // (n + 1)
            r = []
            for k in range(n):
                r += [rng.integers(0, 4, size=gap).astype(np.uint8), G.take(*unique_pos(), seg)]
            r.append(rng.integers(0, 4, size=RDLEN - seg * n - gap * n).astype(np.uint8))
            read(("shortchain", n * 100 + seg, "s0"), np.concatenate(r))
    # ... contiguous, on the four strands of a pair: every fresh strand leaves one hit, then the best strand is searched to its end
    for n, seg in ((3, 17), (3, 20), (2, 17), (3, 14)):
        for rep in range(16):
            a, b = [np.concatenate([G.take(*unique_pos(), seg) for k in range(n)]) for _ in range(2)]
            pair(("shortpair", n * 100 + seg, "s0"), a, b)
    for n, m in ((2, 2), (3, 2), (3, 3)):                  # ... and on the four strands of a pair
        for rep in range(12):                             # (how the four strands' searches interleave decides how many long hits wait at once: a few in a hundred fill the pool)
            pair(("chainpair", n * 10 + m, "s0"), chain(n), chain(m))
    # reads that match nowhere: the most partial searches a read of 128 bases can make
    for rep in range(12):
        read(("junk", 128, "s0"), rng.integers(0, 4, size=128).astype(np.uint8))
    # reads inside the 1024 bases that two neighbouring local indexes share, with clustered substitutions in front of the anchor
    for k in range(7, 16):
        z = k * 56320
        for off, subs in ((20, (40, 43)), (300, (38, 41, 44)), (600, (58, 61)), (880, (30, 33))):
            r = G.take(0, z + off, RDLEN)
            for q in subs:
                r[q] = (int(r[q]) + 1 + q % 3) & 3
            read(("overlap", k, "c%d" % len(subs)), r)
            read(("overlap", k, "r%d" % len(subs)), _mirror_subs(G.take(0, z + off, RDLEN), subs))
    # k substitutions on unique sequence, under the default minimum score and under the relaxed one
    for k in range(0, 7):
        for rep in range(40 if k in (4, 5) else 14):
            ci, p = unique_pos()
            r = _subst(rng, G.take(ci, p, RDLEN), k, 3, RDLEN - 3)
            read(("subst", k, "default"), r)
            read(("subst", k, "relaxed"), r, group="reads_relaxed")
    # evenly spaced substitutions: every partial search ends at the next one, k + 1 long hits of one locus on a strand
    for k in (4, 5, 6, 7):
        for rep in range(20):
            ci, p = unique_pos()
            r = G.take(ci, p, RDLEN)
            step = RDLEN // (k + 1)
            for i in range(1, k + 1):
                q = i * step + int(rng.integers(-1, 2))
                r[q] = (int(r[q]) + int(rng.integers(1, 4))) & 3
            read(("evensub", k, "default"), r)
    # one insertion or deletion
    for rep in range(16):
        ci, p = unique_pos()
        r = G.take(ci, p, RDLEN + 3)
        at = int(rng.integers(25, 75))
        n = 1 + rep % 3
        read(("indel", n, "del"), np.concatenate([r[:at], r[at + n:]])[:RDLEN])
        read(("indel", n, "ins"), np.concatenate([r[:at], rng.integers(0, 4, size=n).astype(np.uint8), r[at:]])[:RDLEN])
    # the lengths at the ends of the pass's range
    for n in (31, 32, 128, 129):
        for rep in range(12):
            ci, p = unique_pos(n)
            read(("length", n, "s0"), G.take(ci, p, n))
            if rep < 6:
                read(("length", n, "s1"), _subst(rng, G.take(ci, p, n), 1))
    # one N
    for rep in range(12):
        ci, p = unique_pos()
        r = G.take(ci, p, RDLEN)
        r[[2, 50, 98][rep % 3]] = 4
        read(("n", 1, "s0"), r)
    # reads that hang off a contig end
    for ci in (0, 1):
        L = len(G.hap[ci])
        for hang in (1, 3, 10, 30):
            junk = rng.integers(0, 4, size=hang).astype(np.uint8)
            read(("hang", hang, "left"), np.concatenate([junk, np.array(G.hap[ci][:RDLEN - hang], dtype=np.uint8)]))
            read(("hang", hang, "right"), np.concatenate([np.array(G.hap[ci][L - (RDLEN - hang):], dtype=np.uint8), junk]))
    # reads across the seam of chr1 and chr2 and across the N run of chr2
    for left in (20, 35, 50, 66, 81):
        read(("straddle", left, "seam"), np.concatenate([np.array(G.hap[0][len(G.hap[0]) - left:], dtype=np.uint8), np.array(G.hap[1][:RDLEN - left], dtype=np.uint8)]))
        a, b = plan["ngap"]
        read(("straddle", left, "nrun"), np.concatenate([G.take(1, a - left, left), G.take(1, b, RDLEN - left)]))
    # low-complexity reads
    for mi, a in enumerate(plan["micro"]):
        for o in (0, 50, 150, 290):
            read(("micro", mi, "inside"), G.take(0, a + o, RDLEN))
        for o in (-60, -30, 330, 360):
            read(("micro", mi, "edge"), G.take(0, a + o, RDLEN))
    # pairs: plain, with substitutions, and with a second mate that needs rescue (5 to 8 substitutions)
    for rep in range(40):
        ci, p = unique_pos(400)
        a, b = G.take(ci, p, RDLEN), G.take(ci, p + 200 + rep % 40, RDLEN)
        pair(("pair", 0, "s0"), a, b)
        pair(("pair", 1, "s1"), _subst(rng, a, 1), _subst(rng, b, 1))
        pair(("pair", 5 + rep % 4, "rescue"), a, _subst(rng, b, 5 + rep % 4))
    # pairs with both mates inside full copies: c x c candidate pairs, of which the concordant ones count
    for c in (1, 2, 3):
        at = plan["full"][c]
        for o in range(0, 60, 4):
            pair(("fullpair", c, "s0"), G.take(0, at[o % c] + o, RDLEN), G.take(0, at[o % c] + 199 - o, RDLEN))
    for a in plan["pairs4"]:
        for o in range(5):
            pair(("pairs4", 4, "s0"), G.take(0, a + o, RDLEN), G.take(0, a + 220 + 4 - o, RDLEN))
    # ... and with the upstream mate in front of a flank-unique array whose cores the second mate covers
    for c in (2, 3, 4, 5):
        at = plan["flank"][c]
        for k, a in enumerate(at):
            for sh in (0, 6):
                pair(("flankpair", c, "s0"), G.take(0, a - 250 + sh, RDLEN), G.take(0, a - 28 + sh, RDLEN))
    # more reads of four and five substitutions under the relaxed minimum score: roots searched until the list of seven is full, and beyond
    for k in (4, 5):
        for rep in range(60):
            ci, p = unique_pos()
            read(("subst", k, "relaxed2"), _subst(rng, G.take(ci, p, RDLEN), k, 3, RDLEN - 3), group="reads_relaxed")
    return U


def text_of(r):
    return "".join("ACGTN"[int(x)] for x in r)


def case(graph):
    """-> (Genome, units): the whole case of one index kind"""
    G, plan = make_genome(graph)
    return G, make_units(G, plan)


def write_genome(G, d):
    """g.fa (and g.snp) in directory d -> the hisat2-build arguments behind the program's name"""
    import os
    fa = os.path.join(d, "g.fa")
    synth.write_fasta(fa, G.ref)
    if G.snps:
        synth.write_snps(os.path.join(d, "g.snp"), G.snps)
        return ["-q", "--snp", os.path.join(d, "g.snp"), fa, os.path.join(d, "g")]
    return ["-q", fa, os.path.join(d, "g")]
