"""Labelled reads and --fr pairs for the fast pass of SPLICED runs (h2g_fast.h with FG_SPLICED = 1), on fuzz_spliced.make_case's genome with planted
GT..AG introns.  Three classes of 101-base reads:
  (a) wholly inside an exon, at least 20 bases from any junction, in an exon without decoys: the pass should complete these;
  (b) crossing one planted junction or more: the spliced machine's;
  (c) inside a DECOY exon: an exon the known-sites file covers with sites that no read supports, one every DECOY_STEP bases, so that every window the
      machine looks up next to a hit of such a read (8 bases or more wide, hybridSearch_recur's database lookups) holds a site — with the file loaded
      the pass has to hand every one of them on.  A class-(c) read carries at most three substitutions (it aligns end to end: a read with more may be given up
      by nextBWT / align() before any hit is extended, and then nobody looks anything up) and a stretch of 32 bases without one, so it has an anchor.
The known-sites file lists a fraction of the real introns plus the decoys.  Class (a) keeps 20 bases from the junctions because the lookup windows reach
at most 16 bases beyond a hit's end (minK_local + min(minK_local, .) = 16)."""
import numpy as np

import fuzz_spliced as FS

RDLEN = 101
MARGIN = 20
DECOY_STEP = 6
DECOY_LEN = 37          # a decoy's "intron": left end p, right end p + DECOY_LEN (longer than --min-intronlen 20)
A, B, C = 0, 1, 2


class Case:
    pass


def genome(seed, glen=400000, nintrons=400):
    contigs, _, introns = FS.make_case(seed, 1, rdlen=RDLEN, glen=glen, nintrons=nintrons)
    return contigs[0], introns


def _mutate(rng, r, sub, keep32=False):
    for _ in range(200):
        m = rng.random(len(r)) < sub
        if keep32:                                   # at most three substitutions, and a stretch of 32 bases without one
            z = np.flatnonzero(np.concatenate([[True], m, [True]]))
            if m.sum() > 3 or (np.diff(z) - 1).max() < 32:
                continue
        return np.where(m, (r + rng.integers(1, 4, size=len(r))) & 3, r).astype(np.uint8)
    return r.copy()


def _indel(rng, r):
    at, k = int(rng.integers(5, len(r) - 5)), int(rng.integers(1, 3))
    if rng.random() < 0.5:
        return np.concatenate([r[:at], rng.integers(0, 4, size=k, dtype=np.uint8), r[at:]])[:len(r)]
    return np.concatenate([r[:at], r[at + k:], rng.integers(0, 4, size=k, dtype=np.uint8)])[:len(r)]


def make(seed, n_reads, n_pairs, sub=0.005, indel=0.0, shares=(0.6, 0.25, 0.15), known_frac=0.5, glen=400000, nintrons=400, genome_seed=None):
    """-> Case: g (the genome), introns, exons, decoy (bool per exon), sites [(0, left, right, '+')], reads (n, 101) + rlabel, m1 / m2 + plabel"""
    c = Case()
    c.g, c.introns = genome(seed if genome_seed is None else genome_seed, glen, nintrons)     # (the reads' seed is their own: one index serves many cases)
    rng = np.random.default_rng(seed + 4242)                 # the site file, then the reads; the pairs draw from a generator of their own (below): a shorter
    #                                                          case with the same seed is a prefix of a longer one, reads and pairs alike
    g = c.g
    c.exons = [(c.introns[k][1], c.introns[k + 1][0]) for k in range(len(c.introns) - 1)]
    long_enough = [k for k, (e0, e1) in enumerate(c.exons) if e1 - e0 >= RDLEN + 2 * MARGIN + 10]
    c.decoy = np.zeros(len(c.exons), dtype=bool)
    c.decoy[[k for k in long_enough if k % 5 == 2]] = True
    plain = [k for k in long_enough if not c.decoy[k]]
    decoys = [k for k in long_enough if c.decoy[k]]
    sites = [(0, a - 1, b, "+") for a, b in c.introns if rng.random() < known_frac]
    for k in decoys:
        e0, e1 = c.exons[k]
        # left ends every DECOY_STEP bases over [e0 - 33, e1 - 4), right ends over [e0 + 4, e1 + 33): both kinds are dense wherever a window of a read
        # MARGIN bases inside the exon can lie (the ends that fall into the neighbouring introns are harmless)
        for p in range(e0 + 4 - DECOY_LEN, e1 - 4, DECOY_STEP):
            sites.append((0, p, p + DECOY_LEN, "+" if (p // DECOY_STEP) % 2 else "-"))
    c.sites = sites
    keep = np.ones(len(g), dtype=bool)
    for a, b in c.introns:
        keep[a:b] = False
    tx = g[keep]                                             # the transcript: every planted intron removed
    txpos = np.flatnonzero(keep)                             # transcript offset -> genome offset
    jun = np.searchsorted(txpos, [b for _, b in c.introns])  # transcript offsets of the junctions (first base behind each)
    cum = np.cumsum(shares)

    def inside(ks, length):
        while True:
            k = ks[int(rng.integers(0, len(ks)))]
            e0, e1 = c.exons[k]
            if e1 - e0 >= length + 2 * MARGIN:
                return int(rng.integers(e0 + MARGIN, e1 - MARGIN - length + 1))

    def crossing(length):
        j = int(jun[int(rng.integers(1, len(jun) - 1))])
        return j - int(rng.integers(8, length - 8))          # at least 8 bases on either side of the junction

    def finish(r, cls, flip):
        r = _mutate(rng, r, sub, keep32=cls == C)
        if indel > 0 and cls != C and rng.random() < indel * RDLEN:
            r = _indel(rng, r)
        return FS.revcomp(r) if flip else r

    c.reads = np.zeros((n_reads, RDLEN), dtype=np.uint8)
    c.rlabel = np.zeros(n_reads, dtype=np.uint8)
    for i in range(n_reads):
        u = rng.random()
        cls = A if u < cum[0] else B if u < cum[1] else C
        if cls == B:
            s = crossing(RDLEN)
            r = tx[s:s + RDLEN]
        else:
            s = inside(plain if cls == A else decoys, RDLEN)
            r = g[s:s + RDLEN]
        c.reads[i] = finish(r.copy(), cls, rng.random() < 0.5)
        c.rlabel[i] = cls
    rng = np.random.default_rng(seed + 4243)
    c.m1 = np.zeros((n_pairs, RDLEN), dtype=np.uint8)
    c.m2 = np.zeros((n_pairs, RDLEN), dtype=np.uint8)
    c.plabel = np.zeros(n_pairs, dtype=np.uint8)
    for i in range(n_pairs):
        u = rng.random()
        cls = A if u < cum[0] else B if u < cum[1] else C
        if cls == B:                                         # a fragment of the transcript whose first mate crosses a junction
            fl = int(rng.integers(180, 320))
            s = crossing(RDLEN)
            f = tx[s:s + fl]
        else:                                                # the whole fragment inside one exon
            fl = int(rng.integers(RDLEN + 20, 200))
            s = inside(plain if cls == A else decoys, fl)
            f = g[s:s + fl]
        f = f.copy()
        left, right = finish(f[:RDLEN].copy(), cls, False), finish(FS.revcomp(f)[:RDLEN].copy(), cls, False)
        if rng.random() < 0.5:
            c.m1[i], c.m2[i] = left, right
        else:
            c.m1[i], c.m2[i] = right, left
        c.plabel[i] = cls
    return c


def write_sites(path, sites, name="chr1"):
    with open(path, "w") as f:
        for _, l, r, d in sites:
            f.write("%s\t%d\t%d\t%s\n" % (name, l, r, d))
