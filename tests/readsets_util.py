"""Read sets for the record-stream tests (tests/test_gpu_readsets.py, the tests/golden/readsets_* fixtures): reads drawn from the golden genome g1, with random
reads for the unaligned side and mates drawn from far-apart places for the non-concordant side, written as FASTA, FASTQ, tab5, tab6 and QSEQ; and the rule by
which `hisat2 --un / --al / --un-conc / --al-conc / --al-conc-disc` sorts reads, applied to SAM lines."""
import gzip
import os

import numpy as np

COMP = str.maketrans("ACGTN", "TGCAN")


def load_genome(golden_dir):
    seqs, cur = [], []
    with gzip.open(os.path.join(golden_dir, "g1.fa.gz"), "rt") as f:
        for line in f:
            if line.startswith(">"):
                if cur:
                    seqs.append("".join(cur))
                cur = []
            else:
                cur.append(line.strip().upper())
    if cur:
        seqs.append("".join(cur))
    return [s for s in seqs if len(s) > 2000]


def revcomp(s):
    return s.translate(COMP)[::-1]


def mutate(rng, s, rate):
    a = list(s)
    for i in np.nonzero(rng.random(len(a)) < rate)[0]:
        a[i] = "ACGT"[int(rng.integers(0, 4))]
    return "".join(a)


def quals(rng, n):
    return "".join(chr(int(q)) for q in rng.integers(40, 74, size=n))


def make_records(genome, seed, n, pair_frac=0.5, rdlen=100, random_frac=0.2, far_frac=0.2, sub=0.01, name="r"):
    """n records: (name, seq1, qual1) or (name, seq1, qual1, seq2, qual2).  Of the reads / pairs, `random_frac` are random sequence (they do not align), and of the
    pairs `far_frac` have mates from far-apart places (they align, not concordantly)."""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        g = genome[int(rng.integers(0, len(genome)))]
        paired = rng.random() < pair_frac
        kind = rng.random()
        rand = lambda: "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=rdlen))
        if not paired:
            p = int(rng.integers(0, len(g) - rdlen))
            s = rand() if kind < random_frac else mutate(rng, g[p:p + rdlen], sub)
            if rng.random() < 0.5:
                s = revcomp(s)
            recs.append((f"{name}{i}", s, quals(rng, rdlen)))
            continue
        frag = int(rng.integers(rdlen + 20, 400))
        p = int(rng.integers(0, len(g) - frag))
        s1, s2 = g[p:p + rdlen], revcomp(g[p + frag - rdlen:p + frag])
        if kind < random_frac:
            s1, s2 = rand(), rand()
        elif kind < random_frac + far_frac:
            p2 = (p + len(g) // 2) % (len(g) - rdlen)
            s2 = revcomp(g[p2:p2 + rdlen])
        elif kind < random_frac + far_frac + 0.1:
            s2 = rand()                                  # one mate aligns
        s1, s2 = mutate(rng, s1, sub), mutate(rng, s2, sub)
        if rng.random() < 0.5:
            s1, s2 = s2, s1
        recs.append((f"{name}{i}", s1, quals(rng, rdlen), s2, quals(rng, rdlen)))
    return recs


def spliced_records(genome, seed, n, njunctions=40, rdlen=100, name="s"):
    """n records (unpaired reads and pairs, half each) whose first read crosses one of `njunctions` GT..AG introns, many reads per intron and some with a short
    anchor on one side: with temporary splice sites, whether such a read aligns across the intron depends on the reads before it"""
    rng = np.random.default_rng(seed)
    junctions = []
    while len(junctions) < njunctions:
        ci = int(rng.integers(0, len(genome)))
        g = genome[ci]
        d = g.find("GT", int(rng.integers(200, len(g) - 3000)))
        a = g.find("AG", d + int(rng.integers(150, 1500))) if d > 0 else -1
        if d < 200 or a < 0 or a + 400 > len(g) or "N" in g[d - 200:a + 400]:
            continue
        junctions.append((ci, d, a + 2))                  # the intron is g[d:a + 2]
    recs = []
    for i in range(n):
        ci, d, a = junctions[int(rng.integers(0, njunctions))]
        g = genome[ci]
        left = int(rng.integers(6, rdlen - 6)) if rng.random() < 0.7 else int(rng.choice([6, 8, 10, rdlen - 10, rdlen - 8, rdlen - 6]))
        s1 = mutate(rng, g[d - left:d] + g[a:a + rdlen - left], 0.005)
        if rng.random() < 0.5:
            recs.append((f"{name}{i}", s1, quals(rng, rdlen)))
        else:
            p2 = a + rdlen - left + int(rng.integers(20, 150))
            recs.append((f"{name}{i}", s1, quals(rng, rdlen), revcomp(g[p2:p2 + rdlen]), quals(rng, rdlen)))
    return recs


def repeated_pairs(genome, n, rdlen=100, name="rep"):
    """pairs whose first mate occurs 2 to 10 times in the genome (which of its equal alignments is reported is the PRNG's choice)"""
    from collections import defaultdict
    at = defaultdict(list)
    for ci, s in enumerate(genome):
        for i in range(0, len(s) - rdlen - 300):
            at[s[i:i + rdlen]].append((ci, i))
    out = []
    for k, v in at.items():
        if "N" in k or not 2 <= len(v) <= 10:
            continue
        ci, i = v[0]
        m2 = genome[ci][i + 200:i + 200 + rdlen]
        if i % 25 == 0 and "N" not in m2:                # (neighbouring windows of one repeat are the same case)
            out.append((f"{name}{len(out)}", k, "I" * rdlen, revcomp(m2), "H" * rdlen))
        if len(out) == n:
            break
    return out


def golden_inputs(genome):
    """the inputs of tests/golden/readsets_pe_in_{1,2}.fq.gz (160 pairs) and readsets_tab_in.tab5.gz (200 records, about half of them pairs); the other
    readsets_* files there are what the reference's wrapper script wrote for them with --un --al --un-conc --al-conc --al-conc-disc (-p 1 --no-spliced-alignment)"""
    return make_records(genome, 77, 160, pair_frac=1.0, name="p"), make_records(genome, 78, 200, pair_frac=0.5, name="t")


def write_tabbed(path, recs, six=False):
    with open(path, "w") as f:
        for r in recs:
            if len(r) == 3:
                f.write("\t".join(r) + "\n")
            elif six:
                f.write("\t".join((r[0], r[1], r[2], r[0] + "_mate", r[3], r[4])) + "\n")
            else:
                f.write("\t".join(r) + "\n")


def write_fastx(path, reads, fasta=False):
    """reads: (name, seq, qual)"""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "wt") as f:
        for nm, s, q in reads:
            f.write(f">{nm}\n{s}\n" if fasta else f"@{nm}\n{s}\n+\n{q}\n")


def qseq_name(i, mate):
    return f"M{i % 3}_12_{i % 8}_{1101 + i % 60}_{(i * 7919) % 20000}_{i}_0/{mate}"


def write_qseq(path, reads, mate, filt):
    """reads: (seq, qual) per record; name from qseq_name; filt[i] is the filter character"""
    with open(path, "w") as f:
        for i, (s, q) in enumerate(reads):
            head = qseq_name(i, mate).split("/")[0].split("_")
            f.write("\t".join(head + [str(mate), s.replace("N", "."), q, filt[i]]) + "\n")


def sort_by_flags(sam_lines, originals):
    """The wrapper script's rule.  sam_lines: the SAM body in read order; originals: per record, in the same order, the original text of the unpaired read
    (text,) or of the two mates (text1, text2).  Returns {kind: [bytes of file 1, bytes of file 2]}."""
    out = {k: ["", ""] for k in ("un", "al", "un-conc", "al-conc", "al-conc-disc")}
    it = iter(originals)
    cur, seen = None, 0
    for line in sam_lines:
        fl = int(line.split("\t")[1])
        if fl & 256:
            continue
        m1, m2 = bool(fl & 64), bool(fl & 128)
        if not m1 and not m2:
            cur = next(it)
            out["un" if fl & 4 else "al"][0] += cur[0]
            continue
        if seen == 0:
            cur = next(it)
        seen = (seen + 1) % 2
        m = 0 if m1 else 1
        out["al-conc" if fl & 2 else "un-conc"][m] += cur[m]
        if not (fl & 4) or not (fl & 8):
            out["al-conc-disc"][m] += cur[m]
    return out
