#!/usr/bin/env python3
"""Development fuzzer for the paired go() (host instantiation) vs the real reference binary."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import pe_sink as PS  # noqa: E402
import sam_util as SU  # noqa: E402
from h2gemu_py import Emu, flat_reads  # noqa: E402
from hisat2_amd import synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")


DP = int(os.environ.get("H2G_FUZZ_DP", "0"))   # --bowtie2-dp for both sides
OPTS = ()   # extra reference command-line options (scoring / reporting), applied to both sides
SNPS = int(os.environ.get("H2G_FUZZ_SNPS", "0"))   # > 0: graph index with a seeded variant every ~SNPS bp, pairs from the alt haplotype


def flatten(m):
    """(codes, offsets) of an (n, L) array or of a list of read arrays of any lengths"""
    if isinstance(m, np.ndarray) and m.ndim == 2:
        return synth.flatten_reads(m)
    return flat_reads(m)


def write_fasta_reads(path, m, quals=None):
    """FASTA, or FASTQ when quals (flat phred+33 bytes over the reads' offsets) is given"""
    off = 0
    with open(path, "wb") as f:
        for i in range(len(m)):
            s = synth._ALPHA[np.asarray(m[i])].tobytes()
            f.write((b">%d\n" % i + s + b"\n") if quals is None else (b"@%d\n" % i + s + b"\n+\n" + quals[off:off + len(s)].tobytes() + b"\n"))
            off += len(s)


def emu_pairs(base, m1, m2, q1, q2, quals=None, options=None):
    """quals = (flat phred+33 bytes of the first mates, of the second mates): FASTQ pairs; options: the reference's options of the case (default: OPTS)"""
    options = OPTS if options is None else options
    e = Emu(base)
    e.L.h2gemu_set_bowtie2_dp(e.h, DP)
    if options:
        from h2gemu_align import set_options
        set_options(e, DP, options)
    e.load_reads(m1, None if quals is None else quals[0])
    if quals is not None:
        assert np.size(quals[1]) == sum(len(r) for r in m2)
        e.set_mate_quals(quals[1])
    return e.align_pairs(m2, q1, q2)


def parse_pe_sam(path):
    names, recs = [], {}
    for line in open(path):
        if line.startswith("@"):
            if line.startswith("@SQ"):
                names.append(line.split("\t")[1][3:])
            continue
        t = line.rstrip("\n").split("\t")
        a = None
        for x in t[11:]:
            if x.startswith("AS:i:"):
                a = int(x[5:])
        recs.setdefault(t[0], []).append((int(t[1]), t[2], int(t[3]), t[5], a))
    return names, recs


def _flip(m1, m2):      # every 4th mate 2 reverse-complemented: same-strand pairs => discordant (YT:Z:DP)
    m2 = m2.copy()
    m2[::4] = np.where(m2[::4, ::-1] < 4, 3 - m2[::4, ::-1], 4)
    return m1, m2


def _nmask(m1, m2):     # N-filtered mates: the other mate goes through initRead (mate 2: rightendonly, hi_aligner.h:3993); N tails
    m1 = m1.copy(); m2 = m2.copy()
    m1[::3] = 4
    m2[1::7] = 4
    m1[5::11, 50:] = 4
    return m1, m2


MUTATORS = {"flip": _flip, "nmask": _nmask}


def run_case(seed, npairs=0, rdlen=0, sub=0.0, lens=(300000, 120000, 60000), repeats=6, gaps=2, frag_mean=300, frag_sd=30, verbose=6,
             backend=None, stride=16, mutate=None, genome=None, pairs=None, info=None, variants=None, extra=(), quals=None, ref_timeout=None, base=None):
    """genome = (records, names) with pairs = (mate 1 list, mate 2 list): a prepared case instead of lens= / npairs= / rdlen=; variants = a
    synth.write_snps list for a graph index of the prepared genome.  info: a dict that receives the reference's records ("want") and the counts
    ("bad", "overflow", "concordant") of the run.  extra: options of this case behind OPTS, for both sides; quals = (flat phred+33 bytes of the
    first mates, of the second mates): FASTQ pairs (prepared cases; the backend gets them as quals=, the options as options=); ref_timeout:
    seconds the reference process may take (subprocess.TimeoutExpired beyond them); base (prepared cases): the genome's index, already built."""
    opts = tuple(OPTS) + tuple(extra)
    tmp = tempfile.mkdtemp(prefix="h2pe")
    if genome is not None:
        fa = os.path.join(tmp, "g.fa")
        synth.write_fasta(fa, genome[0], names=genome[1])
        snp = []
        if variants:
            synth.write_snps(os.path.join(tmp, "g.snp"), variants)
            snp = ["--snp", os.path.join(tmp, "g.snp")]
        if base is None:                # (base: the index of this genome, built by the caller once for many cases)
            base = os.path.join(tmp, "g")
            subprocess.run([os.path.join(REF, "hisat2-build-s"), "-q"] + snp + [fa, base], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        m1, m2 = pairs
        npairs = len(m1)
        return _compare(seed, tmp, base, m1, m2, npairs, verbose, backend, stride, info, f"prepared n {npairs}", graph=bool(variants), opts=opts, quals=quals,
                        ref_timeout=ref_timeout, explicit=bool(extra))
    contigs = synth.make_genome(list(lens), seed, n_gaps=gaps, gap_len=300, repeats=repeats, repeat_len=500)
    fa = os.path.join(tmp, "g.fa")
    synth.write_fasta(fa, contigs)
    base = os.path.join(tmp, "g")
    src = contigs
    if SNPS:
        var = synth.make_snps(contigs, seed + 5, every=SNPS)
        synth.write_snps(os.path.join(tmp, "g.snp"), var)
        subprocess.run([os.path.join(REF, "hisat2-build-s"), "-q", "--snp", os.path.join(tmp, "g.snp"), fa, base], check=True,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        src = synth.apply_snps(contigs, var)
    else:
        subprocess.run([os.path.join(REF, "hisat2-build-s"), "-q", fa, base], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    m1, m2 = synth.make_pairs(src, npairs, rdlen, seed + 1, frag_mean=frag_mean, frag_sd=frag_sd, sub_rate=sub)
    if mutate is not None:   # a name in MUTATORS or a callable (m1, m2) -> (m1, m2)
        m1, m2 = (MUTATORS[mutate] if isinstance(mutate, str) else mutate)(m1, m2)
    return _compare(seed, tmp, base, m1, m2, npairs, verbose, backend, stride, info, f"n {npairs} len {rdlen} sub {sub}", opts=opts, ref_timeout=ref_timeout, explicit=bool(extra))


def _compare(seed, tmp, base, m1, m2, npairs, verbose, backend, stride, info, what, graph=False, opts=None, quals=None, ref_timeout=None, explicit=False):
    OPTS = tuple(globals()["OPTS"]) if opts is None else opts
    f1, f2 = os.path.join(tmp, "r1.fq" if quals else "r1.fa"), os.path.join(tmp, "r2.fq" if quals else "r2.fa")
    write_fasta_reads(f1, m1, None if quals is None else quals[0])
    write_fasta_reads(f2, m2, None if quals is None else quals[1])
    sam = os.path.join(tmp, "ref.sam")
    subprocess.run([os.path.join(REF, "hisat2-align-s"), "-q" if quals else "-f", "-p", "1", "--no-spliced-alignment", "-x", base, "-1", f1, "-2", f2, "-S", sam] + (["--bowtie2-dp", str(DP)] if DP else []) + list(OPTS),
                   check=True, stdout=subprocess.DEVNULL, stderr=open(os.path.join(tmp, "ref.err"), "w"), timeout=ref_timeout)
    refnames, want = parse_pe_sam(sam)
    # -k as the sink sees it (hisat2.cpp:336 default 10, :1891-1907 the presets raise a smaller one, :3903 no -k seen: 5 on a linear index, 10 on a graph)
    saw_k = "-k" in OPTS
    khits = int(OPTS[OPTS.index("-k") + 1]) if saw_k else 10
    if "--sensitive" in OPTS and khits < 10:
        khits, saw_k = 10, True
    elif "--very-sensitive" in OPTS and "--sensitive" not in OPTS and khits < 30:
        khits, saw_k = 30, True
    if not saw_k:
        khits = 10 if SNPS or graph else 5
    secondary = "--secondary" in OPTS
    q = [str(i) for i in range(npairs)]
    kw = {}
    if quals is not None:
        kw["quals"] = quals
    if explicit:                        # (a backend written for OPTS alone keeps its five arguments)
        kw["options"] = OPTS
    outs, r1, r2 = (backend or emu_pairs)(base, m1, m2, q, q, **kw)
    bad = ovf = setbad = 0
    ncon = 0
    gots = {}
    for i in range(npairs):
        got = gots[q[i]] = PS.finish_pair(outs[i], r1, r2, i * (stride if backend else SU.AL_MAX_RESULTS), refnames, (m1[i], m2[i]), khits=khits, secondary=secondary)
        w = want[q[i]]
        ncon += 1 if (w[0][0] & 2) else 0
        ovf += 1 if outs[i].overflow else 0
        if got != w:
            bad += 1
            if sorted(got, key=str) != sorted(w, key=str):
                setbad += 1
            if bad <= verbose:
                print(" pair", i, ("ovf%d" % outs[i].overflow) if outs[i].overflow else "", "\n   GOT ", got, "\n   WANT", w)
    print(f"PE seed {seed} {what}: concordant(ref) {ncon}  mismatching {bad} (set-level {setbad})  overflow {ovf}  tmp {tmp}")
    if info is not None:
        info.update(want=want, got=gots, refnames=refnames, bad=bad, overflow=ovf, concordant=ncon, base=base, tmp=tmp, ref_err=open(os.path.join(tmp, "ref.err")).read())
    return bad, tmp


if __name__ == "__main__":
    a = sys.argv[1:]
    run_case(int(a[0]), int(a[1]), int(a[2]), float(a[3]))
