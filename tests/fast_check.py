"""The fast path of go() (hisat2_amd/csrc/h2g_fast.h) against the general machine, both instantiated on the host (tests/emul):
every read / pair runs through both; what the fast path completes must equal the machine's result bit for bit."""
import os

import numpy as np

from h2gemu_py import Emu

BAIL_REASONS = ["none", "input", "longpool", "subsample", "coords", "nghits", "edits", "depth", "localhits", "gsearch", "nres", "searched",
                "redundant", "mate", "npairs", "partial", "straddle", "other", "indel", "tail", "iedges", "gwalk"]    # == h2g_fast.h FB_* (FB_COUNT entries: tests/test_fast_path_cpu.py checks it)


def fast_check(base, reads1, reads2=None, names=None, quals=None, options=(), variant="", quals2=None, emu=None, spliced=False):
    """-> dict(completed, mismatching, bails {reason: n}, bad [read ids], done flags); quals / quals2: flat phred+33 bytes of reads1 / reads2 (FASTQ).
    emu: an emulator to run on (default: a fresh one of `variant` over `base`).  spliced: h2gemu_fast_check_spl (tests/emul_spl), which adds "spl": per read,
    the machine's result holds a splice edit"""
    e = Emu(base, variant) if emu is None else emu
    if options:
        from h2gemu_align import set_options
        set_options(e, 0, options)
    n = len(reads1)
    e.load_reads(reads1, quals)
    if reads2 is not None and quals2 is not None:
        assert np.size(quals2) == sum(len(r) for r in reads2)
        e.set_mate_quals(quals2)
    stats, bad, done, *spl = e.fast_check(reads2, names, spliced=spliced)
    nbad = int(stats[1])
    r = {"n": n, "completed": int(stats[0]), "mismatching": nbad, "bails": {BAIL_REASONS[k]: int(stats[2 + k]) for k in range(len(BAIL_REASONS)) if stats[2 + k]},
         "bad": [int(x) for x in bad[:min(nbad, 64)]], "done": done}
    if spliced:
        r["spl"] = spl[0]
    return r


def pairs_overflow_check(base, reads1, reads2, slots, ovf_cap):
    """paired go() on the host machine with `slots` record rows per mate and an overflow area of ovf_cap records (MachOut::ovf)
    -> dict(in_area, mismatching, flagged, area_records)"""
    e = Emu(base)
    e.load_reads(reads1)
    stats = e.pairs_overflow_check(reads2, slots, ovf_cap)
    return {"n": len(reads1), "in_area": int(stats[0]), "mismatching": int(stats[1]), "flagged": int(stats[2]), "area_records": int(stats[3])}


if __name__ == "__main__":
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    import bench
    from hisat2_amd import synth
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    mode = sys.argv[2] if len(sys.argv) > 2 else "pairs"
    base, contigs = bench.build_index(os.path.join(ROOT, ".bench_cache"), 4_900_000)
    if mode == "pairs":
        m1, m2 = synth.make_pairs(contigs, n, 101, bench.SEED + 2000, frag_mean=300, frag_sd=30, sub_rate=0.005)
        r = fast_check(base, m1, m2)
    else:
        reads, _ = synth.make_reads(contigs, n, 101, bench.SEED + 1000, sub_rate=0.005)
        r = fast_check(base, reads)
    r.pop("done")
    print(r)
