"""One arm of tests/test_gpu_fast_caps.py on the device (a process of its own: a stream reads its switches from the environment when it is made).
usage: fast_caps_worker.py run   index_base reads_1.txt [reads_2.txt] [opts=<reference options, separated by ';'>]    -> one JSON line
       fast_caps_worker.py sam   ref.sam index_base reads_1.txt [reads_2.txt] [opts=...]                              -> one JSON line
       fast_caps_worker.py reuse index_base reads_1.txt [reads_2.txt]                                                 -> one JSON line

The units (one line of bases per read, tests/fast_caps_util.py; unit i is named "i", as the host program names it) are fed in a seeded shuffle, so that the lanes
of a wave hold units of different families; every id this program prints is the unit's line number.

run:   go() once with the fast pass off (h2g_stream_tune "fast" 0: the general machine alone) and RUNS times with it on; what the fetch returns is compared read
       by read as tests/fast_stress.py does.  The pass's counters come from the first run with the pass on: reads it completed, reads it handed on, and the
       hand-ons by reason (h2g_go_fast_prof, words 48 ..).
sam:   go() with the pass on, rendered as SAM fields by the helpers tests/test_gpu_dense.py uses (sam_util.render_selected, pe_sink.finish_pair), against the
       SAM file the reference aligner wrote for the same units: (flag, rname, pos, cigar, AS) of every line of every unit.
reuse: slot reuse within one launch (reuse(), below)."""
import ctypes as C
import json
import sys

import numpy as np

import fast_stress as FS
from fast_check import BAIL_REASONS
from hisat2_amd import api

RUNS = 3
SHUFFLE_SEED = 977
# reuse: 64 workgroups x the 1 024 slots of a workgroup = 65 536 slots in the launch (tests/test_gpu_fast_caps.py holds the figure to the kernels' sources); three
# times as many units, so that a slot carries three units on average whatever the order in which slots free
REUSE_UNITS = 3 * 65536


def load(fn):
    lut = np.full(256, 4, np.uint8)
    for i, c in enumerate(b"ACGT"):
        lut[c] = i
    return [lut[np.frombuffer(l.strip().encode(), np.uint8)] for l in open(fn)]


def flat(seqs):
    return np.concatenate(seqs + [np.zeros(0, np.uint8)]).astype(np.uint8), np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint32)


def overflowed(res, paired):
    """units of a fetched result (FS.fetch_*: one row of bytes per unit first) whose overflow word is set"""
    off = api.PairResult.overflow.offset if paired else 8          # ReadOut: nres, nselect, overflow
    return int((np.ascontiguousarray(res[0][:, off:off + 4]).view(np.uint32) != 0).sum())


def setup(base, files, opts):
    """-> (index, stream, parameter block, permutation, names, shuffled reads, shuffled mates or None)"""
    s1 = load(files[0])
    s2 = load(files[1]) if len(files) == 2 else None
    n = len(s1)
    perm = np.random.default_rng(SHUFFLE_SEED).permutation(n)
    names = [str(int(i)) for i in perm]
    r1 = [s1[i] for i in perm]
    r2 = [s2[i] for i in perm] if s2 else None
    ix = api.Index(base, device=0)
    st = api.Stream(ix, max_reads=n, max_bases=max(sum(map(len, s1)), sum(map(len, s2 or []))) + 64)
    st.set_reads(*flat(r1)); st.set_read_names(names)
    if r2:
        c2, o2 = flat(r2)
        st.set_mates(c2, o2, names)
    p = st.align_params(); p.no_spliced_alignment = 1
    rest = p.apply_options(list(opts))
    assert not rest, rest
    return ix, st, p, perm, names, r1, r2


def run(base, files, opts):
    ix, st, p, perm, names, r1, r2 = setup(base, files, opts)
    paired, n = r2 is not None, len(r1)
    go = st.align_pairs_run if paired else st.align_run
    fetch = FS.fetch_pairs if paired else FS.fetch_reads
    FS.tune(st, "fast", 0)
    go(p)
    ref = fetch(st, n)
    out = {"n": n, "machine_overflow": int(st.counters().n_overflow) + overflowed(ref, paired)}
    FS.tune(st, "fast", 1)
    go(p)
    c = st.counters()
    v = (C.c_ulonglong * 136)()
    L = api.lib()
    L.h2g_go_fast_prof.argtypes = [C.c_void_p, C.c_void_p]
    assert L.h2g_go_fast_prof(st.h, v) == 0
    out.update(fast=int(c.n_fast), handed_on=int(c.n_fast_bail), overflow=int(c.n_overflow),
               why={BAIL_REASONS[k]: int(v[48 + k]) for k in range(len(BAIL_REASONS)) if v[48 + k]})
    for _ in range(RUNS - 1):                               # the same batch again: what a slot holds from the run before is the read's own state
        go(p)
    got = fetch(st, n)
    out["overflow"] += overflowed(got, paired)
    bad = FS.differing(ref, got, n)
    out["differing"] = len(bad)
    out["first"] = []
    for j in bad[:4]:
        d = FS.describe(ref, got, j)
        d["id"] = int(perm[j])
        out["first"].append(d)
    st.close(); ix.close()
    print(json.dumps(out))


def sam(ref_sam, base, files, opts):
    import sam_util as SU
    ix, st, p, perm, names, r1, r2 = setup(base, files, opts)
    n = len(r1)
    bad, first = [], []
    if r2 is None:
        refnames, want = SU.parse_sam(ref_sam)
        st.align_run(p)
        res, aln = st.align_fetch()
        nover = int((res["overflow"] != 0).sum())
        got = SU.render_selected(res, aln, refnames, r1, names)
        bad = [q for q in names if got[q] != want[q]]
        first = [{"id": int(q), "got": got[q], "want": want[q]} for q in bad[:4]]
    else:
        import fuzz_pairs as F
        import pe_sink as PS
        refnames, want = F.parse_pe_sam(ref_sam)
        st.align_pairs_run(p)
        res, a1, a2 = st.align_pairs_fetch()
        nover = 0
        for j in range(n):
            nover += int(res[j].overflow != 0)
            got = PS.finish_pair(res[j], a1, a2, j * api.PAIR_RES_CAP, refnames, (r1[j], r2[j]), khits=int(p.khits))      # (-k as the sink sees it: 5 on a linear index, 10 on a graph)
            if got != want[names[j]]:
                bad.append(names[j])
                if len(first) < 4:
                    first.append({"id": int(names[j]), "got": got, "want": want[names[j]]})
    c = st.counters()
    st.close(); ix.close()
    print(json.dumps({"n": n, "fast": int(c.n_fast), "overflow": nover, "differing": len(bad), "first": first}, default=str))


def reuse(base, files):
    """Slot reuse: the units tiled by seeded permutations to REUSE_UNITS and more, names distinct per copy, as two resident batches with different permutations.
    h2g_stream_tune "fast_reserve" 192 leaves the fast launch 64 workgroups.  Both batches run with the pass off, then with it on, queued back to back without a
    sync between them; every read of both is compared.  Then each batch runs once more on its own in either arm, for that run's counters."""
    paired = len(files) == 2
    s1 = load(files[0])
    s2 = load(files[1]) if paired else None
    n = len(s1)
    tiles = (REUSE_UNITS + n - 1) // n
    T = tiles * n
    ix = api.Index(base, device=0)
    st = api.Stream(ix, max_reads=T, max_bases=max(sum(map(len, s1)), sum(map(len, s2 or []))) * tiles + 64)
    FS.tune(st, "fast_reserve", 192)
    order = []
    for k in range(2):
        rng = np.random.default_rng(4100 + k)
        idx = np.concatenate([rng.permutation(n) for _ in range(tiles)])
        names = ["%d_%d" % (t // n, i) for t, i in enumerate(idx.tolist())]
        st.select_batch(k)
        st.set_reads(*flat([s1[i] for i in idx])); st.set_read_names(names)
        if paired:
            c2, o2 = flat([s2[i] for i in idx])
            st.set_mates(c2, o2, names)
        order.append(idx)
    p = st.align_params(); p.no_spliced_alignment = 1
    go = st.align_pairs_run if paired else st.align_run
    fetch = FS.fetch_pairs if paired else FS.fetch_reads
    res, counts = {}, {}
    for fast in (0, 1):
        FS.tune(st, "fast", fast)
        for k in range(2):
            st.select_batch(k)
            go(p)
        st.sync()
        res[fast] = []
        for k in range(2):
            st.select_batch(k)
            res[fast].append(fetch(st, T))
        counts[fast] = []
        for k in range(2):                                   # (the counters are those of the run queued last: one run per batch, read before the next)
            st.select_batch(k)
            go(p)
            c = st.counters()
            counts[fast].append({"fast": int(c.n_fast), "handed_on": int(c.n_fast_bail), "overflow": int(c.n_overflow) + overflowed(res[fast][k], paired)})
    out = {"n": n, "units": T, "machine": counts[0], "pass": counts[1], "differing": [], "first": []}
    for k in range(2):
        bad = FS.differing(res[0][k], res[1][k], T)
        out["differing"].append(len(bad))
        for i in bad[:3]:
            d = FS.describe(res[0][k], res[1][k], i)
            d["batch"], d["id"] = k, int(order[k][i])
            out["first"].append(d)
    st.close(); ix.close()
    print(json.dumps(out))


def main():
    mode, args = sys.argv[1], sys.argv[2:]
    opts = ()
    if args and args[-1].startswith("opts="):
        opts = tuple(x for x in args[-1][5:].split(";") if x)
        args = args[:-1]
    if mode == "run":
        run(args[0], args[1:], opts)
    elif mode == "sam":
        sam(args[0], args[1], args[2:], opts)
    elif mode == "reuse":
        reuse(args[0], args[1:])
    else:
        sys.exit("unknown mode " + mode)


if __name__ == "__main__":
    main()
