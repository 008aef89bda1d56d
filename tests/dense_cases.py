"""The in-edge-rich graph fixture `gdense` (tests/gen_golden.py dense): families of repeat copies between unique spacers, SNPs at the SAME element
offsets in every copy (so that a k-mer's node range holds one node per copy, each with extra in-edges), a few copy-private SNPs, and a few short
deletions / insertions.  Everything is seeded; the genome, the variant list and the index are committed, the k-mers and reads are regenerated from
the seeds (tests/test_graph_caps_cpu.py, tests/test_gpu_parity.py)."""
import numpy as np

from hisat2_amd import synth

SEED = 20261019
# (copies, element length): the copy count bounds the node range and the in-edge list of a k-mer of that family
FAMILIES = ((3, 320), (4, 360), (6, 400), (8, 340), (10, 420), (14, 380), (20, 300))
SPACER = (90, 260)
NAME = "chrD"
DIVERGE = 40
MAXROWS = 64          # the row limit handed to the reference probe (ref_probe ... maxrows=64)
N_KMERS = 3000
THIN = 7            # the extend / adjust vectors keep every seventh line of the probe's output
N_READS, N_PAIRS, RDLEN = 2000, 1000, 101


def make_dense_genome(seed=SEED):
    """-> (genome codes, [(family, copy, start, length)])"""
    rng = np.random.default_rng(seed)
    elems = [rng.integers(0, 4, size=L, dtype=np.uint8) for _, L in FAMILIES]
    order = [(f, c) for f, (n, _) in enumerate(FAMILIES) for c in range(n)]
    rng.shuffle(order)
    parts, where, cur = [], [], 0
    for f, c in order:
        sp = rng.integers(0, 4, size=int(rng.integers(*SPACER)), dtype=np.uint8)
        parts.append(sp); cur += len(sp)
        e = elems[f].copy()
        # every copy diverges from its family at a base in DIVERGE: copies identical over hundreds of bases, with SNPs every dozen, make the number
        # of paths the graph builder has to tell apart grow beyond what it indexes
        d = np.nonzero(rng.random(len(e)) < 1.0 / DIVERGE)[0]
        e[d] = (e[d] + rng.integers(1, 4, size=len(d))) & 3
        parts.append(e); where.append((f, c, cur, len(e))); cur += len(e)
    parts.append(rng.integers(0, 4, size=300, dtype=np.uint8))
    return np.concatenate(parts), where


def make_dense_snps(genome, where, seed=SEED + 1):
    """shared SNPs every 10-15 element bases (the same offset and allele in every copy of a family), ~12 copy-private SNPs, 3 deletions and 3 insertions
    of 1-3 bases; never closer than 6 bases -> synth.write_snps records, sorted by position"""
    rng = np.random.default_rng(seed)
    shared = {}
    for f, (_, L) in enumerate(FAMILIES):
        offs, o = [], int(rng.integers(8, 14))
        while o < L - 12:
            offs.append((o, int(rng.integers(1, 4))))
            o += int(rng.integers(10, 16))
        shared[f] = offs
    recs = []
    for f, c, start, L in where:
        for o, sh in shared[f]:
            recs.append((start + o, "single", "ACGT"[(int(genome[start + o]) + sh) & 3]))
    taken = sorted(p for p, _, _ in recs)
    def free(p):
        i = np.searchsorted(taken, p)
        return all(abs(taken[j] - p) >= 6 for j in (i - 1, i) if 0 <= j < len(taken))
    extra = [("single", None)] * 12 + [("deletion", None)] * 3 + [("insertion", None)] * 3
    for typ, _ in extra:
        while True:
            f, c, start, L = where[int(rng.integers(0, len(where)))]
            p = start + int(rng.integers(10, L - 10))
            if free(p):
                break
        if typ == "single":
            recs.append((p, typ, "ACGT"[(int(genome[p]) + int(rng.integers(1, 4))) & 3]))
        elif typ == "deletion":
            recs.append((p, typ, str(int(rng.integers(1, 4)))))
        else:
            recs.append((p, typ, "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=int(rng.integers(1, 4))))))
        taken = sorted(taken + [p])
    recs.sort()
    return [(f"rs{i + 1}", typ, NAME, p, data) for i, (p, typ, data) in enumerate(recs)]


def alt_haplotype(genome, snps):
    return synth.apply_snps([genome], snps, names=[NAME])[0]


def make_kmers(genome, where, snps, n=N_KMERS, seed=SEED + 2):
    """k-mers of 10-24 bases from the element copies of the alternate haplotype (forward strand) -> list of uint8 arrays"""
    rng = np.random.default_rng(seed)
    # positions of the alternate haplotype: shift every element start by the indels before it
    shift = sorted((p, (-int(d) if t == "deletion" else len(d))) for _, t, _, p, d in snps if t != "single")
    alt = alt_haplotype(genome, snps)
    out = []
    while len(out) < n:
        f, c, start, L = where[int(rng.integers(0, len(where)))]
        k = int(rng.integers(10, 25))
        o = int(rng.integers(0, L - k))
        a = start + o + sum(s for p, s in shift if p < start)
        if a < 0 or a + k > len(alt):
            continue
        out.append(alt[a:a + k].copy())
    return out


def write_ragged_fasta(path, reads):
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b">%d\n" % i + synth._ALPHA[r].tobytes() + b"\n")


def make_reads(genome, snps):
    """the 2000 reads of 101 bases and the 1000 pairs from the alternate haplotype -> (reads, mates1, mates2)"""
    alt = alt_haplotype(genome, snps)
    reads, _ = synth.make_reads([alt], N_READS, RDLEN, SEED + 3, sub_rate=0.004)
    m1, m2 = synth.make_pairs([alt], N_PAIRS, RDLEN, SEED + 4, frag_mean=320, frag_sd=60, sub_rate=0.004)
    return reads, m1, m2


# ---- which capacities a coordinate case needs: read from the oracle (pinned to the reference's vectors in tests/test_oracle_golden.py), never from the code under test
CAPS = {          # (H2G_IEDGE_CAP, H2G_GW_MAXELT, H2G_GW_MAXST) of the capacity sets that ship
    "big": (24, 96, 160),      # h2g_go_big.h / h2g_go_xl.h (+ include/h2g.h)
    "gdef": (24, 24, 40),      # h2g_graph.h, include/h2g.h: the default units and the C-ABI primitives
    "gfast": (4, 8, 12),       # h2g_go_fast_graph_caps.h: the graph fast pass
}


def coords_needs(oracle_lib, ix, cases):
    """cases as parity_cases.parse_graph_coords returns them -> [(longest in-edge list, states, elements)] from the oracle's walk of each, after checking that the
    oracle's coordinates are the reference's"""
    import ctypes as C
    import h2o_py as H
    u32 = C.c_uint32
    out = []
    for top, bot, nt, nb, ie, hlen, strad, want in cases:
        buf = (u32 * (2 * max(1, len(ie))))()
        for k, (a, b) in enumerate(ie):
            buf[2 * k], buf[2 * k + 1] = a, b
        co = (H.Coord * 128)()
        nc, st, steps = u32(0), C.c_int(0), u32(0)
        rc = oracle_lib.h2o_genome_coords_graph(ix, top, bot, nt, nb, buf, len(ie), bot - top, hlen, 0, co, C.byref(nc), C.byref(st), C.byref(steps))
        assert rc == 1 and st.value == strad, (top, bot, rc)
        assert [(co[k].tidx, co[k].toff, co[k].joinedOff) for k in range(nc.value)] == want, (top, bot)
        a, b, c = u32(), u32(), u32()
        oracle_lib.h2o_gw_readout(C.byref(a), C.byref(b), C.byref(c))
        out.append((a.value, b.value, c.value))
    return out


def fits(need, caps):
    return need[0] <= caps[0] and need[2] <= caps[1] and need[1] <= caps[2]


def windows(cases, needs):
    """the fixture's conditions: coordinate cases by longest in-edge list and by node range"""
    def count(vals, lo, hi):
        return sum(1 for v in vals if lo <= v <= hi)
    ies = [n[0] for n in needs]
    nodes = [c[3] - c[2] for c in cases]
    return {"ie3_4": count(ies, 3, 4), "ie5_8": count(ies, 5, 8), "ie9_24": count(ies, 9, 24), "ie25up": count(ies, 25, 1 << 30),
            "nodes5_8": count(nodes, 5, 8), "nodes9_24": count(nodes, 9, 24), "nodes25up": count(nodes, 25, 1 << 30)}


# ---- the gdense vectors through a backend with the C ABI's layouts (api.Stream on the device, h2gemu_py.Emu on the host): equal or flagged, flags owed
def load_kmers(golden_dir):
    """-> (flat codes, offsets) of reads_gdense_kmers.fa.gz"""
    import os
    import h2o_py as H
    _, seqs = H.read_fasta_reads(os.path.join(golden_dir, "reads_gdense_kmers.fa.gz"))
    codes = np.concatenate(seqs).astype(np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint32)
    return codes, offs


def check_coords_abi(be, cases, needs, caps, cap=24):
    """be.sa_resolve_graph over the coordinate cases; caps = (H2G_IEDGE_CAP, H2G_GW_MAXELT, H2G_GW_MAXST) of the backend's unit; `cap` coordinates per query
    -> (cases, flagged)"""
    from hisat2_amd import api
    qs, ies = [], []
    for top, bot, nt, nb, ie, hlen, strad, want in cases:
        qs.append(api.GsaQuery(top, bot, nt, nb, bot - top, hlen, 0))
        x = api.IEdges()
        x.n = len(ie)                                        # the true count; the list stores its first H2G_IEDGE_CAP entries
        for k, (a, b) in enumerate(ie[:api.H2G_IEDGE_CAP]):
            x.e[k][0], x.e[k][1] = a, b
        ies.append(x)
    co, res = be.sa_resolve_graph(qs, ies, cap=cap)
    nflag = 0
    for i, ((top, bot, nt, nb, ie, hlen, strad, want), need) in enumerate(zip(cases, needs)):
        flagged = res[i].ok == 0 and res[i].nsteps == 0xFFFFFFFF
        nflag += flagged
        assert not (flagged and fits(need, (caps[0], min(caps[1], cap), caps[2]))), ("flagged although it fits", top, bot, need)
        if not flagged:
            got = [(co[i * cap + k].tidx, co[i * cap + k].toff, co[i * cap + k].joinedOff) for k in range(res[i].ncoords)]
            assert res[i].ok == 1 and res[i].straddled == strad and got == want, (top, bot, need, res[i].ok, res[i].nsteps)
    return len(cases), nflag


def check_psearch_abi(be, golden_dir):
    """be.fm_search_graph over probe_gdense_psearch: every field, the true count of the in-edge list, and its first H2G_IEDGE_CAP entries -> (cases, longer lists)"""
    import h2o_py as H
    from hisat2_amd import api
    qs, want = [], []
    for l in H.glines(golden_dir, "probe_gdense_psearch.txt.gz"):
        f = l.split()
        v = list(map(int, f[:15]))
        qs.append(api.FmQuery(v[0], 0, v[1], 0, 0, 1))
        want.append((v[2:], [tuple(map(int, x.split(":"))) for x in f[16:]]))
    out, ie = be.fm_search_graph(qs, khits=10, kseeds=20)
    nlong = 0
    for o, e, (w, wie), q in zip(out, ie, want, qs):
        assert [getattr(o, f) for f in api.FM_HIT_FIELDS[:13]] == w, (q.read, q.fw, w)
        assert e.n == len(wie) and e.pairs() == wie[:api.H2G_IEDGE_CAP], (q.read, q.fw)
        nlong += len(wie) > api.H2G_IEDGE_CAP
    return len(qs), nlong


def check_extend_abi(be, golden_dir):
    """be.extend over probe_gdense_extend: the reference's extension or the overflow bit, which an extension of at most H2G_MAX_EDITS edits does not owe"""
    import h2o_py as H
    from hisat2_amd import api
    hits, args, want = [], [], []
    for l in H.glines(golden_dir, "probe_gdense_extend.txt.gz"):
        lhs, rhs = l.split(" -> ")
        rid, fw, rdoff, hlen, tidx, toff, joff, mm = map(int, lhs.split())
        h = api.GHit()
        h.read, h.fw, h.rdoff, h.len, h.tidx, h.toff, h.joinedOff = rid, fw, rdoff, hlen, tidx, toff, joff
        hits.append(h)
        args.append(api.ExtArgs(mm, api.MAX, api.MAX))
        want.append(rhs.split())
    out, res = be.extend(hits, args)
    nflag = 0
    for h, r, w in zip(out, res, want):
        if h.overflow:
            nflag += 1
            assert int(w[8]) > 24, ("flagged although it fits", w)          # 24 = H2G_NEW_EDITS of the default units (h2g_graph.h)
            continue
        got = [r.extended, h.rdoff, h.len, h.toff, h.joinedOff, r.leftext, r.rightext, h.score, h.nedits]
        eds = [f"{h.edits[k].pos}:{chr(h.edits[k].chr)}>{chr(h.edits[k].qchr)}:{h.edits[k].type}:{-1 if h.edits[k].snp == api.MAX else h.edits[k].snp}" for k in range(h.nedits)]
        assert got == list(map(int, w[:9])) and eds == w[9:], (got, w)
    return len(hits), nflag


def check_adjust_abi(be, golden_dir, cap=8):
    import parity_cases as PC
    from hisat2_amd import api
    cases = PC.parse_adjust(golden_dir, "probe_gdense_adjust.txt.gz")
    qs = [api.AdjustQuery(c[0], c[1], c[2], c[3], c[4], c[5], c[6]) for c in cases]
    hits, nh = be.adjust_with_alt(qs, cap=cap)
    nflag = 0
    for i, c in enumerate(cases):
        found, want = c[7], c[8]
        if nh[i] == 0xFFFFFFFF:                               # the primitive's capacity flag
            nflag += 1
            assert len(want) > cap or any(w[0][4] > 24 for w in want), ("flagged although it fits", c[:7])
            continue
        assert nh[i] == len(want) and (nh[i] > 0) == bool(found), (c[:7], nh[i])
        got = [([hits[i * cap + k].rdoff, hits[i * cap + k].len, hits[i * cap + k].toff, hits[i * cap + k].joinedOff, hits[i * cap + k].nedits],
                PC.edit_strings_snp(hits[i * cap + k].edits, hits[i * cap + k].nedits)) for k in range(nh[i])]
        assert got == want, (c[:7], got, want)
    return len(cases), nflag
