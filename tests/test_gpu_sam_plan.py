"""Plain SAM lines planned on the device (include/h2g.h: h2g_sam_text_unpaired_planned / h2g_sam_text_paired_planned; k_sam_plan_*, k_sam_plan_scatter, k_sam_plan_place
of csrc/h2g_kernels.hip over the planner of csrc/h2g_sam_plan.h), the handed-on reads by the host planner, merged on the device: the text must equal
h2g_sam_format_*_compact on the same fetch byte for byte, with line_offs, line_ends (those of the whole host plan), the handle's summary, its collected sites, and class
bytes equal to the predicate restated in tests/sam_split_util.py.  The calls' refusals launch and count nothing."""
import ctypes as C
import os

import numpy as np
import pytest

import h2o_py as H
import sam_lines as SL
import sam_plan_util as PU
import sam_split_util as SU
import test_gpu_sam_text as T
from hisat2_amd import api, synth

pytestmark = pytest.mark.gpu
vp, sz = C.c_void_p, C.c_size_t
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")


def _raw(a):
    return a.tobytes() if isinstance(a, np.ndarray) else bytes(a)


def _check_planned(st, L, base, paired, sets, fetch, khits, opts=(), keep=False, setup=None, have_db=False):
    """format (one handle), the whole host plan (another: its line_ends) and the planned text (a third) on the fetch the stream holds -> dict"""
    hs = [T._handle(L, base, opts) for _ in range(3)]
    if setup:
        for h in hs:
            setup(L, h)
    hf, hw, hp = hs
    if paired:
        s1, s2 = sets
        res, r1, b1, r2, b2 = fetch
        n = len(b1) - 1
        want = T._format_paired(L, hf, s1, s2, n, res, r1, b1, r2, b2, khits)
        _, _, ends_w = api.sam_plan_paired(hw.value, *s1, *s2, res, r1, b1, r2, b2, khits)
        got, offs, ends = st.sam_text_paired_planned(hp.value, *s1, *s2, res, r1, b1, r2, b2, khits)
    else:
        s1, = sets
        res, r1, b1 = fetch
        n = len(b1) - 1
        want = T._format_unpaired(L, hf, s1, n, res, r1, b1)
        _, _, ends_w = api.sam_plan_unpaired(hw.value, *s1, res, r1, b1)
        got, offs, ends = st.sam_text_unpaired_planned(hp.value, *s1, res, r1, b1)
    if got != want:                                        # the first line that differs, field by field: (column, planned, format call)
        x, y = next((x, y) for x, y in zip(got.split(b"\n"), want.split(b"\n")) if x != y)
        raise AssertionError((x.split(b"\t")[:9], [(k, f, g) for k, (f, g) in enumerate(zip(x.split(b"\t"), y.split(b"\t"))) if f != g], len(got), len(want)))
    if len(want):
        T._check_offs(got, offs)
    assert (ends == ends_w).all() and (n == 0 or int(ends[-1]) == len(offs) - 1)
    assert PU.summary(L, hf) == PU.summary(L, hp)
    assert PU.novel_text(L, hf) == PU.novel_text(L, hp) and PU.take_novel(L, hf) == PU.take_novel(L, hp)
    stats, cls = st.sam_plan_stats(n)
    nalts, nrefs = SU.index_facts(base)
    o = SU.Opts(nalts, nrefs, discordant="--no-discordant" not in opts, mixed="--no-mixed" not in opts, have_db=have_db)
    if paired:
        rows = (api.PairResult * max(n, 1)).from_buffer_copy(_raw(res)[:max(n, 1) * C.sizeof(api.PairResult)].ljust(C.sizeof(api.PairResult), b"\0"))
        pred, why = SU.predicate_paired(rows, _raw(r1), b1, _raw(r2), b2, n, o)
    else:
        rows = (api.ReadResult * max(n, 1)).from_buffer_copy(_raw(res)[:max(n, 1) * C.sizeof(api.ReadResult)].ljust(C.sizeof(api.ReadResult), b"\0"))
        pred, why = SU.predicate_unpaired(rows, _raw(r1), b1, n, o)
    assert list(cls) == pred, next((i, cls[i], pred[i], why[i]) for i in range(n) if cls[i] != pred[i])
    assert stats.device_planned == sum(1 for c in pred if c) and stats.device_planned + stats.host_planned == n and stats.n_lines == len(offs) - 1
    L.h2g_sam_close(hf); L.h2g_sam_close(hw)
    r = dict(text=got, offs=offs, ends=ends, cls=pred, why=why, stats=stats, h=hp)
    if not keep:
        L.h2g_sam_close(hp)
    return r


def _pairs(base, m1, m2, n1, n2, quals=None, opts=(), khits=None, keep=False, ix_setup=None, params=None, setup=None, have_db=False):
    n = len(m1)
    c1, o1 = T._flat(m1); c2, o2 = T._flat(m2)
    nb1, no1 = api.Stream.pack_names(n1); nb2, no2 = api.Stream.pack_names(n2)
    q1, q2 = (None, None) if quals is None else quals
    ix = api.Index(base, device=0)
    if ix_setup:
        ix_setup(ix)
    st = api.Stream(ix, max_reads=n, max_bases=max(c1.size, c2.size, 1))
    st.set_reads(c1, o1, q1); st.set_read_names((nb1, no1)); st.set_mates(c2, o2, (nb2, no2), q2)
    p = st.align_params()
    if khits:
        p.khits = khits
    if params:
        params(p)
    st.align_pairs_run(p)
    fetch = st.align_pairs_fetch_compact()
    L = SL.load_sam_lib()
    sets = ((c1, o1, q1, nb1, no1), (c2, o2, q2, nb2, no2))
    r = _check_planned(st, L, base, True, sets, fetch, int(p.khits), opts, keep, setup=setup, have_db=have_db)
    if keep:
        r.update(st=st, ix=ix, L=L, sets=sets, fetch=fetch, khits=int(p.khits), n=n)
        return r
    st.close(); ix.close()
    return r


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("with_quals", [False, True])
def test_golden_pairs(g1_index, g1s_index, golden_dir, graph, with_quals):
    """the golden pairs on the linear index, and on its SNP graph with 600 pairs cut from the alternate haplotype, whose Zs:Z lines are handed on"""
    m1, m2, q = T._golden_pairs(golden_dir)
    if graph:
        import gzip
        import parity_cases as PC
        snps = [(f[0], f[1], f[2], int(f[3]), f[4]) for f in (l.split() for l in gzip.open(os.path.join(golden_dir, "g1s.snp.gz"), "rt")) if len(f) == 5]
        x1, x2 = synth.make_pairs(synth.apply_snps(PC.load_contigs(golden_dir), snps), 600, 101, 4712, frag_mean=300, frag_sd=30, sub_rate=0.005)
        m1, m2 = list(m1) + list(x1), list(m2) + list(x2)
        q = [str(i) for i in range(len(m1))]
    quals = None
    if with_quals:
        rng = np.random.default_rng(77)
        quals = tuple(rng.integers(33, 74, size=sum(len(r) for r in m), dtype=np.uint8) for m in (m1, m2))
    r = _pairs(g1s_index if graph else g1_index, m1, m2, q, q, quals=quals)
    assert r["cls"].count(SU.P_CONC) > len(m1) // 4 and r["stats"].host_planned > 0
    if graph:
        assert r["text"].count(b"\tZs:Z:") > 0 and "alt" in r["why"]
        lines = r["text"].split(b"\n")
        for i, c in enumerate(r["cls"]):                       # no plain pair's lines carry Zs:Z
            if c:
                assert all(b"\tZs:Z:" not in l for l in lines[int(r["ends"][i - 1]) if i else 0:int(r["ends"][i])])


def test_unpaired_reads(g1_index, golden_dir):
    """the golden unpaired reads whole and as (first, n) = (37, 101)"""
    names, seqs = H.read_fasta_reads(os.path.join(golden_dir, "reads_se.fa.gz"))
    n = len(seqs)
    codes, offs = T._flat(seqs)
    nb, no = api.Stream.pack_names(names)
    ix = api.Index(g1_index, device=0)
    st = api.Stream(ix, max_reads=n, max_bases=codes.size)
    st.set_reads(codes, offs); st.set_read_names((nb, no))
    st.align_run()
    L = SL.load_sam_lib()
    fetch = st.align_fetch_compact()
    r = _check_planned(st, L, g1_index, False, ((codes, offs, None, nb, no),), fetch, 0)
    assert SU.U_UNIQ in r["cls"] and r["stats"].device_planned > n // 2
    first, cnt = 37, 101
    fetch2 = st.align_fetch_compact(first, cnt)
    s2 = (codes[int(offs[first]):], (offs[first:first + cnt + 1] - offs[first]).astype(np.uint32), None, nb[int(no[first]):], (no[first:first + cnt + 1] - no[first]).astype(np.uint32))
    r2 = _check_planned(st, L, g1_index, False, (s2,), fetch2, 0)
    assert r2["text"] in r["text"] and r2["cls"] == r["cls"][first:first + cnt]
    st.close(); ix.close()


def test_ragged_and_empty_reads(g1_index, golden_dir):
    """mates of 0 to 256 bases in every pairing class of tests/ragged_cases.py under the NAMES list: YF:Z:LN / NS and '*' SEQ from the device planner"""
    import parity_cases as PC
    import ragged_cases as RC
    contigs = PC.load_contigs(golden_dir)
    minK, ftab = RC.index_params(g1_index)
    m1, m2, labels = RC.make_ragged_pairs(contigs, 8101, 450, minK, ftab)
    n = len(m1)
    n1 = [T.NAMES[i % len(T.NAMES)] for i in range(n)]
    n2 = [T.NAMES[(i + 3) % len(T.NAMES)] for i in range(n)]
    quals = (RC.seeded_quals(m1, 3), RC.seeded_quals(m2, 4))
    r = _pairs(g1_index, m1, m2, n1, n2, quals=quals)
    assert any(len(x) == 0 for x in m1 + m2) and r["text"].count(b"\tYF:Z:LN") > 0 and {SU.P_NONE, SU.P_CONC} <= set(r["cls"])
    assert any(c in (SU.P_NONE, SU.P_MATE1, SU.P_MATE2) and (len(m1[i]) == 0 or len(m2[i]) == 0) for i, c in enumerate(r["cls"]))


@pytest.mark.parametrize("database", [False, True])
def test_many_scan_tiles(g1_index, golden_dir, database):
    """30 011 pairs: the scan of the per-read line counts spans 15 tiles and the scan of the line sizes 29 and more.  Once more with a splice-site database in the handles
    (one site, far from every fragment's gap): the kernel then takes its database branch for every concordant pair, and every ZS:i, TLEN and class must stay what it was"""
    import parity_cases as PC
    contigs = PC.load_contigs(golden_dir)
    n = 30011
    m1, m2 = synth.make_pairs(contigs, n, 101, 4711, frag_mean=300, frag_sd=30, sub_rate=0.02)
    q = [str(i) for i in range(n)]
    site = api.splice_site_array([(0, 10, 20, "+")], True)

    def setup(L, h):
        L.h2g_sam_set_splice_sites.argtypes = [vp, vp, sz, C.c_uint32]
        L.h2g_sam_set_splice_sites(h, site, 1, 0)
    r = _pairs(g1_index, list(m1), list(m2), q, q, setup=setup if database else None, have_db=database)
    assert r["text"].count(b"\tZS:i:") > 100
    assert (n + 1 + 2047) // 2048 >= 15 and (len(r["offs"]) + 2047) // 2048 >= 29 and r["stats"].host_planned > 0


def test_one_pair(g1_index, golden_dir):
    m1, m2, q = T._golden_pairs(golden_dir)
    r = _pairs(g1_index, m1[:1], m2[:1], q[:1], q[:1])
    assert len(r["cls"]) == 1


@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "hisat2-build-s")), reason="needs oracle/_ref")
def test_every_read_handed_on(tmp_path, golden_dir):
    """-k 5 over a contig and its copy: every pair has two concordant pairings, nothing is plain, and the merge places uploaded descriptors only"""
    import parity_cases as PC
    import test_gpu_large_k as LK
    c = PC.load_contigs(golden_dir)[0][:40000]
    c = c[c < 4][:30000]
    base = LK.build(str(tmp_path), [c, c.copy()])
    m1, m2 = synth.make_pairs([c], 700, 101, 4713, frag_mean=300, frag_sd=30, sub_rate=0.0)
    q = [str(i) for i in range(len(m1))]
    r = _pairs(base, list(m1), list(m2), q, q, khits=5)
    assert not any(r["cls"]) and r["stats"].device_planned == 0 and "np>=2" in r["why"] and len(r["offs"]) - 1 >= 4 * len(m1)


def _alternate_haplotype_pairs(golden_dir, n, seed):
    import gzip
    import parity_cases as PC
    snps = [(f[0], f[1], f[2], int(f[3]), f[4]) for f in (l.split() for l in gzip.open(os.path.join(golden_dir, "g1s.snp.gz"), "rt")) if len(f) == 5]
    return synth.make_pairs(synth.apply_snps(PC.load_contigs(golden_dir), snps), n, 101, seed, frag_mean=300, frag_sd=30, sub_rate=0.005)


def test_every_read_handed_on_graph(g1s_index, golden_dir):
    """the alternate-haplotype pairs alone on the SNP graph, those of them that cross a variant (a first run tells which: a pair's result does not depend on its
    neighbours): nothing is plain, no slot is read, and the merge places uploaded descriptors only"""
    x1, x2 = _alternate_haplotype_pairs(golden_dir, 900, 4714)
    q = ["alt%d" % i for i in range(len(x1))]
    first = _pairs(g1s_index, list(x1), list(x2), q, q)
    hard = [i for i, c in enumerate(first["cls"]) if not c]
    assert len(hard) > 100 and "alt" in first["why"]
    r = _pairs(g1s_index, [x1[i] for i in hard], [x2[i] for i in hard], [q[i] for i in hard], [q[i] for i in hard])
    assert not any(r["cls"]) and r["stats"].device_planned == 0 and r["stats"].host_planned == len(hard) and [first["why"][i] for i in hard] == r["why"]
    assert r["text"].count(b"\tZs:Z:") > 0


@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "hisat2-build-s")), reason="the fixture of test_gpu_zy_spliced.py is an index built by oracle/_ref/hisat2-build-s")
def test_spliced_pairs_with_a_known_site_database(tmp_path):
    """the paired fixture of test_gpu_zy_spliced.py (planted introns, its known-site list) with the database loaded into the index and the handles and template-length
    adjustment on: junction reads and concordant mates far apart are handed on, the rest is planned on the device; text, sites collected and class bytes as everywhere"""
    import fuzz_spliced as FS
    import fuzz_spliced_pairs as FP
    import test_gpu_large_k as LK
    contigs, m1, m2, introns = FP.make_case(371, 3000, sub=0.01)
    base = LK.build(str(tmp_path), contigs)
    sites = FS.known_sites(introns, 371, 0.8)
    arr = api.splice_site_array(sites, True)
    L0 = api.lib()
    L0.h2g_index_set_splice_sites.argtypes = [vp, vp, sz, C.c_uint32]

    def ix_setup(ix):
        assert L0.h2g_index_set_splice_sites(ix.h, arr, len(sites), 0) == 0

    def params(p):
        p.no_spliced_alignment = 0; p.no_temp_splicesite = 1

    def setup(L, h):
        L.h2g_sam_set_splice_sites.argtypes = [vp, vp, sz, C.c_uint32]
        L.h2g_sam_set_splice_sites(h, arr, len(sites), 0)
        L.h2g_sam_collect_novel_sites.argtypes = [vp, C.c_int]
        L.h2g_sam_collect_novel_sites(h, 1)

    q = [str(i) for i in range(len(m1))]
    r = _pairs(base, list(m1), list(m2), q, q, ix_setup=ix_setup, params=params, setup=setup, have_db=True)
    assert "db-tlen" in r["why"] and "splice" in r["why"] and r["cls"].count(SU.P_CONC) > 100
    assert sum(1 for l in r["text"].split(b"\n") if l and b"N" in l.split(b"\t")[5]) > 100
    # the same fetch without a database in the handles: the far-apart mates are plain, and some TLEN differ — the database mattered
    r0 = _pairs(base, list(m1), list(m2), q, q, ix_setup=ix_setup, params=params)
    assert "db-tlen" not in r0["why"] and r0["cls"].count(SU.P_CONC) > r["cls"].count(SU.P_CONC)
    t1, t0 = r["text"].split(b"\n"), r0["text"].split(b"\n")
    assert len(t1) == len(t0) and sum(1 for a, b in zip(t1, t0) if a and a.split(b"\t")[8] != b.split(b"\t")[8]) > 0


def test_refusals_launch_and_count_nothing(g1_index, golden_dir):
    """cap one byte short: H2G_ERR_ARG, *used exact, guard bytes untouched, summary unchanged, then the same call with room succeeds; a stale fetch; the unpaired entry on a
    paired fetch"""
    m1, m2, q = T._golden_pairs(golden_dir)
    k = _pairs(g1_index, m1[:300], m2[:300], q[:300], q[:300], keep=True)
    st, L, text, n = k["st"], k["L"], k["text"], k["n"]
    L.h2g_sam_close(k["h"])
    h = T._handle(L, g1_index)
    empty = PU.summary(L, h)
    s1, s2 = k["sets"]
    res, r1, b1, r2, b2 = k["fetch"]
    a = [api._ptr(x) for x in s1 + s2]
    f = api.lib().h2g_sam_text_paired_planned
    offs = np.zeros(8 * n + 65, dtype=np.uint64)
    ends = np.full(n, 0xA5A5, dtype=np.uint64)

    def call(out, cap, used, nl):
        return f(st.h, h, *a, n, res.ctypes.data, r1.ctypes.data, b1.ctypes.data, r2.ctypes.data, b2.ctypes.data, k["khits"], out.ctypes.data, cap, C.byref(used),
                 offs.ctypes.data, len(offs) - 1, C.byref(nl), ends.ctypes.data)

    def refused(fn=call, want_used=None):
        out = np.full(len(text) + 64, 0xA5, dtype=np.uint8)
        used, nl = sz(0), sz(0)
        cap = len(text) - 1 if want_used is not None else len(text) + 64
        assert fn(out, cap, used, nl) == api.H2G_ERR_ARG and (out == 0xA5).all() and (ends == 0xA5A5).all()
        assert want_used is None or used.value == want_used
        assert PU.summary(L, h) == empty

    st.align_pairs_fetch_compact()
    refused(want_used=len(text))
    out = np.full(len(text) + 64, 0xA5, dtype=np.uint8)
    used, nl = sz(0), sz(0)
    assert call(out, len(text), used, nl) == 0 and out[:len(text)].tobytes() == text and (out[len(text):] == 0xA5).all() and int(ends[-1]) == nl.value
    once = PU.summary(L, h)
    assert once != empty
    empty = once
    ends[:] = 0xA5A5
    st.align_pairs_fetch_compact(0, 10)                    # stale: another range fetched since
    refused()
    st.align_pairs_fetch_compact()
    st.select_batch(1); st.select_batch(0)                 # stale: the selection made the buffers nobody's
    refused()
    st.align_pairs_fetch_compact()
    fu = api.lib().h2g_sam_text_unpaired_planned           # the unpaired entry on a paired fetch
    refused(lambda out, cap, used, nl: fu(st.h, h, *a[:5], n, res.ctypes.data, r1.ctypes.data, b1.ctypes.data, out.ctypes.data, cap, C.byref(used), offs.ctypes.data,
                                          len(offs) - 1, C.byref(nl), ends.ctypes.data))
    assert api.lib().h2g_last_error()
    assert call(out, len(text), used, nl) == 0 and out[:len(text)].tobytes() == text       # (the refusals left the fetch in place)
    L.h2g_sam_close(h); st.close(); k["ix"].close()
