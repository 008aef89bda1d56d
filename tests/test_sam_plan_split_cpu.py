"""The split SAM planner on the host (include/h2g.h h2g_sam_plan_split_host: classification and the plain planner of csrc/h2g_sam_plan.h instantiated on the host, the
host planner over the handed-on reads, the merge) against the whole planner h2g_sam_plan_*_compact: descriptors, pool and line ends byte for byte, the same summary and
collected junctions, and class bytes equal to the predicate "plain" restated in Python (sam_split_util.py).  No device is needed.

  * every record set that tests/test_sam_plan_cpu.py runs: the tests of test_sam_lines / test_long_edits_cpu run here again under sam_split_util.SplitCheckLib, and so do
    the synthetic sets of test_sam_plan_cpu;
  * a hand-made set that holds every class and every reason to hand a read on, under the options that reach the planner;
  * capacities that are too small; the planner read by read under ASan + UBSan over exactly sized copies, damaged bytes included (tests/samtext/plan_lanes.cpp)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import sam_lines as SL
import sam_plan_util as PU
import sam_split_util as SU
import test_long_edits_cpu as _TLE
import test_sam_lines as _TSL
import test_sam_plan_cpu as _TPC
from hisat2_amd import api

vp, sz = C.c_void_p, C.c_size_t
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _checked_library(monkeypatch):
    real = SL.load_sam_lib
    monkeypatch.setattr(SL, "load_sam_lib", lambda path=None: SU.SplitCheckLib(real(path)))


# tests of those two modules that never format compact records (row layouts only, headers, summaries of their own): the check would not fire in them
NO_COMPACT_CALL = {"test_golden_spliced_default_mode_p1", "test_haplotype_option", "test_new_summary", "test_novel_splicesite_outfile_pairs_no_database", "test_remove_chrname",
                   "test_spliced_on_real_sequence", "test_spliced_scoring_options", "test_temporary_splice_sites_multi_junction_multi_contig",
                   "test_temporary_splice_sites_on_snp_graph", "test_temporary_splice_sites_wave_scheme", "test_temporary_splice_sites_with_known_file_and_outfile"}


def _reaching(fn):
    @functools.wraps(fn)
    def run(*a, **k):
        before = SU.COVER["calls"]
        fn(*a, **k)
        assert SU.COVER["calls"] > before, "this test does not reach a compact format call any more: the split planner was not checked in it"
    return run


for _mod in (_TSL, _TLE):
    for _name, _obj in list(vars(_mod).items()):
        if _name.startswith("test_") and callable(_obj) and _name not in NO_COMPACT_CALL:
            globals()["test_split__" + _name[5:]] = _reaching(_obj)
del _mod, _name, _obj


@pytest.mark.parametrize("opts", _TPC.OPTION_SETS)
@pytest.mark.parametrize("index,snps", [("g1_index", 0), ("g1s_index", 3)])
def test_synthetic_unpaired_sets(request, index, snps, opts):
    """the synthetic unpaired set of test_sam_plan_cpu (every edit kind, trims, a record beyond MAX_EDITS, ALT edits on the graph index): split == whole at its format call"""
    base = request.getfixturevalue(index)
    reads, names, res, aln, led = _TPC._unpaired_case(base, 9100 + snps, snps)
    before = SU.COVER["calls"]
    SL.format_unpaired(SL.load_sam_lib(), base, reads, names, res, aln, options=list(opts), long_edits=led)
    assert SU.COVER["calls"] == before + 1


@pytest.mark.parametrize("opts", _TPC.OPTION_SETS + [("-k", "1")])
@pytest.mark.parametrize("index,snps", [("g1_index", 0), ("g1s_index", 3)])
def test_synthetic_paired_sets(request, index, snps, opts):
    base = request.getfixturevalue(index)
    m1, m2, n1, n2, res, a1, a2 = _TPC._paired_case(base, 9200 + snps, snps)
    before = SU.COVER["calls"]
    SL.format_paired(SL.load_sam_lib(), base, m1, m2, n1, n2, res, a1, a2, 1 if "-k" in opts else 5, options=[o for o in opts if o not in ("-k", "1")])
    assert SU.COVER["calls"] == before + 1


# ---- a hand-made set: every class, every reason ---------------------------------------------------------------------------------------------
MM, RGAP, SPL = 3, 1, 5
NONE = 0xffffffff
INT32 = -(1 << 31)                                                    # an invalid best / second-best score


def _rec(fw=1, tidx=0, toff=1000, ln=50, score=-6, edits=(), trim5=0, trim3=0, nedits=None):
    """one compact record; edits: (pos, type, snp) — a splice edit gets a length of 300 and a known '+' site"""
    ne = len(edits) if nedits is None else nedits
    b = bytearray(np.array([fw, tidx, toff, ln, trim5, trim3, ne, 0], dtype=np.uint32).tobytes() + np.array([score], dtype=np.int64).tobytes())
    for pos, typ, snp in edits:
        if typ == SPL:
            b += np.array([pos], dtype=np.uint32).tobytes() + bytes([300 & 255, 300 >> 8, typ, 0x80 | (2 << 4)]) + np.array([0x3f000000], dtype=np.uint32).tobytes()
        else:
            b += np.array([pos], dtype=np.uint32).tobytes() + bytes([ord("A"), ord("-") if typ == RGAP else ord("C"), typ, 0]) + np.array([snp], dtype=np.uint32).tobytes()
    if len(b) % 8:
        b += b"\0\0\0\0"
    return bytes(b)


def _long_rec(at, **kw):
    """a record beyond MAX_EDITS: 40 mismatches in the long-edit area from entry `at`"""
    b = bytearray(_rec(nedits=40, **kw)[:40])
    b += np.array([at], dtype=np.uint32).tobytes() + bytes(4) + np.array([0x4c4f4e47], dtype=np.uint32).tobytes() + bytes(4)
    return bytes(b)


def _trailer(pairs):
    b = bytearray(40)
    b[4:8] = np.array([len(pairs)], dtype=np.uint32).tobytes()
    b[24:28] = np.array([SU.TRAILER_TAG], dtype=np.uint32).tobytes()
    b += np.array([i | (j << 16) for i, j in pairs], dtype=np.uint32).tobytes()
    if len(b) % 8:
        b += b"\0\0\0\0"
    return bytes(b)


def _long_area():
    area = (api.Edit * 64)()
    for k in range(64):
        area[k].pos, area[k].chr, area[k].qchr, area[k].type, area[k].snp = k, ord("A"), ord("C"), MM, NONE
    return area


def paired_cover_set(snps):
    """[(mate-1 records, mate-2 records, pairings, expected reason or class)], reads of 50 bases.  ALT edits need snps > 0 (the graph index)."""
    mm = [(7, MM, NONE), (30, MM, NONE)]
    far = dict(toff=1000), dict(toff=1800, fw=0)                      # mates 750 bases apart: with a database, fragment_length looks introns up
    P = [
        ([_rec(edits=mm)], [_rec(toff=1100, fw=0)], [(0, 0)], SU.P_CONC),
        ([_rec(score=-3), _rec(toff=5000, score=-9, edits=mm)], [_rec(toff=1150, fw=0, score=0)], [(0, 0)], SU.P_CONC),         # ZS:i on mate 1 from a record that is only scored
        ([_rec(toff=5000, edits=[(20, SPL, 0)]), _rec()], [_rec(toff=1100, fw=0)], [(1, 0)], SU.P_CONC),                        # the other record may be anything that can be scored
        ([_rec()], [_rec(toff=1100, fw=0)], [(0, 0), (3, 0)], SU.P_CONC),                                                       # a pairing beyond n1 is dropped: np == 1
        ([_rec(**far[0])], [_rec(**far[1])], [(0, 0)], "db-tlen"),
        ([_rec()], [_rec(toff=90000)], [], SU.P_DISC),
        ([_rec(trim5=2)], [_rec(toff=1000, fw=1, trim3=1)], [], SU.P_DISC),
        ([], [], [], SU.P_NONE),
        ([_rec(edits=mm, fw=0)], [], [], SU.P_MATE1),
        ([], [_rec(toff=77, fw=0)], [], SU.P_MATE2),
        ([_rec(), _rec(toff=3000)], [_rec(toff=9000)], [], "multi"),
        ([_rec(), _rec(toff=3000)], [_rec(toff=1100, fw=0), _rec(toff=3100, fw=0)], [(0, 0), (1, 1)], "np>=2"),
        ([_rec(edits=[(9, RGAP, NONE)])], [_rec(toff=1100, fw=0)], [(0, 0)], "gap"),
        ([_rec()], [_rec(toff=1100, fw=0, edits=[(25, SPL, 0)])], [(0, 0)], "splice"),
        ([_long_rec(0)], [_rec(toff=1100, fw=0)], [(0, 0)], "long"),
        ([_rec(), _long_rec(8, toff=7000)], [_rec(toff=1100, fw=0)], [(0, 0)], "long"),                                          # a record that would only be scored
        ([_rec() + _trailer([(0, 0)])], [_rec(toff=1100, fw=0)], [], "trailer"),
        ([_rec(edits=[(4, RGAP, NONE)])], [], [], "gap"),
    ]
    if snps:
        P.append(([_rec(edits=[(11, MM, 1)])], [_rec(toff=1100, fw=0)], [(0, 0)], "alt"))
        P.append(([_rec(edits=[(11, MM, 0)])], [_rec(toff=90000)], [], "alt"))
    return P


def build_paired(P):
    n = len(P)
    rng = np.random.default_rng(77)
    m1 = [rng.integers(0, 4, size=50).astype(np.uint8) for _ in range(n)]
    m2 = [rng.integers(0, 4, size=50).astype(np.uint8) for _ in range(n)]
    m2[7][:] = 4                                                       # an unaligned mate that fails --n-ceil: YF:Z:NS
    names1 = ["p%d/1" % i for i in range(n)]; names2 = ["p%d/2" % i for i in range(n)]
    res = (api.PairResult * n)()
    rec1, rec2 = bytearray(), bytearray()
    bo1, bo2 = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
    for i, (r1, r2, pairs, _) in enumerate(P):
        res[i].nres[0], res[i].nres[1], res[i].npairs, res[i].rnd_state = len(r1), len(r2), len(pairs), 12345 + i
        for k, (x, y) in enumerate(pairs):
            res[i].pair_i[k], res[i].pair_j[k] = x, y
        rec1 += b"".join(r1); rec2 += b"".join(r2)
        bo1[i + 1], bo2[i + 1] = len(rec1), len(rec2)
    c1, o1 = SL.flat(m1); c2, o2 = SL.flat(m2)
    nb1, no1 = SL.flat_names(names1); nb2, no2 = SL.flat_names(names2)
    return [None, c1, o1, None, nb1, no1, c2, o2, None, nb2, no2, n, res, bytes(rec1) + bytes(8), bo1, bytes(rec2) + bytes(8), bo2, 5]


def unpaired_cover_set(snps):
    mm = [(7, MM, NONE)]
    U = [([], (0, INT32, INT32), SU.U_UNAL),
         ([_rec(edits=mm)], (1, -6, INT32), SU.U_UNIQ),
         ([_rec(edits=mm, fw=0, trim5=3)], (1, -6, -12), SU.U_UNIQ),                     # ZS:i, MAPQ 60: second best is worse
         ([_rec()], (1, -6, -6), "tied"),
         ([_rec(), _rec(toff=4000)], (2, -6, -6), "multi"),
         ([_rec(edits=[(5, RGAP, NONE)])], (1, -6, INT32), "gap"),
         ([_rec(edits=[(25, SPL, 0)])], (1, -6, INT32), "splice"),
         ([_long_rec(0)], (1, -6, INT32), "long")]
    if snps:
        U.append(([_rec(edits=[(11, MM, 2)])], (1, -6, INT32), "alt"))
    return U


def build_unpaired(U):
    n = len(U)
    rng = np.random.default_rng(78)
    reads = [rng.integers(0, 4, size=50).astype(np.uint8) for _ in range(n)]
    reads[0] = np.zeros(0, dtype=np.uint8)                             # an empty read: YF:Z:LN, '*' SEQ
    res = (api.ReadResult * n)()
    rec = bytearray()
    bo = np.zeros(n + 1, dtype=np.uint64)
    for i, (rs, (nsel, best, sec), _) in enumerate(U):
        res[i].nselect = res[i].nres = nsel
        res[i].best, res[i].secbest, res[i].best_h2, res[i].secbest_h2 = best, sec, 0xffff, 0xffff
        rec += b"".join(rs)
        bo[i + 1] = len(rec)
    codes, offs = SL.flat(reads)
    nb, noffs = SL.flat_names(["u%d" % i for i in range(n)])
    return [None, codes, offs, None, nb, noffs, n, res, bytes(rec) + bytes(8), bo]


def _handles(base, setup):
    L = SL.load_sam_lib()._L
    hs = []
    for _ in range(2):
        h = vp()
        assert L.h2g_sam_open(base.encode(), C.byref(h)) == 0
        setup(L, h)
        hs.append(h)
    return L, hs


def _setter(L, name, *types):
    f = getattr(L, name)
    f.argtypes = [vp] + list(types)
    return f


KEEP = []                                                              # arrays a handle points to


def _opt_no_unal(L, h):
    _setter(L, "h2g_sam_set_no_unal", C.c_int)(h, 1)


def _opt_filter(n):
    def f(L, h):
        q1 = np.ones(n, dtype=np.uint8); q2 = np.ones(n, dtype=np.uint8)
        q1[::3] = 0; q2[1::4] = 0
        KEEP.extend([q1, q2])
        _setter(L, "h2g_sam_set_read_filter", vp, vp)(h, q1.ctypes.data, q2.ctypes.data)
    return f


def _opt_ids(n):
    def f(L, h):
        ids = (np.arange(n, dtype=np.uint64) * 7 + 1000)
        KEEP.append(ids)
        _setter(L, "h2g_sam_set_read_ids", vp)(h, ids.ctypes.data)
        _setter(L, "h2g_sam_collect_novel_sites", C.c_int)(h, 1)
    return f


def _opt_db(L, h):
    sites = api.splice_site_array([(0, 1100, 1700, "+"), (0, 1090, 1750, "+")])
    KEEP.append(sites)
    _setter(L, "h2g_sam_set_splice_sites", vp, sz, C.c_uint32)(h, sites, 2, 0)


def _cli(*opts):
    return lambda L, h: SL._score_min(L, h, list(opts))


OPTIONS = {"default": (lambda L, h: None, {}), "no-mixed": (_cli("--no-mixed"), {"mixed": False}), "no-discordant": (_cli("--no-discordant"), {"discordant": False}),
           "no-unal": (_opt_no_unal, {}), "omit-sec-seq": (_cli("--omit-sec-seq", "--secondary"), {}), "strand-RF": (_cli("--rna-strandness", "RF"), {}),
           "read-group": (_cli("--rg-id", "grp", "--rg", "SM:s"), {}), "qc-filter": (None, {}), "read-ids": (None, {}),
           "database": (_opt_db, {"have_db": True}), "database-no-adjust": (lambda L, h: (_opt_db(L, h), _cli("--no-templatelen-adjustment")(L, h)), {"have_db": True, "tlen_adjust": False})}


def _run(base, snps, name, paired):
    a = build_paired(paired_cover_set(snps)) if paired else build_unpaired(unpaired_cover_set(snps))
    n = a[11] if paired else a[6]
    setup, kw = OPTIONS[name]
    setup = _opt_filter(n) if name == "qc-filter" else _opt_ids(n) if name == "read-ids" else setup
    area = _long_area()

    def full(L, h):
        setup(L, h)
        _setter(L, "h2g_sam_set_long_edits", vp, sz)(h, area, 64)
    L, (hw, hs) = _handles(base, full)
    nalts, nrefs = SU.index_facts(base)
    assert nalts >= snps
    r = SU.check_split(L, base, [], paired, tuple(a), hw, hs, note=False, opts=SU.Opts(nalts, nrefs, **kw))
    assert PU.summary(L, hs) != b""
    L.h2g_sam_close(hw); L.h2g_sam_close(hs)
    return r


@pytest.mark.parametrize("index,snps", [("g1_index", 0), ("g1s_index", 3)])
def test_cover_set_holds_every_class_and_reason(request, index, snps):
    """checked first: the hand-made sets hold each class and each reason to hand on; the predicate says of each entry what the set's author meant"""
    base = request.getfixturevalue(index)
    want = [w for *_, w in paired_cover_set(snps)]
    cls, why = _run(base, snps, "default", True)
    for i, w in enumerate(want):
        if w == "db-tlen":
            assert cls[i] == SU.P_CONC                               # (no database here)
        elif isinstance(w, str):
            assert cls[i] == SU.HOST and why[i] == w, (i, w, why[i])
        else:
            assert cls[i] == w, (i, w, cls[i], why[i])
    assert {SU.P_CONC, SU.P_DISC, SU.P_NONE, SU.P_MATE1, SU.P_MATE2} <= set(cls) and {"np>=2", "gap", "splice", "long", "trailer", "multi"} <= set(why)
    cls, why = _run(base, snps, "database", True)
    assert why[want.index("db-tlen")] == "db-tlen" and cls[0] == SU.P_CONC
    cls, why = _run(base, snps, "database-no-adjust", True)
    assert cls[want.index("db-tlen")] == SU.P_CONC
    cls, why = _run(base, snps, "default", True)
    wantu = [w for *_, w in unpaired_cover_set(snps)]
    clsu, whyu = _run(base, snps, "default", False)
    for i, w in enumerate(wantu):
        assert (clsu[i] == SU.HOST and whyu[i] == w) if isinstance(w, str) else clsu[i] == w, (i, w, clsu[i], whyu[i])
    assert {SU.U_UNAL, SU.U_UNIQ} <= set(clsu) and {"tied", "multi", "gap", "splice", "long"} <= set(whyu)
    if snps:
        assert "alt" in why and "alt" in whyu
    # class (c) with both mates aligned needs discordant reporting off
    cls, why = _run(base, snps, "no-discordant", True)
    assert SU.P_BOTH in cls and SU.P_DISC not in cls


ALL_CLASSES = {SU.U_UNAL, SU.U_UNIQ, SU.P_CONC, SU.P_DISC, SU.P_NONE, SU.P_MATE1, SU.P_MATE2, SU.P_BOTH}
ALL_REASONS = {"np>=2", "gap", "splice", "alt", "long", "tied", "trailer", "db-tlen"}


def test_record_sets_together_cover_the_list(monkeypatch, g1_index, g1s_index):
    """the synthetic sets of test_sam_plan_cpu (through the checked library, so every class byte is compared with the predicate) hold every class and the reasons
    np >= 2, gap, splice, ALT edit and long record; a tied best with one alignment selected, a trailer and the database TLEN case exist only in the hand-made set, which
    was added for them: together they hold the whole list"""
    seen = {"classes": set(), "reasons": set(), "calls": 0, "reads": 0, "plain": 0}
    monkeypatch.setattr(SU, "COVER", seen)
    for base, snps in ((g1_index, 0), (g1s_index, 3)):
        reads, names, res, aln, led = _TPC._unpaired_case(base, 9100 + snps, snps)
        SL.format_unpaired(SL.load_sam_lib(), base, reads, names, res, aln, long_edits=led)
        m1, m2, n1, n2, pres, a1, a2 = _TPC._paired_case(base, 9200 + snps, snps)
        for opts in ((), ("--no-discordant",)):
            SL.format_paired(SL.load_sam_lib(), base, m1, m2, n1, n2, pres, a1, a2, 5, options=list(opts))
    assert seen["calls"] == 6 and 0 < seen["plain"] < seen["reads"]
    assert seen["classes"] == ALL_CLASSES | {SU.HOST}
    assert {"np>=2", "gap", "splice", "alt", "long", "multi"} <= seen["reasons"]
    hand = set()
    for name, paired in (("default", True), ("database", True), ("default", False)):
        hand |= {w for w in _run(g1s_index, 3, name, paired)[1] if w}
    assert ALL_REASONS - seen["reasons"] <= {"tied", "trailer", "db-tlen"} <= hand and ALL_REASONS <= seen["reasons"] | hand


@pytest.mark.parametrize("paired", [True, False])
@pytest.mark.parametrize("name", [k for k in OPTIONS if k != "default"])
@pytest.mark.parametrize("index,snps", [("g1_index", 0), ("g1s_index", 3)])
def test_options(request, index, snps, name, paired):
    cls, why = _run(request.getfixturevalue(index), snps, name, paired)
    assert any(cls) and not all(cls)
    if name == "no-mixed" and paired:
        assert SU.P_MATE1 not in cls and "multi" not in why and cls.count(SU.P_NONE) >= 4


@pytest.mark.parametrize("paired", [True, False])
def test_partial_range(request, g1_index, paired):
    """(first, n) = (37, 101) of a synthetic set: lines[].read counts from the range's first read"""
    if paired:
        m1, m2, n1, n2, res, a1, a2 = _TPC._paired_case(g1_index, 9600, n=150)
        L = SL.load_sam_lib()._L
        n = len(m1)
        c1, o1 = SL.flat(m1); c2, o2 = SL.flat(m2)
        nb1, no1 = SL.flat_names(n1); nb2, no2 = SL.flat_names(n2)
        rec1, bo1 = SL.to_compact(a1, np.arange(n) * api.PAIR_RES_CAP, [res[i].nres[0] for i in range(n)])
        rec2, bo2 = SL.to_compact(a2, np.arange(n) * api.PAIR_RES_CAP, [res[i].nres[1] for i in range(n)])
        sub = (api.PairResult * 101).from_address(C.addressof(res) + 37 * C.sizeof(api.PairResult))
        a = (None, c1, o1[37:139], None, nb1, no1[37:139], c2, o2[37:139], None, nb2, no2[37:139], 101, sub, rec1, bo1[37:139], rec2, bo2[37:139], 5)
    else:
        reads, names, res, aln, led = _TPC._unpaired_case(g1_index, 9601, n=150)
        L = SL.load_sam_lib()._L
        n = len(reads)
        codes, offs = SL.flat(reads); nb, noffs = SL.flat_names(names)
        rec, bo = SL.to_compact(aln, np.arange(n) * api.ALN_CAP, [res[i].nselect for i in range(n)])
        sub = (api.ReadResult * 101).from_address(C.addressof(res) + 37 * C.sizeof(api.ReadResult))
        a = (None, codes, offs[37:139], None, nb, noffs[37:139], 101, sub, rec, bo[37:139])
    a = tuple(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x for x in a)
    hs = []
    for _ in range(2):
        h = vp()
        assert L.h2g_sam_open(g1_index.encode(), C.byref(h)) == 0
        if not paired:
            _setter(L, "h2g_sam_set_long_edits", vp, sz)(h, led[0], led[1])
        _setter(L, "h2g_sam_set_first_read_id", C.c_uint64)(h, 37)
        hs.append(h)
    nalts, nrefs = SU.index_facts(g1_index)
    cls, why = SU.check_split(L, g1_index, [], paired, a, hs[0], hs[1], note=False, opts=SU.Opts(nalts, nrefs))
    assert len(cls) == 101 and any(cls) and not all(cls)
    for h in hs:
        L.h2g_sam_close(h)


def test_short_capacity_counts_nothing(g1_index):
    a = build_paired(paired_cover_set(0))
    area = _long_area()
    L, (hw, hs) = _handles(g1_index, lambda L, h: _setter(L, "h2g_sam_set_long_edits", vp, sz)(h, area, 64))
    empty = PU.summary(L, hs)
    f = L.h2g_sam_plan_split_host
    f.argtypes = [vp] * 11 + [sz, vp, vp, vp, vp, vp, C.c_uint32, vp, sz, C.POINTER(sz), vp, sz, C.POINTER(sz), vp, vp]
    args = [PU._addr(x) for x in a]
    nl, na = sz(0), sz(0)
    call = lambda lines, lc, aux, ac: f(hs, *args[1:11], a[11], *args[12:17], a[17], None if lines is None else lines.ctypes.data, lc, C.byref(nl),
                                        None if aux is None else aux.ctypes.data, ac, C.byref(na), None, None)
    assert call(None, 0, None, 0) == api.H2G_ERR_ARG and nl.value > a[11] and na.value > 0
    need_l, need_a = nl.value, na.value
    lines = np.zeros(need_l, dtype=api.SAM_LINE_DTYPE); aux = np.zeros(need_a, dtype=np.uint8)
    for lc, ac in ((need_l - 1, need_a), (need_l, need_a - 1)):
        nl.value = na.value = 0
        assert call(lines, lc, aux, ac) == api.H2G_ERR_ARG and (nl.value, na.value) == (need_l, need_a)
        assert PU.summary(L, hs) == empty and not lines.view(np.uint8).any() and not aux.any()
    assert call(lines, need_l, aux, need_a) == 0
    assert PU.summary(L, hs) != empty
    rc, l2, a2, _ = SU.plan_whole(L, hw, True, tuple(a))
    assert rc == 0 and l2.tobytes() == lines.tobytes() and a2.tobytes() == aux.tobytes() and PU.summary(L, hw) == PU.summary(L, hs)
    L.h2g_sam_close(hw); L.h2g_sam_close(hs)


def test_api_wrapper(g1_index):
    a = build_unpaired(unpaired_cover_set(0))
    area = _long_area()
    L, (hw, hs) = _handles(g1_index, lambda L, h: _setter(L, "h2g_sam_set_long_edits", vp, sz)(h, area, 64))
    lines, aux, ends, cls = api.sam_plan_split_host(hs.value, (a[1], a[2], None, a[4], a[5]), None, a[7], a[8], a[9])
    l2, a2, e2 = api.sam_plan_unpaired(hw.value, a[1], a[2], None, a[4], a[5], a[7], a[8], a[9])
    assert lines.tobytes() == l2.tobytes() and aux.tobytes() == a2.tobytes() and (ends == e2).all() and list(cls[:2]) == [api.SAM_CLS_U_UNAL, api.SAM_CLS_U_UNIQ]
    L.h2g_sam_close(hw); L.h2g_sam_close(hs)


def test_planner_read_by_read_under_sanitizers(tmp_path):
    """tests/samtext/plan_lanes.cpp drives the H2G_HD planner read by read over exactly sized heap copies of each read's bytes, damaged ones included (an nedits that runs
    past the read's end, a truncated last record, a trailer with a count beyond its bytes, pair_i beyond n1): clean under ASan + UBSan, and handed on or dropped"""
    exe = str(tmp_path / "plan_lanes")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", exe,
                    os.path.join(ROOT, "tests", "samtext", "plan_lanes.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout and int(r.stdout.split()[0]) > 200, r.stdout + r.stderr
