"""The split planner (include/h2g.h: h2g_sam_plan_split_host / h2g_sam_text_*_planned; csrc/h2g_sam_plan.h) against the whole planner it must equal.

  * predicate_*: the predicate "plain" restated in Python from the fetched arrays alone (result headers, compact bytes, offsets) — nothing of it comes from the library;
  * SplitCheckLib: a stand-in for the library object of sam_lines.load_sam_lib() (the idea of sam_plan_util.PlanCheckLib): every call goes through, and at each
    h2g_sam_format_*_compact call the same arguments also run through h2g_sam_plan_*_compact on one twin handle and h2g_sam_plan_split_host on another: descriptors, pool,
    line ends, summary and collected sites must be equal, and the class bytes must equal the predicate.  COVER collects which classes and hand-on reasons were met."""
import ctypes as C

import numpy as np

import sam_plan_util as PU
from hisat2_amd import api

vp, sz = C.c_void_p, C.c_size_t
MAX_EDITS = api.MAX_EDITS
TRAILER_TAG = 0x52494150
INT32_MIN = -(1 << 31)
HOST, U_UNAL, U_UNIQ, P_CONC, P_DISC, P_NONE, P_MATE1, P_MATE2, P_BOTH = range(9)
COVER = {"classes": set(), "reasons": set(), "calls": 0, "reads": 0, "plain": 0}
_INDEX_FACTS = {}


class _OracleAlt(C.Structure):      # h2o_alt (oracle/h2o.h)
    _fields_ = [("pos", C.c_uint32), ("type", C.c_uint32), ("len", C.c_uint32), ("seq", C.c_uint64)]


def _index_facts3(base):
    base = base.decode() if isinstance(base, bytes) else base
    if base not in _INDEX_FACTS:
        import h2o_py
        ix = h2o_py.load_index(h2o_py.load(), base)
        nalts = int(ix.contents.nalts)
        alts = (_OracleAlt * max(nalts, 1)).from_address(ix.contents.alts) if nalts else []
        _INDEX_FACTS[base] = (nalts, int(ix.contents.r.nrefs), any(a.type == 5 for a in alts))       # 5: a splice-site ALT — such an index brings a database of its own
    return _INDEX_FACTS[base]


def index_facts(base):
    """(number of ALTs, number of references) of an index, read by the oracle's loader"""
    return _index_facts3(base)[:2]


class Opts:
    def __init__(self, nalts, nrefs, discordant=True, mixed=True, tlen_adjust=True, have_db=False):
        self.nalts, self.nrefs, self.discordant, self.mixed, self.tlen_adjust, self.have_db = nalts, nrefs, discordant, mixed, tlen_adjust, have_db


def _u32(raw, at):
    return int.from_bytes(raw[at:at + 4], "little")


def _record_reason(raw, off, o):
    """None when the record at off is device-plannable, else why not"""
    ne = _u32(raw, off + 24)
    if ne > MAX_EDITS:
        return "long"
    if _u32(raw, off + 4) >= o.nrefs:
        return "reference"
    for k in range(ne):
        e = off + 40 + 12 * k
        typ, snp = raw[e + 6], _u32(raw, e + 8)
        if typ == 5:
            return "splice"
        if typ != 3:
            return "gap"
        if snp < o.nalts:
            return "alt"
    return None


def _walk(raw, b, e):
    """the records of bytes [b, e) as compact_walk finds them -> (offsets, parses, trailer)"""
    offs, p = [], b
    while p + 40 <= e:
        ne = _u32(raw, p + 24)
        if ne == TRAILER_TAG:
            return offs, True, True
        nb = (40 + 12 * (1 if ne > MAX_EDITS else ne) + 7) & ~7
        if p + nb > e:
            return offs, False, False
        offs.append(p)
        p += nb
    return offs, p == e, False


def predicate_unpaired(res, raw, boffs, n, o):
    """-> ([class], [reason or None]) for reads 0 .. n; res: ReadResult-like rows"""
    cls, why = [], []
    for i in range(n):
        r = res[i]
        c, w = HOST, None
        b, e = int(boffs[i]), int(boffs[i + 1])
        if r.nselect > 1:
            w = "multi"
        elif r.secbest != INT32_MIN and r.best != INT32_MIN and r.best == r.secbest and r.best_h2 == r.secbest_h2:
            w = "tied"
        elif r.nselect == 0:
            c = U_UNAL
        else:
            offs, ok, trailer = _walk(raw, b, e)
            if not offs:
                w = "parse"
            else:
                w = _record_reason(raw, offs[0], o)
                if w is None:
                    c = U_UNIQ
        cls.append(c); why.append(w)
    return cls, why


def _ends(raw, off):
    toff, ln, t5, t3 = _u32(raw, off + 8), _u32(raw, off + 12), _u32(raw, off + 16), _u32(raw, off + 20)
    return toff - t5, toff + ln - 1 + t3


def predicate_paired(res, raw1, boffs1, raw2, boffs2, n, o):
    cls, why = [], []
    for i in range(n):
        pr = res[i]
        c, w = HOST, None
        r1, ok1, tr1 = _walk(raw1, int(boffs1[i]), int(boffs1[i + 1]))
        r2, ok2, tr2 = _walk(raw2, int(boffs2[i]), int(boffs2[i + 1]))
        if tr1 or tr2:
            w = "trailer"
        elif not ok1 or not ok2:
            w = "parse"
        else:
            n1, n2 = len(r1), len(r2)
            pairs = [(pr.pair_i[k], pr.pair_j[k]) for k in range(min(pr.npairs, api.PAIR_CAP)) if pr.pair_i[k] < n1 and pr.pair_j[k] < n2]
            if len(pairs) >= 2:
                w = "np>=2"
            elif len(pairs) == 1:
                if any(_u32(raw1, x + 24) > MAX_EDITS for x in r1) or any(_u32(raw2, x + 24) > MAX_EDITS for x in r2):
                    w = "long"
                else:
                    a, b = r1[pairs[0][0]], r2[pairs[0][1]]
                    w = _record_reason(raw1, a, o) or _record_reason(raw2, b, o)
                    if w is None and o.have_db and o.tlen_adjust:
                        (sa, ea), (sb, eb) = _ends(raw1, a), _ends(raw2, b)
                        if min(ea, eb) + 100 < max(sa, sb):
                            w = "db-tlen"
                    if w is None:
                        c = P_CONC
            elif o.discordant and n1 == 1 and n2 == 1:
                w = _record_reason(raw1, r1[0], o) or _record_reason(raw2, r2[0], o)
                if w is None:
                    c = P_DISC
            else:
                u1, u2 = (n1, n2) if o.mixed else (0, 0)
                if u1 > 1 or u2 > 1:
                    w = "multi"
                else:
                    w = (_record_reason(raw1, r1[0], o) if u1 else None) or (_record_reason(raw2, r2[0], o) if u2 else None)
                    if w is None:
                        c = P_BOTH if u1 and u2 else P_MATE1 if u1 else P_MATE2 if u2 else P_NONE
        cls.append(c); why.append(w)
    return cls, why


def opts_from_log(base, log):
    """the handle state the predicate depends on, from the setter calls a handle has seen"""
    nalts, nrefs = index_facts(base)
    o = Opts(nalts, nrefs, have_db=_index_facts3(base)[2])
    for name, a in log:
        if name == "h2g_sam_set_report_policy":
            o.discordant, o.mixed = bool(a[1]), bool(a[2])
        elif name == "h2g_sam_set_templatelen_adjustment":
            o.tlen_adjust = bool(a[1])
        elif name == "h2g_sam_set_splice_sites":
            o.have_db = a[2] > 0 or _index_facts3(base)[2]
        elif name == "h2g_sam_add_splice_sites" and a[2] > 0:
            o.have_db = True
    return o


def split_host(L, h, paired, a):
    """a = the arguments of the format call behind the handle, up to khits -> (rc, lines, aux, line_ends, classes) of h2g_sam_plan_split_host on handle h"""
    n = a[11] if paired else a[6]
    args = [PU._addr(x) for x in a]
    f = L.h2g_sam_plan_split_host
    f.argtypes = [vp] * 11 + [sz, vp, vp, vp, vp, vp, C.c_uint32, vp, sz, C.POINTER(sz), vp, sz, C.POINTER(sz), vp, vp]
    if paired:
        head, tail = args[1:11], args[12:17] + [a[17]]
    else:
        head, tail = args[1:6] + [None] * 5, args[7:10] + [None, None, 0]
    nl, na = sz(0), sz(0)
    ends = np.zeros(max(n, 1), dtype=np.uint64)
    cls = np.full(max(n, 1), 0xEE, dtype=np.uint8)
    rc = f(h, *head, n, *tail, None, 0, C.byref(nl), None, 0, C.byref(na), ends.ctypes.data, cls.ctypes.data)
    if rc != 0 and nl.value == 0 and na.value == 0:
        return rc, None, None, None, None
    lines = np.zeros(max(nl.value, 1), dtype=api.SAM_LINE_DTYPE)
    aux = np.zeros(max(na.value, 1), dtype=np.uint8)
    if rc != 0:
        assert (cls == 0xEE).all()                                       # (a refusal writes nothing)
        rc = f(h, *head, n, *tail, lines.ctypes.data, nl.value, C.byref(nl), aux.ctypes.data, na.value, C.byref(na), ends.ctypes.data, cls.ctypes.data)
        assert rc == 0, rc
    return 0, lines[:nl.value], aux[:na.value], ends[:n], cls[:n]


def plan_whole(L, h, paired, a):
    """a = the arguments of the format call, up to khits -> (rc, lines, aux, line_ends) of h2g_sam_plan_*_compact on handle h"""
    n = a[11] if paired else a[6]
    args = [PU._addr(x) for x in a]
    tail = args[12:17] + [a[17]] if paired else args[7:10]
    head = args[1:11] if paired else args[1:6]
    f = L.h2g_sam_plan_paired_compact if paired else L.h2g_sam_plan_unpaired_compact
    f.argtypes = [vp] * (len(head) + 1) + [sz] + [vp] * (5 if paired else 3) + ([C.c_uint32] if paired else []) + [vp, sz, C.POINTER(sz), vp, sz, C.POINTER(sz), vp]
    nl, na = sz(0), sz(0)
    ends = np.zeros(max(n, 1), dtype=np.uint64)
    rc = f(h, *head, n, *tail, None, 0, C.byref(nl), None, 0, C.byref(na), ends.ctypes.data)
    if rc != 0 and nl.value == 0 and na.value == 0:
        return rc, None, None, None
    lines = np.zeros(max(nl.value, 1), dtype=api.SAM_LINE_DTYPE)
    aux = np.zeros(max(na.value, 1), dtype=np.uint8)
    if rc != 0:
        rc = f(h, *head, n, *tail, lines.ctypes.data, nl.value, C.byref(nl), aux.ctypes.data, na.value, C.byref(na), ends.ctypes.data)
        assert rc == 0, rc
    return 0, lines[:nl.value], aux[:na.value], ends[:n]


def check_split(L, base, log, paired, a, h_whole, h_split, note=True, opts=None):
    """plan_*_compact on h_whole against split_host on h_split (both fresh twins in the state the format call's handle was in): everything equal, classes == predicate.
    -> (classes, reasons), or None when both refuse"""
    n = a[11] if paired else a[6]
    before = PU.summary(L, h_split)
    prc, lines, aux, ends = plan_whole(L, h_whole, paired, a)
    src, l2, a2, e2, cls = split_host(L, h_split, paired, a)
    if prc != 0:
        assert src != 0 and PU.summary(L, h_split) == before
        return None
    assert src == 0
    assert l2.tobytes() == lines.tobytes(), "descriptors differ: line %d" % next(j for j in range(min(len(l2), len(lines))) if l2[j:j + 1].tobytes() != lines[j:j + 1].tobytes())
    assert a2.tobytes() == aux.tobytes() and (e2 == ends).all()
    assert PU.summary(L, h_split) == PU.summary(L, h_whole)
    assert PU.novel_text(L, h_split) == PU.novel_text(L, h_whole) and PU.take_novel(L, h_split) == PU.take_novel(L, h_whole)
    o = opts if opts is not None else opts_from_log(base, log)
    args = [PU._addr(x) for x in a]
    if paired:
        bo1 = np.ctypeslib.as_array((C.c_uint64 * (n + 1)).from_address(args[14])); bo2 = np.ctypeslib.as_array((C.c_uint64 * (n + 1)).from_address(args[16]))
        raw1 = C.string_at(args[13], int(bo1[n])) if not isinstance(args[13], bytes) else args[13]
        raw2 = C.string_at(args[15], int(bo2[n])) if not isinstance(args[15], bytes) else args[15]
        res = (api.PairResult * max(n, 1)).from_address(args[12])
        want, why = predicate_paired(res, raw1, bo1, raw2, bo2, n, o)
    else:
        bo = np.ctypeslib.as_array((C.c_uint64 * (n + 1)).from_address(args[9]))
        raw = C.string_at(args[8], int(bo[n])) if not isinstance(args[8], bytes) else args[8]
        res = (api.ReadResult * max(n, 1)).from_address(args[7])
        want, why = predicate_unpaired(res, raw, bo, n, o)
    assert list(cls) == want, "class bytes differ from the predicate: read %d, library %d, predicate %d (%s)" % next((i, cls[i], want[i], why[i]) for i in range(n) if cls[i] != want[i])
    if note:
        COVER["classes"].update(want); COVER["reasons"].update(w for w in why if w); COVER["calls"] += 1; COVER["reads"] += n; COVER["plain"] += sum(1 for c in want if c)
    return want, why


class SplitCheckLib(PU.PlanCheckLib):
    """PlanCheckLib's bookkeeping of handles and setter calls; the check at a format_*_compact call is the split planner's"""
    def _call(self, name, real, a):
        if name not in ("h2g_sam_format_unpaired_compact", "h2g_sam_format_paired_compact"):
            return PU.PlanCheckLib._call(self, name, real, a)
        st = self._state.get(PU._val(a[0])) if a and a[0] is not None else None
        if st is None:
            return real(*a)
        paired = "unpaired" not in name
        nargs = 18 if paired else 10
        tw, tw2 = self._twin(st), self._twin(st)
        rc = real(*a)
        st["formats"] += 1
        used = a[nargs + 2]._obj.value
        try:
            if rc != 0 and not (used == 0 or used <= a[nargs + 1]):
                return rc                                             # (a text capacity that was too small is the caller's business)
            r = check_split(self._L, st["base"], st["log"], paired, a[:nargs], tw, tw2)
            assert (r is None) == (rc != 0)
        finally:
            self._L.h2g_sam_close(tw); self._L.h2g_sam_close(tw2)
        return rc
