"""The line plan against the formatter it was cut from (include/h2g.h, h2g_sam_plan_*_compact + h2g_sam_text_from_plan_host): a stand-in for the library object
of sam_lines.load_sam_lib() that lets every call through and, at each h2g_sam_format_*_compact call, also runs the same arguments through the planner and the
emitter's host instantiation on twin handles set up by replaying the setter calls the handle under test has seen.  Whatever helper formats records through
sam_lines (test_sam_lines, test_long_edits_cpu, temp_splice, ...) is checked without a change to it."""
import ctypes as C
import hashlib

import numpy as np

from hisat2_amd import api

vp, sz = C.c_void_p, C.c_size_t
REPLAYED = ("h2g_sam_set_", "h2g_sam_add_", "h2g_sam_collect_")
STATS = {"calls": 0, "lines": 0, "whole": 0, "aux_lines": 0, "simple": 0, "refused": 0, "novel": 0}
DIGESTS = None            # a list: every h2g_sam_format_* call through a PlanCheckLib appends format_digests() of itself (test_sam_plan_cpu.text_digests)


def _val(h):
    return h.value if hasattr(h, "value") else int(h)


def _addr(x):
    if x is None:
        return None
    if isinstance(x, (bytes, int)):
        return x
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return C.addressof(x)


def summary(L, h):
    L.h2g_sam_summary.argtypes = [vp, vp, sz]
    L.h2g_sam_summary.restype = sz
    b = C.create_string_buffer(8192)
    n = L.h2g_sam_summary(h, b, 8192)
    return b.raw[:n]


def take_novel(L, h):
    L.h2g_sam_take_novel_sites.argtypes = [vp, vp, sz]
    L.h2g_sam_take_novel_sites.restype = sz
    n = L.h2g_sam_take_novel_sites(h, None, 0)
    a = (api.SpliceSite * max(1, n))()
    assert L.h2g_sam_take_novel_sites(h, a, n) == n
    return bytes(a)[:n * C.sizeof(api.SpliceSite)]


def novel_text(L, h):
    L.h2g_sam_novel_splice_sites_text.argtypes = [vp, vp, sz]
    L.h2g_sam_novel_splice_sites_text.restype = sz
    n = L.h2g_sam_novel_splice_sites_text(h, None, 0)
    b = C.create_string_buffer(n + 1)
    L.h2g_sam_novel_splice_sites_text(h, b, n)
    return b.raw[:n]


def has_long_record(rec, nbytes):
    """does a compact buffer hold a record beyond MAX_EDITS (whole records back to back, trailers included)"""
    raw = C.string_at(rec, nbytes) if isinstance(rec, int) else bytes(rec[:nbytes])
    at = 0
    while at + 40 <= len(raw):
        ne = int.from_bytes(raw[at + 24:at + 28], "little")
        if ne == 0x52494150:                       # a pair trailer: tidx = the number of pairs
            at += (40 + 4 * int.from_bytes(raw[at + 4:at + 8], "little") + 7) & ~7
            continue
        if ne > api.MAX_EDITS:
            return True
        at += (40 + 12 * ne + 7) & ~7
    return False


def _sha(*parts):
    d = hashlib.sha256()
    for p in parts:
        p = p if isinstance(p, bytes) else repr(p).encode()
        d.update(b"%d:" % len(p))
        d.update(p)
    return d.hexdigest()


def _mem(x, nbytes):
    return b"" if x is None else bytes(x[:nbytes]) if isinstance(x, bytes) else C.string_at(_addr(x), nbytes)


def format_inputs(L, name, a, log):
    """everything a format call reads, as bytes: the handle's header (reference names and lengths) and the setter calls it has seen (`log`, with the long-edit area's
    entries), then every array at the size the call's own counts and offsets give it.  name / a: the h2g_sam_format_* function and its arguments"""
    paired = "unpaired" not in name
    nsets = 2 if paired else 1
    n = a[1 + 5 * nsets]
    rest = a[2 + 5 * nsets:]                                  # res, then the records in the layout the name says
    hb = C.create_string_buffer(1 << 16)
    L.h2g_sam_header.argtypes = [vp, C.c_char_p, vp, sz]
    L.h2g_sam_header.restype = sz
    parts = [name, n, hb.raw[:L.h2g_sam_header(a[0], b"", hb, 1 << 16)]]
    for nm, ar in log:
        if nm == "h2g_sam_set_record_ends":                    # (an output array)
            continue
        if nm == "h2g_sam_set_long_edits":
            parts += [nm, ar[2], _mem(ar[1], ar[2] * C.sizeof(api.Edit))]
        else:
            parts += [nm] + [x if isinstance(x, (int, float, bytes, type(None))) else bytes(x) for x in ar[1:]]
    for m in range(nsets):
        codes, offs, quals, nb, noffs = a[1 + 5 * m:6 + 5 * m]
        o = np.frombuffer(_mem(offs, 4 * (n + 1)), dtype=np.uint32)
        no = np.frombuffer(_mem(noffs, 4 * (n + 1)), dtype=np.uint32)
        parts += [o.tobytes(), _mem(codes, int(o[n])), _mem(quals, int(o[n])), no.tobytes(), _mem(nb, int(no[n]))]
    parts.append(_mem(rest[0], n * C.sizeof(api.PairResult if paired else api.ReadResult)))
    rs, cap = C.sizeof(api.AlnRes), api.PAIR_RES_CAP if paired else api.ALN_CAP
    if name.endswith(("_dense", "_compact")):                  # records, offsets [n + 1] per mate: counted in records / in bytes
        unit = rs if name.endswith("_dense") else 1
        for m in range(nsets):
            bo = np.frombuffer(_mem(rest[2 + 2 * m], 8 * (n + 1)), dtype=np.uint64)
            parts += [bo.tobytes(), _mem(rest[1 + 2 * m], int(bo[n]) * unit)]
    else:
        parts += [_mem(rest[1 + m], n * cap * rs) for m in range(nsets)]
    if paired:
        parts.append(rest[-4])                                # khits
    return parts


def plan_and_text(L, h, paired, a, with_ends=True):
    """a = the arguments of the format call behind the handle, up to khits -> (rc, lines, aux, line_ends, text, line_offs) of plan + host text on handle h"""
    n = a[11] if paired else a[6]
    args = [_addr(x) for x in a]
    tail = args[12:17] + [a[17]] if paired else args[7:10]
    head = args[:11] if paired else args[:6]
    f = L.h2g_sam_plan_paired_compact if paired else L.h2g_sam_plan_unpaired_compact
    f.argtypes = [vp] * len(head) + [sz] + [vp] * (5 if paired else 3) + ([C.c_uint32] if paired else []) + [vp, sz, C.POINTER(sz), vp, sz, C.POINTER(sz), vp]
    nl, na = sz(0), sz(0)
    ends = np.zeros(max(n, 1), dtype=np.uint64)
    rc = f(h, *head[1:], n, *tail, None, 0, C.byref(nl), None, 0, C.byref(na), ends.ctypes.data if with_ends else None)   # sizes only: a capacity error, which counts nothing
    if rc != 0 and nl.value == 0 and na.value == 0:
        return rc, None, None, None, None, None                  # refused (a batch without a line has succeeded above)
    lines = np.zeros(max(nl.value, 1), dtype=api.SAM_LINE_DTYPE)
    aux = np.zeros(max(na.value, 1), dtype=np.uint8)
    if rc != 0:
        rc = f(h, *head[1:], n, *tail, lines.ctypes.data, nl.value, C.byref(nl), aux.ctypes.data, na.value, C.byref(na), ends.ctypes.data if with_ends else None)
        assert rc == 0, rc
    lines, aux = lines[:nl.value], aux[:na.value]
    t = L.h2g_sam_text_from_plan_host
    t.argtypes = [vp] * 11 + [sz, vp, sz, vp, sz, vp, sz, vp, sz, vp, sz, C.POINTER(sz), vp]
    if paired:
        bo1 = (C.c_uint64 * (n + 1)).from_address(args[14]); bo2 = (C.c_uint64 * (n + 1)).from_address(args[16])
        sets, recs = args[1:11], (args[13], int(bo1[n]), args[15], int(bo2[n]))
    else:
        bo = (C.c_uint64 * (n + 1)).from_address(args[9])
        sets, recs = args[1:6] + [None] * 5, (args[8], int(bo[n]), None, 0)
    used = sz(0)
    offs = np.zeros(len(lines) + 1, dtype=np.uint64)
    rc2 = t(h, *sets, n, *recs, lines.ctypes.data, len(lines), aux.ctypes.data, len(aux), None, 0, C.byref(used), None)
    assert (rc2 == 0) == (used.value == 0), rc2
    out = np.zeros(used.value + 16, dtype=np.uint8)
    out[used.value:] = 0xA5
    assert t(h, *sets, n, *recs, lines.ctypes.data, len(lines), aux.ctypes.data, len(aux), out.ctypes.data, used.value, C.byref(used), offs.ctypes.data) == 0
    assert (out[used.value:] == 0xA5).all()
    return 0, lines, aux, ends[:n], out[:used.value].tobytes(), offs


class _Fn:
    """a library function seen through the stand-in: attribute writes (argtypes, restype) reach the real one"""
    def __init__(self, owner, name, real):
        object.__setattr__(self, "_owner", owner); object.__setattr__(self, "_name", name); object.__setattr__(self, "_real", real)

    def __setattr__(self, k, v):
        setattr(self._real, k, v)

    def __getattr__(self, k):
        return getattr(self._real, k)

    def __call__(self, *a):
        return self._owner._call(self._name, self._real, a)


class PlanCheckLib:
    def __init__(self, L):
        self._L = L
        self._fns = {}
        self._state = {}          # handle -> {"base", "log": [(name, args)], "formats": int, "own_ends": bool}

    def __getattr__(self, name):
        real = getattr(self._L, name)
        if not name.startswith("h2g_sam_"):
            return real
        if name not in self._fns:
            self._fns[name] = _Fn(self, name, real)
        return self._fns[name]

    def _twin(self, st):
        h = vp()
        self._L.h2g_sam_open.argtypes = [C.c_char_p, C.POINTER(vp)]
        assert self._L.h2g_sam_open(st["base"], C.byref(h)) == 0
        for name, args in st["log"]:
            getattr(self._L, name)(h, *args[1:])
        return h

    def _format(self, name, real, a, st):
        """the format call itself; with DIGESTS set, also what it read, what it wrote and the handle's summary after it, each as a SHA-256"""
        if DIGESTS is None:
            return real(*a)
        inputs = _sha(*format_inputs(self._L, name, a, st["log"]))
        rc = real(*a)
        out, used = a[-3], a[-1]._obj.value
        text = b"" if rc != 0 else out.raw[:used] if hasattr(out, "raw") else C.string_at(_addr(out), used)
        DIGESTS.append({"call": name, "rc": rc, "inputs": inputs, "text": _sha(text), "summary": _sha(summary(self._L, a[0]))})
        return rc

    def _call(self, name, real, a):
        L = self._L
        if name == "h2g_sam_open":
            rc = real(*a)
            if rc == 0:
                self._state[_val(a[1]._obj)] = {"base": a[0], "log": [], "formats": 0, "own_ends": False}
            return rc
        st = self._state.get(_val(a[0])) if a and a[0] is not None else None
        if st is None:
            return real(*a)
        if name == "h2g_sam_close":
            del self._state[_val(a[0])]
            return real(*a)
        if name.startswith(REPLAYED):
            st["log"].append((name, a))
            if name == "h2g_sam_set_record_ends":
                st["own_ends"] = a[1] is not None
            return real(*a)
        if name not in ("h2g_sam_format_unpaired_compact", "h2g_sam_format_paired_compact"):
            if name.startswith("h2g_sam_format_"):
                st["formats"] += 1
                return self._format(name, real, a, st)
            return real(*a)
        paired = name.endswith("paired_compact") and "unpaired" not in name
        n = a[11] if paired else a[6]
        nargs = 18 if paired else 10
        fresh = st["formats"] == 0
        collect = any(nm == "h2g_sam_collect_novel_sites" and ar[1] for nm, ar in st["log"])
        tw = self._twin(st)                               # (before the call: the state the handle is in now)
        tw_fmt = self._twin(st) if (not fresh or collect) else None
        ends = np.zeros(max(n, 1), dtype=np.uint64)
        if not st["own_ends"]:
            L.h2g_sam_set_record_ends.argtypes = [vp, vp]
            L.h2g_sam_set_record_ends(a[0], ends.ctypes.data)
        rc = self._format(name, real, a, st)
        if not st["own_ends"]:
            L.h2g_sam_set_record_ends(a[0], None)
        st["formats"] += 1
        used = a[nargs + 2]._obj.value
        want = a[nargs].raw[:used] if hasattr(a[nargs], "raw") else C.string_at(a[nargs], used)
        before = summary(L, tw)
        prc, lines, aux, line_ends, text, line_offs = plan_and_text(L, tw, paired, a[:nargs])
        STATS["calls"] += 1
        if rc != 0:
            # a refused batch (malformed bytes): refused by the planner too, and nothing counted.  (A text capacity that was too small is the caller's business.)
            if used == 0 or used <= a[nargs + 1]:
                assert prc != 0 and summary(L, tw) == before
                STATS["refused"] += 1
            L.h2g_sam_close(tw)
            if tw_fmt:
                L.h2g_sam_close(tw_fmt)
            return rc
        assert prc == 0
        assert text == want, "plan + emitter differs from the formatter: " + repr(next((x, y) for x, y in zip(text.split(b"\n"), want.split(b"\n")) if x != y))
        assert int(line_offs[-1]) == len(want) and (np.diff(line_offs.astype(np.int64)) > 0).all()
        if not st["own_ends"] and n:
            assert (line_offs[line_ends.astype(np.int64)] == ends[:n]).all(), "line_ends / line_offs do not reproduce h2g_sam_set_record_ends"
        if tw_fmt is not None:                           # the handle under test has counted other calls: a twin runs the format call
            b2 = C.create_string_buffer(used + 8)
            u2 = sz(0)
            assert real(tw_fmt, *a[1:nargs], b2, used + 8, C.byref(u2)) == 0 and b2.raw[:u2.value] == want
            ref = tw_fmt
        else:
            ref = a[0]
        assert summary(L, tw) == summary(L, ref)
        if collect:
            assert novel_text(L, tw) == novel_text(L, tw_fmt)
            taken = take_novel(L, tw)
            assert taken == take_novel(L, tw_fmt)
            STATS["novel"] += len(taken) // C.sizeof(api.SpliceSite)
            assert take_novel(L, tw) == b"" and summary(L, tw) == summary(L, tw_fmt)
        nwhole = int(((lines["bits"] & api.SAM_LINE_WHOLE_LINE) != 0).sum())
        args = [_addr(x) for x in a[:nargs]]
        if paired:
            long_ = has_long_record(args[13], int((C.c_uint64 * (n + 1)).from_address(args[14])[n])) or has_long_record(args[15], int((C.c_uint64 * (n + 1)).from_address(args[16])[n]))
        else:
            long_ = has_long_record(args[8], int((C.c_uint64 * (n + 1)).from_address(args[9])[n]))
        assert nwhole == 0 or long_, "WHOLE_LINE used without a record beyond MAX_EDITS"
        STATS["lines"] += len(lines); STATS["whole"] += nwhole
        STATS["aux_lines"] += int(((lines["bits"] & api.SAM_LINE_AUX_CIGAR_MDZ) != 0).sum())
        STATS["simple"] += int(((lines["bits"] & (api.SAM_LINE_AUX_CIGAR_MDZ | api.SAM_LINE_WHOLE_LINE)) == 0).sum())
        L.h2g_sam_close(tw)
        if tw_fmt:
            L.h2g_sam_close(tw_fmt)
        return rc
