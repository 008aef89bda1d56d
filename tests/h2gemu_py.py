"""ctypes binding of tests/emul/libh2gemu.so — host instantiation of the device item functions (tests only)."""
import ctypes as C
import os
import subprocess

import numpy as np

from hisat2_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))


def flat_reads(reads, pad=0):
    """a list of read arrays of any lengths (or an (n, L) array) -> (codes u8 with `pad` zero bytes behind them, offsets u32).  pad=8 for second mates: they
    are read in place, and the word-wise readers may touch a few bytes past the last read"""
    lst = [np.asarray(r, dtype=np.uint8) for r in reads]
    return np.concatenate(lst + [np.zeros(pad, np.uint8)]), np.concatenate([[0], np.cumsum([len(r) for r in lst])]).astype(np.uint32)


def name_blob(names):
    """read names -> (their bytes back to back, offsets u32)"""
    return "".join(names).encode(), np.concatenate([[0], np.cumsum([len(q) for q in names])]).astype(np.uint32)


_vp, _u32, _sz, _cp = C.c_void_p, C.c_uint32, C.c_size_t, C.c_char_p
_PAIRS = [_vp, _vp, _cp, _vp, _cp, _vp]          # codes2, offs2, names1, noffs1, names2, noffs2 (Emu._pair_args)
# every entry point that takes the handle first: the arguments behind it.  Symbols a library does not have (tests/emul_spl, tests/dense_sa, tests/dense_lsa add
# theirs) are skipped
_ARGTYPES = {
    "set_reads": [_vp, _vp, _vp, _sz], "set_mate_quals": [_vp, _sz], "set_bowtie2_dp": [_u32], "rank": [_vp, _vp, _sz, _vp], "fm_search": [_vp, _sz, _u32, _vp],
    "sa_resolve": [_vp, _sz, _u32, _vp, _vp], "sw_align": [_vp, _sz, _vp], "adjust_with_alt": [_vp, _sz, _u32, _vp, _vp],
    "sa_resolve_graph": [_vp, _vp, _sz, _u32, _vp, _vp], "graph_lf": [_vp, _sz, _u32, _vp, _vp], "local_graph_lf": [_vp, _sz, _u32, _vp, _vp],
    "fm_search_graph": [_vp, _sz, _u32, _u32, _vp, _vp], "extend": [_vp, _vp, _sz, _vp], "seed_extend": [_u32, _u32, _vp],
    "align": [_u32, _cp, _vp, _vp, _vp], "align_abi": [_u32, _cp, _vp, _vp, _vp, _u32, _vp, _u32, C.POINTER(_u32)], "align_pairs": [_u32] + _PAIRS + [_vp, _vp, _vp],
    "fast_check": _PAIRS + [_vp, _vp, _u32, _vp], "fast_check_spl": _PAIRS + [_vp, _vp, _u32, _vp, _vp], "pairs_overflow_check": _PAIRS + [_u32, _u32, _vp],
    "pair_trips": _PAIRS + [_vp, _sz, _vp],
    "dense_build": [], "dense_attach": [_u32], "dense_check": [_vp], "dense_digest": _PAIRS + [_vp],
    "lsa_build": [], "lsa_attach": [_u32], "lsa_check": [_vp], "lsa_digest": _PAIRS + [_u32, _vp],
}


class Emu:
    def __init__(self, base, variant=""):
        """variant "" = the shipped kernel's configuration; "am" = alignMate in the fast path (tests/emul/Makefile)"""
        subprocess.run(["make", "-s", "-j2", "-C", os.path.join(HERE, "emul")], check=True)
        self.L = C.CDLL(os.environ.get("H2GEMU_LIB") or os.path.join(HERE, "emul", "libh2gemu%s.so" % ("_" + variant if variant else "")))
        self.L.h2gemu_load.argtypes = [_cp, C.POINTER(_vp)]
        for name, args in _ARGTYPES.items():
            f = getattr(self.L, "h2gemu_" + name, None)
            if f is not None:
                f.argtypes, f.restype = [_vp] + args, None
        for name in ("ghit_edits", "dense_sat", "lsa_sat"):          # no handle: a constant of the build
            f = getattr(self.L, "h2gemu_" + name, None)
            if f is not None:
                f.argtypes, f.restype = [], _u32
                setattr(self, name, f)
        self.h = _vp()
        rc = self.L.h2gemu_load(base.encode(), C.byref(self.h))
        assert rc == 0, rc
        for name in ("dense_build", "dense_attach", "lsa_build", "lsa_attach"):      # the derived harnesses' switches, as methods where the library has them
            f = getattr(self.L, "h2gemu_" + name, None)
            if f is not None:
                setattr(self, name, lambda *a, _f=f: _f(self.h, *a))
        self.n_reads = 0

    # ---- go() over the resident batch.  reads2: the second mates (a list of arrays; None = unpaired); names / names2: default "0", "1", ...
    def load_reads(self, reads, quals=None):
        """set_reads for a list of read arrays; quals: flat phred+33 bytes over the same offsets (FASTQ), None = FASTA ('I')"""
        self.set_reads(*flat_reads(reads), quals)

    def set_mate_quals(self, quals):
        """flat phred+33 bytes of the second mates handed to align_pairs / fast_check; they go with the reads set last"""
        q = np.ascontiguousarray(quals, dtype=np.uint8)
        self.L.h2gemu_set_mate_quals(self.h, q.ctypes.data, q.size)

    def _pair_args(self, reads2, names, names2=None):
        """-> the six arguments every paired entry point takes, and the arrays they point into (to be kept until the call returns)"""
        nb, no = name_blob([str(i) for i in range(self.n_reads)] if names is None else names)
        if reads2 is None:
            return (None, None, nb, no.ctypes.data, None, None), (no,)
        c2, o2 = flat_reads(reads2, pad=8)
        nb2, no2 = (nb, no) if names2 is None else name_blob(names2)
        return (c2.ctypes.data, o2.ctypes.data, nb, no.ctypes.data, nb2, no2.ctypes.data), (no, c2, o2, no2)

    def align(self, names=None, no_spliced=1, rec_type=None):
        """-> (ReadOut per read, records: sam_util.AL_MAX_RESULTS of rec_type per read — default sam_util.AlnRec, the 32-edit libraries' layout)"""
        import sam_util as SU
        n = self.n_reads
        args, keep = self._pair_args(None, names)
        outs, recs = (SU.ReadOut * n)(), ((rec_type or SU.AlnRec) * (n * SU.AL_MAX_RESULTS))()
        self.L.h2gemu_align(self.h, no_spliced, args[2], args[3], outs, recs)
        return outs, recs

    def align_pairs(self, reads2, names=None, names2=None, no_spliced=1, rec_type=None):
        """-> (PairOut per pair, records of the first mates, of the second mates: as align's)"""
        import pe_sink as PS
        import sam_util as SU
        n = self.n_reads
        args, keep = self._pair_args(reads2, names, names2)
        T = rec_type or SU.AlnRec
        outs, r1, r2 = (PS.PairOut * n)(), (T * (n * SU.AL_MAX_RESULTS))(), (T * (n * SU.AL_MAX_RESULTS))()
        self.L.h2gemu_align_pairs(self.h, no_spliced, *args, outs, r1, r2)
        return outs, r1, r2

    def align_abi(self, names=None, ledits_cap=1 << 18, no_spliced=1):
        """go() with the rows of the C ABI (api.ALN_CAP per read) and a long-edit area of ledits_cap edits -> (ReadOut per read, rows, area, edits written to it)"""
        import sam_util as SU
        n = self.n_reads
        args, keep = self._pair_args(None, names)
        outs, rows, led, used = (SU.ReadOut * n)(), (api.AlnRes * (n * api.ALN_CAP))(), (api.Edit * ledits_cap)(), C.c_uint32(0)
        self.L.h2gemu_align_abi(self.h, no_spliced, args[2], args[3], outs, rows, api.ALN_CAP, led, ledits_cap, C.byref(used))
        return outs, rows, led, used.value

    def fast_check(self, reads2=None, names=None, spliced=False, cap=64):
        """h2gemu_fast_check, or (spliced, tests/emul_spl) h2gemu_fast_check_spl -> (stats u64: [0] completed, [1] mismatching, [2 + why] bails; the first
        mismatching ids; done flag per read) + (the machine's result holds a splice edit, per read) when spliced"""
        n = self.n_reads
        args, keep = self._pair_args(reads2, names)
        stats, bad, done = np.zeros(64, dtype=np.uint64), np.zeros(cap, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
        if not spliced:
            self.L.h2gemu_fast_check(self.h, *args, stats.ctypes.data, bad.ctypes.data, cap, done.ctypes.data)
            return stats, bad, done
        spl = np.zeros(n, dtype=np.uint8)
        self.L.h2gemu_fast_check_spl(self.h, *args, stats.ctypes.data, bad.ctypes.data, cap, done.ctypes.data, spl.ctypes.data)
        return stats, bad, done, spl

    def pairs_overflow_check(self, reads2, slots, ovf_cap, names=None):
        """-> [pairs kept in the overflow area, pairs with a wrong record, pairs flagged (area full), records the area holds at the end]"""
        args, keep = self._pair_args(reads2, names)
        stats = np.zeros(4, dtype=np.uint64)
        self.L.h2gemu_pairs_overflow_check(self.h, *args, slots, ovf_cap, stats.ctypes.data)
        return stats

    def pair_trips(self, reads2, ids, names=None):
        """-> (len(ids), 16) u32: the machine's requests by primitive for each read id, [15] = control phases"""
        args, keep = self._pair_args(reads2, names)
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        out = np.zeros((len(ids), 16), dtype=np.uint32)
        self.L.h2gemu_pair_trips(self.h, *args, ids.ctypes.data, len(ids), out.ctypes.data)
        return out

    def table_check(self, kind, nout):
        """h2gemu_dense_check / h2gemu_lsa_check (kind "dense" / "lsa") -> its nout counters"""
        out = np.zeros(nout, dtype=np.uint64)
        getattr(self.L, f"h2gemu_{kind}_check")(self.h, out.ctypes.data)
        return out

    def table_digest(self, kind, reads2=None, midwalk=None, names=None):
        """h2gemu_dense_digest / h2gemu_lsa_digest (midwalk: the latter's switch) -> u64[5]: machine hash, fast hash, completed, nsteps, (lsa) reads switched"""
        args, keep = self._pair_args(reads2, names)
        out = np.zeros(5, dtype=np.uint64)
        getattr(self.L, f"h2gemu_{kind}_digest")(self.h, *args, *(() if midwalk is None else (midwalk,)), out.ctypes.data)
        return out

    def set_reads(self, codes, offs, quals=None):
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint32)
        if quals is not None:
            quals = np.ascontiguousarray(np.frombuffer(quals, dtype=np.uint8) if isinstance(quals, (bytes, bytearray)) else quals, dtype=np.uint8)
            assert quals.size == codes.size
        self._keep = (codes, offs, quals)
        self.n_reads = len(offs) - 1
        self.L.h2gemu_set_reads(self.h, codes.ctypes.data, offs.ctypes.data, quals.ctypes.data if quals is not None else None, self.n_reads)

    def rank(self, rows, cs):
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        cs = np.ascontiguousarray(cs, dtype=np.uint8)
        out = np.empty(len(rows), dtype=np.uint32)
        self.L.h2gemu_rank(self.h, rows.ctypes.data, cs.ctypes.data, len(rows), out.ctypes.data)
        return out

    def fm_search(self, queries, khits=5):
        n = len(queries)
        q = (api.FmQuery * n)(*queries)
        out = (api.FmHit * n)()
        self.L.h2gemu_fm_search(self.h, q, n, khits, out)
        return out

    def sw_align(self, queries, repeats=1):
        n = len(queries)
        q = (api.SwQuery * n)(*queries)
        out = (api.SwResult * n)()
        self.L.h2gemu_sw_align(self.h, q, n, out)
        return out, 0.0

    def adjust_with_alt(self, queries, cap=8):
        n = len(queries)
        q = (api.AdjustQuery * n)(*queries)
        hits = (api.GHit * (n * cap))()
        nh = (C.c_uint32 * n)()
        self.L.h2gemu_adjust_with_alt(self.h, q, n, cap, hits, nh)
        return hits, nh

    def local_graph_lf(self, q6, k=10):
        """q6: (n, 6) uint32 rows {single, tidx, toff, top, bot, c} -> mapGLF / mapGLF1 on the covering local graph index"""
        q6 = np.ascontiguousarray(q6, dtype=np.uint32)
        n = len(q6)
        res = (api.GlfResult * n)()
        ie = (api.IEdges * n)()
        self.L.h2gemu_local_graph_lf(self.h, q6.ctypes.data, n, k, res, ie)
        return res, ie

    def sa_resolve_graph(self, queries, iedges, cap=24):
        n = len(queries)
        q = (api.GsaQuery * n)(*queries)
        ie = (api.IEdges * n)(*iedges)
        co = (api.Coord * (n * cap))()
        res = (api.SaResult * n)()
        self.L.h2gemu_sa_resolve_graph(self.h, q, ie, n, cap, co, res)
        return co, res

    def graph_lf(self, queries, k=10):
        n = len(queries)
        q = (api.GlfQuery * n)(*queries)
        res = (api.GlfResult * n)()
        ie = (api.IEdges * n)()
        self.L.h2gemu_graph_lf(self.h, q, n, k, res, ie)
        return res, ie

    def fm_search_graph(self, queries, khits=10, kseeds=20):
        n = len(queries)
        q = (api.FmQuery * n)(*queries)
        out = (api.FmHit * n)()
        ie = (api.IEdges * n)()
        self.L.h2gemu_fm_search_graph(self.h, q, n, khits, kseeds, out, ie)
        return out, ie

    def sa_resolve(self, queries, cap=16):
        n = len(queries)
        q = (api.SaQuery * n)(*queries)
        co = (api.Coord * (n * cap))()
        res = (api.SaResult * n)()
        self.L.h2gemu_sa_resolve(self.h, q, n, cap, co, res)
        return co, res

    def extend(self, hits, args):
        n = len(hits)
        h = (api.GHit * n)(*hits)
        a = (api.ExtArgs * n)(*args)
        res = (api.ExtResult * n)()
        self.L.h2gemu_extend(self.h, h, a, n, res)
        return h, res

    def seed_extend(self, pseudogeneStop=0, khits=5):
        out = np.zeros(self.n_reads * 2, dtype=api.SEED_RESULT_DTYPE)
        self.L.h2gemu_seed_extend(self.h, pseudogeneStop, khits, out.ctypes.data)
        return out
