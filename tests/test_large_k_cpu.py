"""The concordant-list trailer of the compact paired layout (include/h2g.h H2G_PAIR_TRAILER_TAG): an XL run's pair with more concordant pairings
than h2g_pair_result carries, or with a mate list longer than 255 records, brings its whole list behind mate 1's records.  Synthetic compact
records go through h2g_sam_format_paired_compact and every printed line is compared with the Python restatement of the paired sink
(tests/pe_sink.py).  A stream without trailers prints what the dense formatter prints."""
import ctypes as C
import gzip
import os
import shutil

import numpy as np
import pytest

import pe_sink as PS
import sam_lines as SL
from hisat2_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
TAG = 0x52494150
RDLEN = 101


@pytest.fixture(scope="module")
def g1(tmp_path_factory):
    t = tmp_path_factory.mktemp("g1")
    for k in range(1, 9):
        src = os.path.join(HERE, "golden", "g1.%d.ht2.gz" % k)
        with gzip.open(src) as f, open(t / ("g1.%d.ht2" % k), "wb") as o:
            shutil.copyfileobj(f, o)
    return str(t / "g1")


def _rec(fw, toff, score):
    r = api.AlnRes()
    r.fw, r.tidx, r.toff, r.len, r.trim5, r.trim3, r.nedits, r.splicescore, r.score = fw, 0, toff, RDLEN, 0, 0, 0, 0, score
    return r


def _compact(recs):
    return b"".join(bytes(r)[:40] for r in recs)       # no edits: 40 bytes each


def _trailer(pairs):
    b = bytearray(40)
    b[4:8] = len(pairs).to_bytes(4, "little")
    b[24:28] = TAG.to_bytes(4, "little")
    for i, j in pairs:
        b += (i | (j << 16)).to_bytes(4, "little")
    if len(pairs) & 1:
        b += b"\0" * 4
    return bytes(b)


class _Out:      # what pe_sink.finish_pair reads of a pair's result, with the whole concordant list
    def __init__(self, nres, pairs, rnd):
        self.nres, self.npairs, self.rnd_state = nres, len(pairs), rnd
        self.pair_i, self.pair_j = [p[0] for p in pairs], [p[1] for p in pairs]


def make_stream(rng, n, trailers):
    """n pairs of synthetic lists: (m1 records, m2 records, concordant pairs, rnd).  trailers: every other pair has more than 32 pairings and
    its mate-1 list more than 255 records"""
    out = []
    for i in range(n):
        big = trailers and i % 2 == 0
        n1 = int(rng.integers(256, 300)) if big else int(rng.integers(1, 20))
        n2 = int(rng.integers(40, 80)) if big else int(rng.integers(1, 20))
        r1 = [_rec(1, 1000 + 37 * k, -6 * int(rng.random() < 0.15)) for k in range(n1)]
        r2 = [_rec(0, 1200 + 37 * k, -6 * int(rng.random() < 0.15)) for k in range(n2)]
        npairs = int(rng.integers(33, 200)) if big else int(rng.integers(0, min(n1 * n2, 32) + 1))
        pairs = []
        for k in range(npairs):
            a = int(rng.integers(200, n1)) if big and k % 3 == 0 else int(rng.integers(0, n1))
            pairs.append((a, int(rng.integers(0, n2))))
        out.append((r1, r2, pairs, int(rng.integers(0, 1 << 32))))
    return out


def run_compact(L, base, stream, khits, with_trailers):
    n = len(stream)
    rng = np.random.default_rng(7)
    m1 = [rng.integers(0, 4, size=RDLEN, dtype=np.uint8) for _ in range(n)]
    m2 = [rng.integers(0, 4, size=RDLEN, dtype=np.uint8) for _ in range(n)]
    c1, o1 = SL.flat(m1)
    c2, o2 = SL.flat(m2)
    names = ["p%d" % i for i in range(n)]
    nb, no = SL.flat_names(names)
    res = (api.PairResult * n)()
    rec1, rec2 = bytearray(), bytearray()
    b1, b2 = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
    for i, (r1, r2, pairs, rnd) in enumerate(stream):
        p = res[i]
        p.nres[0], p.nres[1], p.npairs, p.rnd_state = len(r1), len(r2), len(pairs), rnd
        for k in range(min(len(pairs), api.PAIR_CAP)):
            p.pair_i[k], p.pair_j[k] = pairs[k][0] & 0xFF, pairs[k][1] & 0xFF
        rec1 += _compact(r1)
        if with_trailers and (len(pairs) > api.PAIR_CAP or any(a > 255 or b > 255 for a, b in pairs)):
            rec1 += _trailer(pairs)
        rec2 += _compact(r2)
        b1[i + 1], b2[i + 1] = len(rec1), len(rec2)
    h = C.c_void_p()
    assert L.h2g_sam_open(base.encode(), C.byref(h)) == 0
    L.h2g_sam_format_paired_compact.argtypes = [C.c_void_p] + [C.c_void_p] * 10 + [C.c_size_t] + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_size_t,
                                                                                                         C.POINTER(C.c_size_t)]
    cap = 1 << 26
    buf = C.create_string_buffer(cap)
    used = C.c_size_t(0)
    r1b, r2b = bytes(rec1) + b"\0" * 8, bytes(rec2) + b"\0" * 8
    rc = L.h2g_sam_format_paired_compact(h, c1.ctypes.data, o1.ctypes.data, None, nb, no.ctypes.data, c2.ctypes.data, o2.ctypes.data, None, nb,
                                         no.ctypes.data, n, C.addressof(res), r1b, b1.ctypes.data, r2b, b2.ctypes.data, khits, buf, cap, C.byref(used))
    dense = None
    if not with_trailers:        # the same records through the dense formatter
        a1 = (api.AlnRes * max(1, sum(len(s[0]) for s in stream)))()
        a2 = (api.AlnRes * max(1, sum(len(s[1]) for s in stream)))()
        d1, d2 = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
        for i, (r1, r2, _, _) in enumerate(stream):
            for k, r in enumerate(r1):
                a1[int(d1[i]) + k] = r
            for k, r in enumerate(r2):
                a2[int(d2[i]) + k] = r
            d1[i + 1], d2[i + 1] = d1[i] + len(r1), d2[i] + len(r2)
        h2 = C.c_void_p()
        assert L.h2g_sam_open(base.encode(), C.byref(h2)) == 0
        buf2 = C.create_string_buffer(cap)
        u2 = C.c_size_t(0)
        assert L.h2g_sam_format_paired_dense(h2, c1.ctypes.data, o1.ctypes.data, None, nb, no.ctypes.data, c2.ctypes.data, o2.ctypes.data, None, nb,
                                             no.ctypes.data, n, C.addressof(res), a1, d1.ctypes.data, a2, d2.ctypes.data, khits, buf2, cap, C.byref(u2)) == 0
        L.h2g_sam_close(h2)
        dense = buf2.raw[:u2.value].decode().splitlines()
    L.h2g_sam_close(h)
    assert rc == 0, rc
    return buf.raw[:used.value].decode().splitlines(), dense


def fields(line):
    f = line.split("\t")
    a = [x for x in f[11:] if x.startswith("AS:i:")]
    return (int(f[1]), f[2], int(f[3]), f[5], int(a[0][5:]) if a else None)


def expected(stream, refname, khits):
    want = []
    for r1, r2, pairs, rnd in stream:
        out = _Out((len(r1), len(r2)), pairs, rnd)
        want += PS.finish_pair(out, r1, r2, 0, [refname], (RDLEN, RDLEN), khits=khits)
    return want


def _refname(base):
    L = SL.load_sam_lib()
    h = C.c_void_p()
    assert L.h2g_sam_open(base.encode(), C.byref(h)) == 0
    hb = C.create_string_buffer(1 << 16)
    nh = L.h2g_sam_header(h, b"", hb, 1 << 16)
    L.h2g_sam_close(h)
    sq = [l for l in hb.raw[:nh].decode().splitlines() if l.startswith("@SQ")]
    return sq[0].split("\t")[1][3:]


@pytest.mark.parametrize("khits", [100, 128, 5])
def test_trailer_lists_equal_the_sink(g1, khits):
    L = SL.load_sam_lib()
    stream = make_stream(np.random.default_rng(100 + khits), 40, trailers=True)
    assert max(len(s[2]) for s in stream) > 32 and max(len(s[0]) for s in stream) > 255
    got, _ = run_compact(L, g1, stream, khits, True)
    want = expected(stream, _refname(g1), khits)
    assert len(got) == len(want)
    assert [fields(l) for l in got] == want
    if khits > 32:
        assert max(sum(1 for l in got if l.startswith("p%d\t" % i) and int(l.split("\t")[1]) & 0x42 == 0x42) for i in range(0, 40, 2)) > 32


def test_stream_without_trailers_unchanged(g1):
    L = SL.load_sam_lib()
    stream = make_stream(np.random.default_rng(5), 60, trailers=False)
    got, dense = run_compact(L, g1, stream, 10, False)
    assert got == dense
    assert [fields(l) for l in got] == expected(stream, _refname(g1), 10)


def test_trailer_must_end_mate_1(g1):
    """a trailer that is not the last entry of a pair's mate-1 bytes is refused (H2G_ERR_ARG)"""
    L = SL.load_sam_lib()
    stream = make_stream(np.random.default_rng(9), 2, trailers=True)
    r1, r2, pairs, _ = stream[0]
    # a trailer in mate 2's bytes
    res = (api.PairResult * 1)()
    res[0].nres[0], res[0].nres[1], res[0].npairs = len(r1), len(r2), len(pairs)
    rec1 = _compact(r1) + b"\0" * 8
    rec2 = _compact(r2) + _trailer(pairs) + b"\0" * 8
    b1 = np.array([0, len(rec1) - 8], dtype=np.uint64)
    b2 = np.array([0, len(rec2) - 8], dtype=np.uint64)
    c, o = SL.flat([np.zeros(RDLEN, dtype=np.uint8)])
    nb, no = SL.flat_names(["x"])
    h = C.c_void_p()
    assert L.h2g_sam_open(g1.encode(), C.byref(h)) == 0
    L.h2g_sam_format_paired_compact.argtypes = [C.c_void_p] + [C.c_void_p] * 10 + [C.c_size_t] + [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p, C.c_size_t,
                                                                                                         C.POINTER(C.c_size_t)]
    buf = C.create_string_buffer(1 << 20)
    used = C.c_size_t(0)
    rc = L.h2g_sam_format_paired_compact(h, c.ctypes.data, o.ctypes.data, None, nb, no.ctypes.data, c.ctypes.data, o.ctypes.data, None, nb, no.ctypes.data, 1,
                                         C.addressof(res), rec1, b1.ctypes.data, rec2, b2.ctypes.data, 100, buf, 1 << 20, C.byref(used))
    L.h2g_sam_close(h)
    assert rc != 0
