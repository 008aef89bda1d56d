"""SAM text written on the device (include/h2g.h: h2g_sam_text_unpaired / h2g_sam_text_paired, the kernels k_sam_line_sizes / k_sam_line_write of csrc/h2g_kernels.hip
over the emitter of csrc/h2g_sam_line.h) from a host-made line plan, against h2g_sam_format_*_compact on the same fetch: byte for byte; line_offs monotone and ending
at `used`; the calls' refusals, which launch nothing."""
import ctypes as C
import os

import numpy as np
import pytest

import h2o_py as H
import sam_lines as SL
import sam_plan_util as PU
from hisat2_amd import api, synth

pytestmark = pytest.mark.gpu
vp, sz = C.c_void_p, C.c_size_t


def _handle(L, base, opts=()):
    h = vp()
    L.h2g_sam_open.argtypes = [C.c_char_p, C.POINTER(vp)]
    assert L.h2g_sam_open(base.encode(), C.byref(h)) == 0
    SL._score_min(L, h, list(opts))
    return h


def _flat(reads):
    codes = np.concatenate([np.asarray(r, dtype=np.uint8) for r in reads] + [np.zeros(0, dtype=np.uint8)])
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint32)
    return codes, offs


def _format_paired(L, h, s1, s2, n, res, r1, b1, r2, b2, khits):
    f = L.h2g_sam_format_paired_compact
    f.argtypes = [vp] * 11 + [sz] + [vp] * 5 + [C.c_uint32, vp, sz, C.POINTER(sz)]
    cap = 1200 * n + 8 * int(s1[1][-1] + s2[1][-1]) + 4096
    buf = C.create_string_buffer(cap)
    used = sz(0)
    a = [api._ptr(x) for x in s1 + s2]
    assert f(h, *a, n, res.ctypes.data, r1.ctypes.data, b1.ctypes.data, r2.ctypes.data, b2.ctypes.data, khits, buf, cap, C.byref(used)) == 0
    return buf.raw[:used.value]


def _format_unpaired(L, h, s1, n, res, rec, boffs):
    f = L.h2g_sam_format_unpaired_compact
    f.argtypes = [vp] * 6 + [sz] + [vp] * 3 + [vp, sz, C.POINTER(sz)]
    cap = 3000 * n + 8 * int(s1[1][-1]) + 4096
    buf = C.create_string_buffer(cap)
    used = sz(0)
    assert f(h, *[api._ptr(x) for x in s1], n, res.ctypes.data, rec.ctypes.data, boffs.ctypes.data, buf, cap, C.byref(used)) == 0
    return buf.raw[:used.value]


def _check_offs(text, offs):
    assert int(offs[0]) == 0 and int(offs[-1]) == len(text) and (np.diff(offs.astype(np.int64)) > 0).all()
    assert all(text[int(o) - 1:int(o)] == b"\n" for o in offs[1:])


def _pairs_on_device(base, m1, m2, n1, n2, quals=None, opts=(), keep=False):
    """aligns the pairs, then formats the compact fetch twice: the host formatter (a handle of its own) and plan + device text -> (want, got, lines, ...)"""
    n = len(m1)
    c1, o1 = _flat(m1); c2, o2 = _flat(m2)
    nb1, no1 = api.Stream.pack_names(n1); nb2, no2 = api.Stream.pack_names(n2)
    q1, q2 = (None, None) if quals is None else quals
    ix = api.Index(base, device=0)
    st = api.Stream(ix, max_reads=n, max_bases=max(c1.size, c2.size, 1))
    st.set_reads(c1, o1, q1); st.set_read_names((nb1, no1)); st.set_mates(c2, o2, (nb2, no2), q2)
    p = st.align_params()
    st.align_pairs_run(p)
    res, r1, b1, r2, b2 = st.align_pairs_fetch_compact()
    L = SL.load_sam_lib()
    hf, hp = _handle(L, base, opts), _handle(L, base, opts)
    s1, s2 = (c1, o1, q1, nb1, no1), (c2, o2, q2, nb2, no2)
    want = _format_paired(L, hf, s1, s2, n, res, r1, b1, r2, b2, int(p.khits))
    lines, aux, ends = api.sam_plan_paired(hp.value, *s1, *s2, res, r1, b1, r2, b2, int(p.khits))
    got, offs = st.sam_text_paired(hp.value, lines, aux)
    assert got == want, next((x, y) for x, y in zip(got.split(b"\n"), want.split(b"\n")) if x != y)
    _check_offs(got, offs)
    assert PU.summary(L, hf) == PU.summary(L, hp)
    L.h2g_sam_close(hf)
    if keep:
        return dict(ix=ix, st=st, L=L, h=hp, lines=lines, aux=aux, text=got, offs=offs, sets=(s1, s2), fetch=(res, r1, b1, r2, b2), n=n)
    L.h2g_sam_close(hp); st.close(); ix.close()
    return got, lines


def _golden_pairs(golden_dir):
    _, s1 = H.read_fasta_reads(os.path.join(golden_dir, "reads_pe_1.fa.gz"))
    _, s2 = H.read_fasta_reads(os.path.join(golden_dir, "reads_pe_2.fa.gz"))
    q = [str(i) for i in range(len(s1))]
    return s1, s2, q


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("with_quals", [False, True])
def test_golden_pairs(g1_index, g1s_index, golden_dir, graph, with_quals):
    """the golden pairs on the linear index and on its SNP graph (Zs:Z among the lines), without qualities ('I') and with random ones"""
    m1, m2, q = _golden_pairs(golden_dir)
    if graph:      # the golden pairs follow the reference haplotype: pairs cut from the alternate one (every variant of g1s.snp applied) bring the Zs:Z lines
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
    got, lines = _pairs_on_device(g1s_index if graph else g1_index, m1, m2, q, q, quals=quals)
    simple = int(((lines["bits"] & (api.SAM_LINE_AUX_CIGAR_MDZ | api.SAM_LINE_WHOLE_LINE)) == 0).sum())
    assert simple > len(lines) // 2 and int((lines["bits"] & api.SAM_LINE_WHOLE_LINE).sum()) == 0
    if graph:
        assert got.count(b"\tZs:Z:") > 0
    if not with_quals:
        assert all(set(l.split(b"\t")[10]) <= {ord("I")} for l in got.split(b"\n")[:50] if l)


def test_unpaired_reads(g1_index, golden_dir):
    names, seqs = H.read_fasta_reads(os.path.join(golden_dir, "reads_se.fa.gz"))
    n = len(seqs)
    codes, offs = _flat(seqs)
    nb, no = api.Stream.pack_names(names)
    ix = api.Index(g1_index, device=0)
    st = api.Stream(ix, max_reads=n, max_bases=codes.size)
    st.set_reads(codes, offs); st.set_read_names((nb, no))
    st.align_run()
    res, rec, boffs = st.align_fetch_compact()
    L = SL.load_sam_lib()
    hf, hp = _handle(L, g1_index), _handle(L, g1_index)
    s1 = (codes, offs, None, nb, no)
    want = _format_unpaired(L, hf, s1, n, res, rec, boffs)
    lines, aux, ends = api.sam_plan_unpaired(hp.value, *s1, res, rec, boffs)
    got, loffs = st.sam_text_unpaired(hp.value, lines, aux)
    assert got == want and len(lines) >= n
    _check_offs(got, loffs)
    # a part of the batch: the fetch of (first, n) is what lines[].read counts from
    first, cnt = 37, 101
    res2, rec2, boffs2 = st.align_fetch_compact(first, cnt)
    s2 = (codes[int(offs[first]):], (offs[first:first + cnt + 1] - offs[first]).astype(np.uint32), None, nb[int(no[first]):], (no[first:first + cnt + 1] - no[first]).astype(np.uint32))
    want2 = _format_unpaired(L, hf, s2, cnt, res2, rec2, boffs2)
    lines2, aux2, _ = api.sam_plan_unpaired(hp.value, *s2, res2, rec2, boffs2)
    got2, _ = st.sam_text_unpaired(hp.value, lines2, aux2)
    assert got2 == want2 and got2 in want
    L.h2g_sam_close(hf); L.h2g_sam_close(hp); st.close(); ix.close()


NAMES = ["r", "", "read/1", "read/2", "x/3", "y/4", "two words", " lead", "n" * 254, "m" * 255, "k" * 256, "q" * 254 + " z", "w" * 255 + " z", "v" * 300, "tab\there/1"]


def test_ragged_and_empty_reads(g1_index, golden_dir):
    """mates of 0, 1, 2 ... 256 bases in every pairing class of tests/ragged_cases.py, under names of 0 to 300 bytes with blanks and mate suffixes"""
    import parity_cases as PC
    import ragged_cases as RC
    contigs = PC.load_contigs(golden_dir)
    minK, ftab = RC.index_params(g1_index)
    m1, m2, labels = RC.make_ragged_pairs(contigs, 8101, 450, minK, ftab)
    n = len(m1)
    n1 = [NAMES[i % len(NAMES)] for i in range(n)]
    n2 = [NAMES[(i + 3) % len(NAMES)] for i in range(n)]
    quals = (RC.seeded_quals(m1, 3), RC.seeded_quals(m2, 4))
    got, lines = _pairs_on_device(g1_index, m1, m2, n1, n2, quals=quals)
    assert any(len(r) == 0 for r in m1 + m2) and got.count(b"\tYF:Z:LN") > 0 and len(lines) >= 2 * n


def test_many_scan_tiles(g1_index, golden_dir):
    """30 011 pairs, about 60 000 lines: the scan of the line sizes spans 29 tiles and more"""
    import parity_cases as PC
    contigs = PC.load_contigs(golden_dir)
    n = 30011
    m1, m2 = synth.make_pairs(contigs, n, 101, 4711, frag_mean=300, frag_sd=30, sub_rate=0.02)
    q = [str(i) for i in range(n)]
    got, lines = _pairs_on_device(g1_index, list(m1), list(m2), q, q)
    assert (len(lines) + 1 + 2047) // 2048 >= 29


def test_refusals_launch_nothing(g1_index, golden_dir):
    """cap one byte short: H2G_ERR_ARG, *used exact, the guard bytes behind cap untouched; a stale fetch (another range fetched since, another batch selected) and
    bad descriptors (read == n, a misaligned rec_off, a pool range past n_aux): H2G_ERR_ARG"""
    m1, m2, q = _golden_pairs(golden_dir)
    k = _pairs_on_device(g1_index, m1[:300], m2[:300], q[:300], q[:300], keep=True)
    st, h, lines, aux, text = k["st"], k["h"], k["lines"], k["aux"], k["text"]
    f = api.lib().h2g_sam_text_paired
    call = lambda ls, ax, out, cap, used, n_aux=None: f(st.h, h, ls.ctypes.data, len(ls), ax.ctypes.data, len(ax) if n_aux is None else n_aux, out.ctypes.data, cap, C.byref(used), None)
    aux_ = np.ascontiguousarray(aux) if len(aux) else np.zeros(1, dtype=np.uint8)
    out = np.full(len(text) + 64, 0xA5, dtype=np.uint8)
    used = sz(0)
    assert call(lines, aux_, out, len(text) - 1, used, len(aux)) == api.H2G_ERR_ARG and used.value == len(text) and (out == 0xA5).all()
    assert call(lines, aux_, out, len(text), used, len(aux)) == 0 and out[:len(text)].tobytes() == text and (out[len(text):] == 0xA5).all()

    def refused(ls, n_aux=len(aux)):
        o = np.full(len(text) + 64, 0xA5, dtype=np.uint8)
        u = sz(0)
        assert call(ls, aux_, o, len(text) + 64, u, n_aux) == api.H2G_ERR_ARG and (o == 0xA5).all()
        assert api.lib().h2g_last_error()

    j = int(np.flatnonzero(lines["rec_off"] != api.SAM_NONE)[0])
    for field, value in (("read", k["n"]), ("rec_off", int(lines["rec_off"][j]) + 4), ("rec_off", 1 << 40), ("mate", 2), ("oref_tidx", 99)):
        ls = lines.copy()
        ls[field][j] = value
        refused(ls)
    ls = lines.copy()
    ls["aux_off"][j], ls["aux_len"][j] = len(aux), 1
    refused(ls)
    ls = lines.copy()                                      # a record offset inside the bytes whose record, read there, does not end inside them
    ls["rec_off"][j] = (int(k["fetch"][2][-1]) - 40) & ~7
    bytes1 = k["fetch"][1]
    ne = int.from_bytes(bytes1[int(ls["rec_off"][j]) + 24:int(ls["rec_off"][j]) + 28].tobytes(), "little")
    if ne > 0:
        refused(ls)
    assert call(lines, aux_, out, len(text), used, len(aux)) == 0           # (the refusals left the fetch in place)
    # stale: another range fetched since; then the matching plan works again; then another batch selected
    st.align_pairs_fetch_compact(0, 10)
    refused(lines)
    st.align_pairs_fetch_compact()
    assert call(lines, aux_, out, len(text), used, len(aux)) == 0 and out[:len(text)].tobytes() == text
    st.select_batch(1)
    refused(lines)
    st.select_batch(0)
    refused(lines)                                          # (the selection itself made the buffers nobody's)
    # the unpaired call on a paired fetch
    fu = api.lib().h2g_sam_text_unpaired
    st.align_pairs_fetch_compact()
    u = sz(0)
    assert fu(st.h, h, lines.ctypes.data, len(lines), aux_.ctypes.data, len(aux), out.ctypes.data, len(out), C.byref(u), None) == api.H2G_ERR_ARG
    k["L"].h2g_sam_close(h); st.close(); k["ix"].close()
