"""SAM lines from a host-made plan (include/h2g.h: h2g_sam_plan_*_compact -> h2g_sam_line descriptors + a byte pool; the emitter of csrc/h2g_sam_line.h instantiated
on the host, h2g_sam_text_from_plan_host) against the formatter the plan was cut from, byte for byte, with the handle's summary, its collected junctions and the
per-read ends.  No device is needed.

Two sources of record sets:
  * every set that tests/test_sam_lines.py and tests/test_long_edits_cpu.py format: their tests run here again with the library object of sam_lines replaced by
    sam_plan_util.PlanCheckLib, which checks plan + text at every h2g_sam_format_*_compact call (those that need oracle/_ref skip without it, as there);
  * synthetic records built here (no reference binary needed): every kind of edit, trims, both strands, a record beyond MAX_EDITS, pairs of every class, and the
    options that reach the emitter's tables."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import sam_lines as SL
import sam_plan_util as PU
import test_long_edits_cpu as _TLE
import test_sam_lines as _TSL
from hisat2_amd import api

vp, sz = C.c_void_p, C.c_size_t


@pytest.fixture(autouse=True)
def _checked_library(monkeypatch):
    real = SL.load_sam_lib
    monkeypatch.setattr(SL, "load_sam_lib", lambda path=None: PU.PlanCheckLib(real(path)))


for _mod in (_TSL, _TLE):
    for _name, _obj in list(vars(_mod).items()):
        if _name.startswith("test_") and callable(_obj):
            globals()["test_plan__" + _name[5:]] = _obj
del _mod, _name, _obj


# ---- synthetic records ---------------------------------------------------------------------------------------------------------------------
def _refs(L, base):
    h = vp()
    L.h2g_sam_open.argtypes = [C.c_char_p, C.POINTER(vp)]
    assert L.h2g_sam_open(base.encode(), C.byref(h)) == 0
    L.h2g_sam_header.argtypes = [vp, C.c_char_p, vp, sz]
    L.h2g_sam_header.restype = sz
    b = C.create_string_buffer(1 << 16)
    nhead = L.h2g_sam_header(h, b"", b, 1 << 16)
    txt = b.raw[:nhead].decode()
    L.h2g_sam_close.argtypes = [vp]
    L.h2g_sam_close(h)
    return [int(l.split("LN:")[1]) for l in txt.splitlines() if l.startswith("@SQ")]


def _record(rng, r, rdlen, reflens, kind, led, snps):
    """fills AlnRes r with a plausible alignment of a read of rdlen >= 40 bases; kind: mm / gap / spl / long"""
    r.fw = int(rng.integers(0, 2))
    r.tidx = int(rng.integers(0, len(reflens)))
    r.len = rdlen
    r.trim5, r.trim3 = (int(rng.integers(0, 4)), int(rng.integers(0, 4))) if rng.random() < 0.3 and kind != "spl" else (0, 0)
    lt = rdlen - r.trim5 - r.trim3
    r.toff = int(rng.integers(0, max(1, reflens[r.tidx] - 3 * rdlen - 2000)))
    r.score = -int(rng.integers(0, 40))
    r.pad = 0
    ne = 40 if kind == "long" else int(rng.integers(0, 7)) if kind == "mm" else int(rng.integers(1, 7))
    ne = min(ne, lt - 4)
    pos = np.sort(rng.choice(np.arange(1, lt - 2), size=ne, replace=False))
    r.nedits = ne
    edits = r.edits
    if kind == "long":
        at = led["n"]
        r.edits[0].pos, r.edits[0].snp = at, 0x4c4f4e47
        edits = (api.Edit * ne).from_address(C.addressof(led["area"]) + at * C.sizeof(api.Edit))
        led["n"] += ne
    special = int(rng.integers(0, ne)) if ne and kind in ("gap", "spl") else -1
    for k in range(ne):
        e = edits[k]
        e.pos, e.snp, e.pad = int(pos[k]), 0xffffffff, 0
        e.chr, e.qchr, e.type = b"ACGT"[int(rng.integers(0, 4))], b"ACGT"[int(rng.integers(0, 4))], 3
        if snps and rng.random() < 0.4:
            e.snp = int(rng.integers(0, snps))
        if k == special and kind == "gap":
            e.type = 1 if rng.random() < 0.5 else 2
            e.snp = 0xffffffff
            if e.type == 1:
                e.qchr = ord("-")
            else:
                e.chr = ord("-")
        elif k == special:
            ln = int(rng.integers(60, 900))
            e.type, e.chr, e.qchr, e.pad = 5, ln & 255, (ln >> 8) & 255, (int(rng.integers(1, 6)) << 4) | (0x80 if rng.random() < 0.5 else 0)
            e.snp = 0x3f000000


NAMES = ["r", "", "read/1", "read/2", "x/3", "y/4", "two words", " lead", "n" * 254, "m" * 255, "k" * 256, "q" * 254 + " z", "w" * 255 + " z", "v" * 300, "tab\there/1"]


def _reads(rng, n, paired_suffix=None):
    lens = [0, 1, 2, 40, 41, 63, 64, 65, 101, 150, 255, 256, 257] + [int(x) for x in rng.integers(40, 160, size=max(0, n - 13))]
    lens = lens[:n]
    reads = [rng.integers(0, 4, size=l).astype(np.uint8) for l in lens]
    for r in reads[5:9]:
        r[::7] = 4
    reads[9][:] = 4                                   # fails --n-ceil
    reads[10][3] = 7                                  # a code above 4 prints N
    names = [NAMES[i % len(NAMES)] if i < 2 * len(NAMES) else "read%d" % i for i in range(n)]
    if paired_suffix:
        names = [nm + paired_suffix if i % 3 == 0 else nm for i, nm in enumerate(names)]
    return reads, names


def _unpaired_case(base, seed, snps=0, n=120):
    rng = np.random.default_rng(seed)
    reflens = _refs(SL.load_sam_lib(), base)
    reads, names = _reads(rng, n)
    res = (api.ReadResult * n)()
    aln = (api.AlnRes * (n * api.ALN_CAP))()
    led = {"area": (api.Edit * 4096)(), "n": 0}
    for i in range(n):
        r = res[i]
        r.best = r.secbest = -(1 << 31)
        if len(reads[i]) < 40 or i == 9 or rng.random() < 0.15:
            continue
        r.nselect = r.nres = int(rng.integers(1, 4))
        for k in range(r.nselect):
            kind = ("mm", "mm", "gap", "spl", "long")[int(rng.integers(0, 5))] if len(reads[i]) >= 60 else "mm"
            _record(rng, aln[i * api.ALN_CAP + k], len(reads[i]), reflens, kind, led, snps)
        sc = sorted((aln[i * api.ALN_CAP + k].score for k in range(r.nselect)), reverse=True)
        r.best, r.best_h2 = sc[0], 0xffff
        if len(sc) > 1:
            r.secbest, r.secbest_h2 = sc[1], 0xffff
    return reads, names, res, aln, (led["area"], led["n"])


def _paired_case(base, seed, snps=0, n=120):
    rng = np.random.default_rng(seed)
    reflens = _refs(SL.load_sam_lib(), base)
    m1, n1 = _reads(rng, n, "/1")
    m2, n2 = _reads(np.random.default_rng(seed + 1), n, "/2")
    m2 = m2[::-1]
    res = (api.PairResult * n)()
    a1 = (api.AlnRes * (n * api.PAIR_RES_CAP))()
    a2 = (api.AlnRes * (n * api.PAIR_RES_CAP))()
    led = {"area": (api.Edit * 16)(), "n": 0}
    for i in range(n):
        pr = res[i]
        pr.rnd_state = int(rng.integers(0, 1 << 32))
        for m, (rd, a) in enumerate(((m1[i], a1), (m2[i], a2))):
            if len(rd) < 60 or (m == 0 and i == 9) or rng.random() < 0.2:
                continue
            pr.nres[m] = int(rng.integers(1, 4))
            for k in range(pr.nres[m]):
                _record(rng, a[i * api.PAIR_RES_CAP + k], len(rd), reflens, ("mm", "mm", "gap", "spl")[int(rng.integers(0, 4))], led, snps)
        if pr.nres[0] and pr.nres[1] and rng.random() < 0.7:
            k = 0
            for x in range(pr.nres[0]):
                for y in range(pr.nres[1]):
                    if rng.random() < 0.6 and k < api.PAIR_CAP:
                        pr.pair_i[k], pr.pair_j[k] = x, y
                        if rng.random() < 0.5:
                            a2[i * api.PAIR_RES_CAP + y].tidx = a1[i * api.PAIR_RES_CAP + x].tidx
                        k += 1
            pr.npairs = k
    return m1, m2, n1, n2, res, a1, a2


OPTION_SETS = [(), ("--secondary", "--omit-sec-seq", "--rg-id", "g", "--rg", "SM:x", "--rna-strandness", "FR"), ("--rna-strandness", "R", "--remove-chrname", "--no-mixed"),
               ("--rna-strandness", "RF", "--no-discordant", "--no-templatelen-adjustment"), ("--rna-strandness", "F", "--add-chrname")]


@pytest.mark.parametrize("opts", OPTION_SETS)
@pytest.mark.parametrize("index,snps", [("g1_index", 0), ("g1s_index", 3)])
def test_synthetic_unpaired_sets(request, index, snps, opts):
    """every edit kind, trims, both strands, empty / short / N-rich reads, names that are cut, a record beyond MAX_EDITS (the only user of WHOLE_LINE), with and
    without qualities: the checked library compares plan + text with the compact formatter inside SL.format_unpaired"""
    base = request.getfixturevalue(index)
    reads, names, res, aln, led = _unpaired_case(base, 9100 + snps, snps)
    before = dict(PU.STATS)
    L = SL.load_sam_lib()
    lines = SL.format_unpaired(L, base, reads, names, res, aln, options=list(opts), long_edits=led)
    quals = np.random.default_rng(5).integers(33, 74, size=sum(len(r) for r in reads)).astype(np.uint8)
    lines_q = SL.format_unpaired(L, base, reads, names, res, aln, quals=quals, options=list(opts), long_edits=led)
    assert len(lines) == len(lines_q) > len(reads)
    d = {k: PU.STATS[k] - before[k] for k in before}
    assert d["calls"] == 2 and d["whole"] > 0 and d["aux_lines"] > 0 and d["simple"] > d["lines"] // 3 and d["refused"] == 0
    if snps:
        assert any("Zs:Z:" in l for l in lines)


@pytest.mark.parametrize("opts", OPTION_SETS + [("-k", "1")])
@pytest.mark.parametrize("index,snps", [("g1_index", 0), ("g1s_index", 3)])
def test_synthetic_paired_sets(request, index, snps, opts):
    """concordant, discordant, mixed and unaligned pairs in one set: YS:i, RNEXT / PNEXT from the opposite record, TLEN, the unaligned mate placed at its partner"""
    base = request.getfixturevalue(index)
    m1, m2, n1, n2, res, a1, a2 = _paired_case(base, 9200 + snps, snps)
    before = dict(PU.STATS)
    khits = 1 if "-k" in opts else 5
    lines = SL.format_paired(SL.load_sam_lib(), base, m1, m2, n1, n2, res, a1, a2, khits, options=[o for o in opts if o not in ("-k", "1")])
    flags = [int(l.split("\t")[1]) for l in lines]
    assert any(f & 2 for f in flags) and any((f & 1) and not (f & 2) and not (f & 12) for f in flags) and any(f & 4 for f in flags)
    assert "--no-mixed" in opts or any((f & 8) and not (f & 4) for f in flags)        # (a mate aligned alone is what --no-mixed leaves out)
    d = {k: PU.STATS[k] - before[k] for k in before}
    assert d["calls"] == 1 and d["whole"] == 0 and d["aux_lines"] > 0 and d["simple"] > 0 and d["lines"] == len(lines)


def _handle(L, base, opts=()):
    h = vp()
    assert L.h2g_sam_open(base.encode(), C.byref(h)) == 0
    SL._score_min(L, h, list(opts))
    return h


def _unpaired_args(reads, names, res, aln):
    codes, offs = SL.flat(reads)
    nb, noffs = SL.flat_names(names)
    n = len(reads)
    rec, boffs = SL.to_compact(aln, np.arange(n) * api.ALN_CAP, [res[i].nselect for i in range(n)])
    return (codes, offs, None, nb, noffs, n, res, rec, boffs)


def test_capacity_errors_count_nothing(g1_index):
    """a descriptor array or a pool that is too small: H2G_ERR_ARG, the needed counts, and the handle as it was — the call after it counts once"""
    L = SL.load_sam_lib()._L
    reads, names, res, aln, led = _unpaired_case(g1_index, 9300)
    h = _handle(L, g1_index)
    L.h2g_sam_set_long_edits.argtypes = [vp, vp, sz]
    L.h2g_sam_set_long_edits(h, led[0], led[1])
    empty = PU.summary(L, h)
    a = _unpaired_args(reads, names, res, aln)
    codes, offs, _, nb, noffs, _, _, rec, boffs = a
    f = L.h2g_sam_plan_unpaired_compact
    f.argtypes = [vp] * 6 + [sz, vp, vp, vp, vp, sz, C.POINTER(sz), vp, sz, C.POINTER(sz), vp]
    call = lambda lines, lc, aux, ac, nl, na: f(h, codes.ctypes.data, offs.ctypes.data, None, nb, noffs.ctypes.data, len(reads), C.addressof(res), rec, boffs.ctypes.data,
                                                 None if lines is None else lines.ctypes.data, lc, C.byref(nl), None if aux is None else aux.ctypes.data, ac, C.byref(na), None)
    nl, na = sz(0), sz(0)
    assert call(None, 0, None, 0, nl, na) == api.H2G_ERR_ARG and nl.value > len(reads) // 2 and na.value > 0
    need_l, need_a = nl.value, na.value
    lines = np.zeros(need_l, dtype=api.SAM_LINE_DTYPE); aux = np.zeros(need_a, dtype=np.uint8)
    for lc, ac in ((need_l - 1, need_a), (need_l, need_a - 1), (0, need_a)):
        nl.value = na.value = 0
        assert call(lines, lc, aux, ac, nl, na) == api.H2G_ERR_ARG and (nl.value, na.value) == (need_l, need_a)
        assert PU.summary(L, h) == empty
    assert call(lines, need_l, aux, need_a, nl, na) == 0 and (nl.value, na.value) == (need_l, need_a)
    once = PU.summary(L, h)
    assert once != empty
    h2 = _handle(L, g1_index)
    L.h2g_sam_set_long_edits(h2, led[0], led[1])
    rc, l2, a2, _, text, _ = PU.plan_and_text(L, h2, False, (h2,) + a)
    assert rc == 0 and PU.summary(L, h2) == once and bytes(l2.tobytes()) == lines.tobytes() and a2.tobytes() == aux.tobytes()
    # the text call's own capacity: one byte short -> the bytes needed, nothing written
    set1 = (codes, offs, None, nb, noffs)
    with pytest.raises(api.H2GError):
        api.sam_text_from_plan_host(h2.value, set1, None, np.frombuffer(rec, dtype=np.uint8)[:int(boffs[-1])], None, l2, a2, cap=len(text) - 1)
    got, offs_ = api.sam_text_from_plan_host(h2.value, set1, None, np.frombuffer(rec, dtype=np.uint8)[:int(boffs[-1])], None, l2, a2)
    assert got == text and int(offs_[-1]) == len(text)
    L.h2g_sam_close(h); L.h2g_sam_close(h2)


def test_collected_junctions_are_equal(g1_index):
    """h2g_sam_collect_novel_sites on: the planner collects the sites the formatter collects (h2g_sam_take_novel_sites, the --novel-splicesite-outfile text), also on a
    handle that has counted an earlier call"""
    L = SL.load_sam_lib()
    reads, names, res, aln, led = _unpaired_case(g1_index, 9500)
    h = vp()
    L.h2g_sam_open.argtypes = [C.c_char_p, C.POINTER(vp)]
    assert L.h2g_sam_open(g1_index.encode(), C.byref(h)) == 0
    L.h2g_sam_collect_novel_sites.argtypes = [vp, C.c_int]
    L.h2g_sam_collect_novel_sites(h, 1)
    L.h2g_sam_set_long_edits.argtypes = [vp, vp, sz]
    L.h2g_sam_set_long_edits(h, led[0], led[1])
    L.h2g_sam_set_first_read_id.argtypes = [vp, C.c_uint64]
    L.h2g_sam_set_first_read_id(h, 1000)
    codes, offs, _, nb, noffs, _, _, rec, boffs = _unpaired_args(reads, names, res, aln)
    f = L.h2g_sam_format_unpaired_compact
    f.argtypes = [vp] * 6 + [sz, vp, C.c_char_p, vp, vp, sz, C.POINTER(sz)]
    buf = C.create_string_buffer(1 << 22)
    used = sz(0)
    before = dict(PU.STATS)
    for _ in range(2):
        assert f(h, codes.ctypes.data, offs.ctypes.data, None, nb, noffs.ctypes.data, len(reads), C.addressof(res), rec, boffs.ctypes.data, buf, 1 << 22, C.byref(used)) == 0
    assert PU.STATS["calls"] - before["calls"] == 2 and PU.STATS["novel"] - before["novel"] >= 2
    L.h2g_sam_close.argtypes = [vp]
    L.h2g_sam_close(h)


def test_bad_descriptors_are_refused(g1_index):
    """what the text calls check before a byte is read through a descriptor: read, mate, alignment and extent of the record offsets, pool ranges, reference indexes"""
    L = SL.load_sam_lib()._L
    reads, names, res, aln, led = _unpaired_case(g1_index, 9400)
    h = _handle(L, g1_index)
    L.h2g_sam_set_long_edits.argtypes = [vp, vp, sz]
    L.h2g_sam_set_long_edits(h, led[0], led[1])
    a = _unpaired_args(reads, names, res, aln)
    codes, offs, _, nb, noffs, _, _, rec, boffs = a
    rc, lines, aux, _, text, _ = PU.plan_and_text(L, h, False, (h,) + a)
    assert rc == 0
    recs = np.frombuffer(rec, dtype=np.uint8)[:int(boffs[-1])]
    set1 = (codes, offs, None, nb, noffs)
    ok = lambda ls, ax=aux, rc_=recs: api.sam_text_from_plan_host(h.value, set1, None, rc_, None, ls, ax)[0]
    assert ok(lines) == text
    j = int(np.flatnonzero((lines["rec_off"] != api.SAM_NONE) & ((lines["bits"] & api.SAM_LINE_AUX_CIGAR_MDZ) != 0))[0])
    w = int(np.flatnonzero((lines["bits"] & api.SAM_LINE_WHOLE_LINE) != 0)[0])
    last = int(np.flatnonzero(lines["rec_off"] != api.SAM_NONE)[-1])

    def bad(field, value, at=j, **kw):
        ls = lines.copy()
        ls[field][at] = value
        with pytest.raises(api.H2GError):
            ok(ls, **kw)

    bad("read", len(reads))
    bad("mate", 1)
    bad("rec_off", int(lines["rec_off"][j]) + 4)
    bad("rec_off", len(recs))
    bad("rec_off", len(recs) - 8)
    bad("orec_off", 0)                                  # an unpaired run has no other mate
    bad("aux_len", len(aux) - int(lines["aux_off"][j]) + 1)
    bad("aux_off", len(aux), at=w)
    bad("cigar_len", int(lines["aux_len"][j]) + 1)
    bad("oref_tidx", 1 << 20)
    at, long_off = 0, None                              # a record beyond MAX_EDITS named by a line that would read its edits inline
    while at + 40 <= len(recs) and long_off is None:
        ne = int.from_bytes(recs[at + 24:at + 28].tobytes(), "little")
        long_off = at if ne > api.MAX_EDITS else None
        at += (40 + 12 * min(ne, 1 if ne > api.MAX_EDITS else ne) + 7) & ~7
    assert long_off is not None
    bad("rec_off", long_off)
    # the last record cut short: its edits end beyond the bytes
    ne = int.from_bytes(recs[int(lines["rec_off"][last]) + 24:int(lines["rec_off"][last]) + 28].tobytes(), "little")
    if 0 < ne <= api.MAX_EDITS:
        with pytest.raises(api.H2GError):
            ok(lines, rc_=recs[:int(lines["rec_off"][last]) + 40])
    L.h2g_sam_close(h)


def test_struct_mirror_matches_the_header(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    fields = [f for f, _ in api.SamLine._fields_]
    body = 'printf("%zu", sizeof(h2g_sam_line));' + "".join('printf(" %%zu", offsetof(h2g_sam_line, %s));' % f for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void){%sreturn 0;}\n' % (os.path.join(root, "include", "h2g.h"), body))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "sz"), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "sz")], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(api.SamLine) == 64
    assert out[1:] == [getattr(api.SamLine, f).offset for f in fields] == [api.SAM_LINE_DTYPE.fields[f][1] for f in fields]


def test_emitter_lane_by_lane_under_sanitizers(tmp_path):
    """tests/samtext/line_check.cpp drives the emitter of csrc/h2g_sam_line.h group-lane by group-lane, as the write kernel does, into exactly sized heap buffers and
    compares count and bytes with a naive string build: clean under ASan + UBSan"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "line_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", exe,
                    os.path.join(root, "tests", "samtext", "line_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout and int(r.stdout.split()[0]) > 2000, r.stdout + r.stderr


# ---- the formatter's bytes, pinned -----------------------------------------------------------------------------------------------------------
# Since the format calls write through the emitter, PlanCheckLib compares the emitter with itself.  What the formatter wrote before that change is kept as SHA-256
# digests in tests/golden/sam_text_digests.json: per case, every h2g_sam_format_* call (slot, dense and compact layouts) with a digest of everything it reads, of its
# text and of the handle's summary after it (sam_plan_util.format_inputs / PlanCheckLib._format).  Written by `PYTHONPATH=. python tests/test_sam_plan_cpu.py` at the
# commit the file names; a change that is meant to alter a line's bytes writes it again and says so.
DIGEST_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sam_text_digests.json")


def _format_unpaired_sets(base, snps, opts):
    reads, names, res, aln, led = _unpaired_case(base, 9100 + snps, snps)
    quals = np.random.default_rng(5).integers(33, 74, size=sum(len(r) for r in reads)).astype(np.uint8)
    for q in (None, quals):
        SL.format_unpaired(SL.load_sam_lib(), base, reads, names, res, aln, quals=q, options=list(opts), long_edits=led)


def _format_paired_sets(base, snps, opts):
    m1, m2, n1, n2, res, a1, a2 = _paired_case(base, 9200 + snps, snps)
    rng = np.random.default_rng(6)
    quals = [rng.integers(33, 74, size=sum(len(r) for r in m)).astype(np.uint8) for m in (m1, m2)]
    for q in (None, quals):
        SL.format_paired(SL.load_sam_lib(), base, m1, m2, n1, n2, res, a1, a2, 1 if "-k" in opts else 5, options=[o for o in opts if o not in ("-k", "1")], quals=q)


def _digest_cases():
    """id -> run(index): every parametrization of the two synthetic tests above, with and without qualities, and every record set test_long_edits_cpu formats (its
    tests themselves, whatever their skip marks say: without oracle/_ref they fail here)"""
    cases = {}
    for index, snps in (("g1_index", 0), ("g1s_index", 3)):
        for k, opts in enumerate(OPTION_SETS):
            cases["unpaired-%s-opts%d" % (index, k)] = (lambda ix, index=index, snps=snps, opts=opts: _format_unpaired_sets(ix(index), snps, opts))
        for k, opts in enumerate(OPTION_SETS + [("-k", "1")]):
            cases["paired-%s-opts%d" % (index, k)] = (lambda ix, index=index, snps=snps, opts=opts: _format_paired_sets(ix(index), snps, opts))
    beyond = _TLE.test_records_beyond_32_edits_equal_the_reference
    for mark in beyond.pytestmark:
        if mark.name == "parametrize":
            for case in mark.args[1]:
                cases["long-edits-seed%d" % case["seed"]] = (lambda ix, case=case: beyond(case))
    cases["long-edits-N-run"] = lambda ix: _TLE.test_reads_across_a_50_base_N_run_equal_the_reference()
    return cases


DIGEST_CASES = _digest_cases()


def text_digests(case, index):
    """the digests of every format call of a case; index: the name of an index fixture -> its basename"""
    PU.DIGESTS = got = []
    try:
        DIGEST_CASES[case](index)
    finally:
        PU.DIGESTS = None
    return got


@pytest.mark.parametrize("case", sorted(DIGEST_CASES))
def test_text_equals_the_recorded_digests(request, case):
    with open(DIGEST_FILE) as f:
        want = json.load(f)["cases"]
    assert sorted(want) == sorted(DIGEST_CASES), "the recorded cases are not the cases of this module"
    got = text_digests(case, request.getfixturevalue)
    assert got and [(g["call"], g["rc"], g["inputs"]) for g in got] == [(w["call"], w["rc"], w["inputs"]) for w in want[case]], "inputs changed: the case no longer formats what was recorded"
    for g, w in zip(got, want[case]):
        assert g["text"] == w["text"], "formatter regression: %s of %s writes other bytes than recorded" % (g["call"], case)
        assert g["summary"] == w["summary"], "formatter regression: the summary after %s of %s differs from the recorded one" % (g["call"], case)


if __name__ == "__main__":
    import gzip
    import subprocess
    import tempfile
    real = SL.load_sam_lib
    SL.load_sam_lib = lambda path=None: PU.PlanCheckLib(real(path))
    tmp = tempfile.mkdtemp(prefix="h2gdigest")

    def unpack(fixture):
        stem = fixture[:-len("_index")]
        for k in range(1, 9):
            with gzip.open(os.path.join(os.path.dirname(DIGEST_FILE), "%s.%d.ht2.gz" % (stem, k)), "rb") as f, open(os.path.join(tmp, "%s.%d.ht2" % (stem, k)), "wb") as o:
                o.write(f.read())
        return os.path.join(tmp, stem)

    commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=os.path.dirname(DIGEST_FILE), check=True, capture_output=True, text=True).stdout.strip()
    with open(DIGEST_FILE, "w") as f:
        json.dump({"formatter_commit": commit, "cases": {c: text_digests(c, unpack) for c in sorted(DIGEST_CASES)}}, f, indent=1)
        f.write("\n")
