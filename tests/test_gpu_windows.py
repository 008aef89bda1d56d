"""GPU: -F <len>,<step>, the read set expanded on the device.  (1) h2g_set_reads_windows + h2g_fetch_reads equal the numpy expansion on all five arrays, byte for
byte; (2) a stream filled by it aligns exactly as the same stream filled by h2g_set_reads + h2g_set_read_names + h2g_set_read_ids, on a linear and on an SNP-graph
index; (3) the command line equals `hisat2-align-s -p 1` (`-p 2 --reorder` for a step of 1 with temporary splice sites): SAM body and summary."""
import os
import subprocess

import numpy as np
import pytest

import sam_lines as SL
import windows_util as W
from hisat2_amd import api, synth
from test_sam_lines import diff_lines

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not os.path.exists(os.path.join(W.REF, "hisat2-align-s")), reason="needs oracle/_ref")

LENS = (1, 3, 30, 33, 128, 129, 512)
MAX_READS, MAX_BASES = 4096, 1 << 21


@pytest.fixture(scope="module")
def stream(g1_index):
    ix = api.Index(g1_index)
    st = api.Stream(ix, max_reads=MAX_READS, max_bases=MAX_BASES)
    yield st
    st.close()
    ix.close()


def seg(text_start, name_off0, rdid0, n, pstart, plen):
    return (text_start, name_off0, rdid0, n, pstart, plen, 0)


def shapes(length, step, rng):
    """the segment tables of one (len, step): (what, segs, prefixes)"""
    out = [("single window", [seg(0, 0, 0, 1, 0, 2)], b"r_")]
    for nw in (63, 64, 65):
        out.append((f"{nw} windows", [seg(2, 5, 1000, nw, 0, 5)], b"chr1_"))
    v, pre, t, rid = [], b"", 0, 17                            # 300 segments of 1-3 windows
    for k in range(300):
        nw = int(rng.integers(1, 4))
        p = b"ctg%d_" % k
        v.append(seg(t, 0, rid, nw, len(pre), len(p)))
        pre += p
        t += (nw - 1) * step + length + int(rng.integers(0, 4))
        rid += (nw - 1) * step + 1
    out.append(("300 segments", v, pre))
    v, t = [], 3                                               # printed offsets that straddle a decimal width (and ids that pass 2^32); an empty and a 200-byte prefix
    pre = b"x_" + b"p" * 199 + b"_"
    for e in (9, 99, 999999, 4294967290):
        off0 = max(0, e - 3 * max(step, 1))
        ps, pl = (0, 0) if e == 99 else (2, 200) if e == 999999 else (0, 2)
        v.append(seg(t, off0, off0 + 12345, 9, ps, pl))
        t += 8 * step + length
    out.append(("width edges", v, pre))
    return out


def fill_and_check(st, length, step, segs, pre, rng, what):
    segs = np.array(segs, dtype=api.WINDOW_SEG_DTYPE)
    n_text = int((segs["text_start"] + (segs["n_windows"] - 1).astype(np.uint64) * np.uint64(step)).max()) + length
    text = rng.integers(0, 5, size=n_text, dtype=np.uint8)     # (code 4 included)
    st.set_reads_windows(text, segs, length, step, pre)
    want = api.expand_windows(text, segs, length, step, pre)
    check(st, want, what)
    return want


def check(st, want, what):
    got = st.fetch_reads()
    codes, offs, names, noffs, ids = want
    assert np.array_equal(got["offs"], offs), what
    assert np.array_equal(got["codes"], codes), what
    assert np.array_equal(got["name_offs"], noffs), what
    assert got["names"] == names, what
    assert np.array_equal(got["ids"], ids), what


@pytest.mark.parametrize("length", LENS)
def test_expansion_is_exact(stream, length):
    rng = np.random.default_rng(900 + length)
    for step in (0, 1, 7, length, length + 5):
        for what, segs, pre in shapes(length, step, rng):
            fill_and_check(stream, length, step, segs, pre, rng, f"len {length} step {step}: {what}")


def test_a_smaller_set_leaves_no_stale_tail(stream):
    rng = np.random.default_rng(77)
    fill_and_check(stream, 129, 7, [seg(0, 0, 0, 900, 0, 4)], b"big_", rng, "large set")
    fill_and_check(stream, 30, 1, [seg(5, 95, 3, 11, 0, 2)], b"s_", rng, "small set after a large one")
    assert stream.n_reads == 11


def test_two_resident_batches_back_to_back(stream):
    rng = np.random.default_rng(78)
    stream.select_batch(0)
    a = fill_and_check(stream, 33, 5, [seg(0, 0, 0, 65, 0, 2), seg(400, 0, 400, 3, 2, 3)], b"a_bb_", rng, "batch 0")
    stream.select_batch(1)
    b = fill_and_check(stream, 128, 1, [seg(1, 7, 9, 200, 0, 0)], b"", rng, "batch 1")
    stream.select_batch(0)
    check(stream, a, "batch 0 after batch 1 was filled")
    stream.select_batch(1)
    check(stream, b, "batch 1 again")
    stream.select_batch(0)


def test_the_streams_sizes_are_respected(stream):
    text = np.zeros(MAX_BASES + 4096, dtype=np.uint8)
    with pytest.raises(api.H2GError):
        stream.set_reads_windows(text, np.array([seg(0, 0, 0, MAX_READS + 1, 0, 0)], dtype=api.WINDOW_SEG_DTYPE), 1, 1)
    with pytest.raises(api.H2GError):
        stream.set_reads_windows(text, np.array([seg(0, 0, 0, MAX_BASES // 512 + 1, 0, 0)], dtype=api.WINDOW_SEG_DTYPE), 512, 1)
    with pytest.raises(api.H2GError):                              # a segment that names text it was not given
        stream.set_reads_windows(text[:100], np.array([seg(0, 0, 0, 72, 0, 0)], dtype=api.WINDOW_SEG_DTYPE), 30, 1)


# ---- a 100 kb genome with planted repeats (tie-breaks depend on the name-seeded PRNG), introns for a spliced transcript; the queries
def _world(tmp):
    rng = np.random.default_rng(4242)
    g = synth.make_genome([100000], 4242, repeats=30, repeat_len=400)[0].copy()
    g[g > 3] = 0
    exons, pos = [], 60000                                     # canonical introns GT .. AG between the exons of one transcript
    while pos < 75000:
        e = int(rng.integers(150, 400))
        i = int(rng.integers(100, 1200))
        exons.append((pos, pos + e))
        g[pos + e:pos + e + 2] = [2, 3]
        g[pos + e + i - 2:pos + e + i] = [0, 2]
        pos += e + i
    fa = os.path.join(tmp, "g.fa")
    synth.write_fasta(fa, [g])
    snps = synth.make_snps([g], 4247, every=200)
    synth.write_snps(os.path.join(tmp, "g.snp"), snps)
    lin, gra = os.path.join(tmp, "lin"), os.path.join(tmp, "gra")
    subprocess.run([os.path.join(W.REF, "hisat2-build-s"), "-q", fa, lin], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    subprocess.run([os.path.join(W.REF, "hisat2-build-s"), "-q", "--snp", os.path.join(tmp, "g.snp"), fa, gra], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    q = g[30000:50000].copy()                                  # a mutated copy of 20 kb, with an N run
    m = rng.random(len(q)) < 0.01
    q[m] = (q[m] + rng.integers(1, 4, size=int(m.sum()))) % 4
    q[7000:7040] = 4
    tr = np.concatenate([g[a:b] for a, b in exons])            # the spliced transcript
    alpha = np.frombuffer(b"ACGTN", dtype=np.uint8)
    qfa, tfa = os.path.join(tmp, "query.fa"), os.path.join(tmp, "transcript.fa")
    for path, name, s in ((qfa, "contig7 mutated copy", q), (tfa, "tx1", tr)):
        txt = alpha[s].tobytes().decode()
        with open(path, "w") as f:
            f.write(">%s\n" % name + "\n".join(txt[k:k + 70] for k in range(0, len(txt), 70)) + "\n")
    return {"lin": lin, "gra": gra, "query": qfa, "transcript": tfa}


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return _world(str(tmp_path_factory.mktemp("winworld")))


@needs_ref
@pytest.mark.parametrize("kind", ("lin", "gra"))
def test_alignment_equals_the_three_upload_calls(world, kind):
    plan = api.WindowPlan(50, 7)
    for fn in (world["query"], world["transcript"]):
        plan.add_file(open(fn, "rb").read())
    text, pre, segs = plan.text(), plan.prefixes(), plan.segments()
    codes, offs, names, noffs, ids = api.expand_windows(text, segs, 50, 7, pre)
    n = plan.n_reads
    assert n > 3000
    ix = api.Index(world[kind])
    st = api.Stream(ix, max_reads=n, max_bases=n * 50)
    p = st.align_params()
    outs = []
    for way in ("windows", "three calls"):
        if way == "windows":
            st.set_reads_windows(text, segs, 50, 7, pre)
        else:
            st.set_reads(codes, offs)
            st.set_read_names((names, noffs))
            st.set_read_ids(ids)
        st.align_run(p)
        res, rec, boffs = st.align_fetch_compact()
        outs.append((res.tobytes(), rec[:int(boffs[n])].tobytes(), boffs.tobytes()))
    assert outs[0][2] == outs[1][2] and outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1]
    res = np.frombuffer(outs[0][0], dtype=api.READ_RESULT_DTYPE)
    assert (res["nselect"] > 0).sum() > n // 2 and (res["nselect"] > 1).sum() > 0      # repeats: reads with several placements
    st.close()
    ix.close()
    plan.close()


def _cli_equals_reference(tmp, base, files, f_arg, ref_opts, amd_opts):
    ref_sam, amd_sam = os.path.join(tmp, "ref.sam"), os.path.join(tmp, "amd.sam")
    common = ["-x", base, "-F", f_arg, "-U", ",".join(files)]
    subprocess.run([os.path.join(W.REF, "hisat2-align-s"), "-S", ref_sam] + common + ref_opts, check=True, stdout=subprocess.DEVNULL, stderr=open(os.path.join(tmp, "ref.err"), "w"))
    subprocess.run([W.CLI, "-S", amd_sam] + common + amd_opts, check=True, stderr=open(os.path.join(tmp, "amd.err"), "w"))
    want = SL.body_lines(ref_sam)
    assert len(want) > 0 and diff_lines(SL.body_lines(amd_sam), want) == 0
    assert open(os.path.join(tmp, "amd.err")).read() == open(os.path.join(tmp, "ref.err")).read()
    return want


CLI_CASES = (
    # (index, -F, the reference's options, this program's options); the two default-mode cases read the transcript first, so that their windows are spliced
    ("lin", "50,7", ["-p", "1", "--no-spliced-alignment"], ["-p", "4", "--batch", "700", "--no-spliced-alignment"]),
    ("lin", "100,1", ["-p", "1", "--no-temp-splicesite"], ["-p", "4", "--no-temp-splicesite"]),
    ("lin", "30,10", ["-p", "1", "-u", "3000"], ["-p", "1", "-u", "3000", "tx-first"]),                  # the default mode at -p 1: 300 windows
    ("lin", "40,1", ["-p", "2", "--reorder", "-u", "6000"], ["-p", "2", "-u", "6000", "tx-first"]),        # the default mode, a step of 1 at -p 2
    ("lin", "50,7", ["-p", "1", "--no-temp-splicesite", "-s", "19000", "-u", "2500"], ["-p", "3", "--no-temp-splicesite", "-s", "19000", "-u", "2500", "--batch", "100"]),
    ("gra", "50,7", ["-p", "1", "--no-temp-splicesite"], ["-p", "4", "--no-temp-splicesite", "--batch", "700"]),
)


@needs_ref
@pytest.mark.parametrize("kind,f_arg,ref_opts,amd_opts", CLI_CASES)
def test_command_line_equals_the_reference(world, tmp_path, kind, f_arg, ref_opts, amd_opts):
    files = [world["query"], world["transcript"]]
    if amd_opts[-1] == "tx-first":
        files, amd_opts = files[::-1], amd_opts[:-1]
    want = _cli_equals_reference(str(tmp_path), world[kind], files, f_arg, ref_opts, amd_opts)
    if "--no-spliced-alignment" not in ref_opts and "-s" not in ref_opts:
        assert sum(1 for l in want if "N" in l.split("\t")[5]) > 5
