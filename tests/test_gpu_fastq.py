"""GPU: FASTQ records parsed on the device (h2g_set_reads_fastq, --h2g-device-parse).  (1) set_reads_fastq + fetch_read_set equal the arrays built in Python from the
same records, byte for byte, for both mates; (2) a stream filled by it aligns exactly as the same stream filled by set_reads + set_read_names + set_mates with host-made
arrays; (3) no stale tail, two resident batches; (4) the stream's sizes; (5) records that are not plain are reported and leave the batch empty; (6) - (8) the command
line with and without --h2g-device-parse writes the same bytes, also against the reference run live and on files that make it fall back to the host parser."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import fastq_cases as F
import readsets_util as R
import sam_lines as SL
from hisat2_amd import api
from test_sam_lines import diff_lines

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "hisat2_amd", "hisat2-align-amd")
REF = os.path.join(ROOT, "oracle", "_ref", "hisat2-align-s")
needs_ref = pytest.mark.skipif(not os.path.exists(REF), reason="needs oracle/_ref")
MAX_READS, MAX_BASES = 8192, 1 << 21


@pytest.fixture(scope="module")
def genome(golden_dir):
    return R.load_genome(golden_dir)


@pytest.fixture(scope="module")
def stream(g1_index):
    ix = api.Index(g1_index)
    st = api.Stream(ix, max_reads=MAX_READS, max_bases=MAX_BASES)
    yield st
    st.close()
    ix.close()


@pytest.fixture(scope="module")
def sets():
    """the record sets, made once: mate 1 and mate 2 of the ragged set (5 000 records) and of the common case (300 records of 100 bases)"""
    return {"ragged": (F.ragged_records(11, 5000), F.ragged_records(12, 5000)), "hundred": (F.fixed_records(13, 300), F.fixed_records(14, 300)),
            "ragged64": (F.ragged_records(15, 700, phred64=True), F.ragged_records(16, 700, phred64=True))}


def check_mate(st, mate, want, what):
    got = st.fetch_read_set(mate)
    assert np.array_equal(got["offs"], want["offs"]), what
    assert np.array_equal(got["codes"], want["codes"]), what
    assert np.array_equal(got["quals"], want["quals"]), what
    assert np.array_equal(got["name_offs"], want["name_offs"]), what
    assert got["names"] == want["names"], what


def fill_and_check(st, recs1, recs2, what, n=None, crlf=False, last_newline=True, final=True, max_records=0, **opts):
    """n: the records the call is to parse (default: all)"""
    n = len(recs1) if n is None else n
    t1 = F.text_of(recs1, crlf, last_newline)
    t2 = None if recs2 is None else F.text_of(recs2, crlf, last_newline)
    res = st.set_reads_fastq(t1, t2, final=final, max_records=max_records, **opts)
    assert (res.n_records, res.n_not_plain, res.first_not_plain) == (n, 0, n), what
    assert st.n_reads == n
    # the bytes those records occupy: the text of the first n, less the line end a text without a last newline lacks
    whole = n == len(recs1) and not last_newline
    assert res.consumed1 == len(F.text_of(recs1[:n], crlf, not whole)), what
    assert res.consumed2 == (0 if recs2 is None else len(F.text_of(recs2[:n], crlf, not whole))), what
    w1 = F.expected(recs1[:n], **opts)
    w2 = None if recs2 is None else F.expected(recs2[:n], **opts)
    assert (res.n_bases1, res.n_name_bytes1) == (len(w1["codes"]), len(w1["names"])), what
    assert res.max_read_len == max(w1["max_len"], w2["max_len"] if w2 else 0), what
    if n == 0:
        return
    check_mate(st, 0, w1, what + " (mate 1)")
    if w2:
        assert (res.n_bases2, res.n_name_bytes2) == (len(w2["codes"]), len(w2["names"])), what
        check_mate(st, 1, w2, what + " (mate 2)")


@pytest.mark.parametrize("which", ["ragged", "hundred"])
@pytest.mark.parametrize("crlf", [False, True])
def test_parse_is_exact(stream, sets, which, crlf):
    a, b = sets[which]
    fill_and_check(stream, a, b, f"{which}, pairs", crlf=crlf)
    fill_and_check(stream, a, None, f"{which}, unpaired", crlf=crlf)
    # a last line without '\n': complete when the text ends the input, else its record stays unconsumed
    fill_and_check(stream, a, b, f"{which}, no last newline", crlf=crlf, last_newline=False)
    fill_and_check(stream, a, b, f"{which}, no last newline, not final", n=len(a) - 1, crlf=crlf, last_newline=False, final=False)


@pytest.mark.parametrize("trim5", [0, 3, 200])
@pytest.mark.parametrize("trim3", [0, 3, 200])
def test_trimmed(stream, sets, trim5, trim3):
    for which in ("ragged", "hundred"):
        a, b = sets[which]
        fill_and_check(stream, a, b, f"{which} -5 {trim5} -3 {trim3}", trim5=trim5, trim3=trim3)


def test_phred64(stream, sets):
    a, b = sets["ragged64"]
    fill_and_check(stream, a, b, "phred64", phred64=True)
    fill_and_check(stream, a, b, "phred64, trimmed, CRLF", crlf=True, phred64=True, trim5=3, trim3=3)


@pytest.mark.parametrize("which", ["ragged", "hundred"])
def test_max_records(stream, sets, which):
    a, b = sets[which]
    n = len(a)
    for mr in (1, 7, n, n + 5):
        fill_and_check(stream, a, b, f"{which}, max_records {mr}", n=min(mr, n), max_records=mr)
    fill_and_check(stream, a, b[:n - 9], f"{which}, a shorter mate 2 text", n=n - 9)


def test_text_beyond_one_scan_tile_of_workgroups(g1_index):
    """90 000 records of 100 bases are 21 MB of text: more than the 2 048 workgroups (4 KB of text each) one tile of the newline-count scan holds"""
    recs = F.fixed_records(17, 90000)
    assert len(F.text_of(recs)) > 2048 * 4096 * 2
    ix = api.Index(g1_index)
    st = api.Stream(ix, max_reads=90000, max_bases=9000000)
    try:
        fill_and_check(st, recs, None, "90 000 records")
        fill_and_check(st, recs, None, "90 000 records, no last newline, trimmed", last_newline=False, trim5=1, trim3=2)
    finally:
        st.close()
        ix.close()


def test_one_record_and_empty_text(stream, sets):
    a, b = sets["ragged"]
    fill_and_check(stream, a[:1], b[:1], "one record")
    fill_and_check(stream, a[1:2], None, "one record, no last newline", last_newline=False)
    fill_and_check(stream, [], [], "empty texts")
    assert stream.fetch_read_set(0)["offs"].tolist() == [0]
    fill_and_check(stream, [], None, "empty text")
    fill_and_check(stream, a[:40], [], "an empty mate 2 text", n=0)


# ---- (2) the same batch as the three calls
def _three_calls(st, w1, w2):
    st.set_reads(w1["codes"], w1["offs"], w1["quals"])
    st.set_read_names((w1["names"], w1["name_offs"]))
    if w2:
        st.set_mates(w2["codes"], w2["offs"], (w2["names"], w2["name_offs"]), w2["quals"])


def test_aligns_as_after_the_three_upload_calls(stream, genome):
    """2 000 pairs with unequal mates (mate 2 loses 0 .. 30 bases), then the same reads unpaired, fast pass on: the compact fetch of the run is the same bytes"""
    rng = np.random.default_rng(5)
    recs = R.make_records(genome, 501, 2000, pair_frac=1.0)
    a = [(r[0].encode() + b"/1", r[1].encode(), r[2].encode()) for r in recs]
    b = []
    for r in recs:
        cut = len(r[3]) - int(rng.integers(0, 31))
        b.append((r[0].encode() + b"/2", r[3][:cut].encode(), r[4][:cut].encode()))
    w1, w2 = F.expected(a), F.expected(b)
    outs = []
    for device in (False, True):
        if device:
            res = stream.set_reads_fastq(F.text_of(a), F.text_of(b))
            assert res.n_not_plain == 0 and res.n_records == len(a)
        else:
            _three_calls(stream, w1, w2)
            stream.n_reads = len(a)
        stream.align_pairs_run()
        res, r1, o1, r2, o2 = stream.align_pairs_fetch_compact()
        outs.append((bytes(res), r1[:int(o1[-1])].tobytes(), o1.tobytes(), r2[:int(o2[-1])].tobytes(), o2.tobytes()))
    assert outs[0] == outs[1]
    assert stream.counters().n_fast > len(a) // 2                  # the fast pass took them
    outs = []
    for device in (False, True):
        if device:
            stream.set_reads_fastq(F.text_of(a))
        else:
            _three_calls(stream, w1, None)
            stream.n_reads = len(a)
        stream.align_run()
        res, rec, boffs = stream.align_fetch_compact()
        outs.append((res.tobytes(), rec[:int(boffs[-1])].tobytes(), boffs.tobytes()))
    assert outs[0] == outs[1]
    assert (np.frombuffer(outs[0][0], dtype=api.READ_RESULT_DTYPE)["nselect"] > 0).sum() > len(a) // 2


# ---- (3)
def test_a_smaller_set_leaves_no_stale_tail(stream, sets):
    a, b = sets["ragged"]
    fill_and_check(stream, a, b, "large set")
    fill_and_check(stream, a[100:111], b[200:211], "small set after a large one")
    assert stream.n_reads == 11


def test_two_resident_batches_back_to_back(stream, sets):
    a, b = sets["ragged"]
    h1, h2 = sets["hundred"]
    stream.select_batch(0)
    fill_and_check(stream, a[:900], b[:900], "batch 0")
    stream.select_batch(1)
    fill_and_check(stream, h1, h2, "batch 1")
    stream.select_batch(0)
    check_mate(stream, 0, F.expected(a[:900]), "batch 0 after batch 1 was filled")
    check_mate(stream, 1, F.expected(b[:900]), "batch 0 after batch 1 was filled (mate 2)")
    stream.select_batch(1)
    check_mate(stream, 0, F.expected(h1), "batch 1 again")
    check_mate(stream, 1, F.expected(h2), "batch 1 again (mate 2)")
    stream.select_batch(0)


# ---- (4)
def test_the_streams_sizes_are_respected(stream, sets):
    many = [(b"x", b"A", b"I")] * (MAX_READS + 1)
    with pytest.raises(api.H2GError) as e:
        stream.set_reads_fastq(F.text_of(many))
    assert e.value.result.n_records == MAX_READS + 1 and e.value.result.n_bases1 == MAX_READS + 1 and e.value.result.n_name_bytes1 == MAX_READS + 1
    assert stream.fetch_read_set(0)["offs"].tolist() == [0] and stream.n_reads == 0
    long = F.fixed_records(3, MAX_BASES // 8000 + 1, length=8000)
    with pytest.raises(api.H2GError) as e:
        stream.set_reads_fastq(F.text_of(sets["hundred"][0][:len(long)]), F.text_of(long))
    assert e.value.result.n_bases2 == 8000 * len(long) > MAX_BASES and e.value.result.n_records == len(long)
    assert stream.fetch_read_set(0)["offs"].tolist() == [0]
    # a text of 2^32 bytes: refused by its length, before a byte of it is looked at
    buf = np.zeros(64, np.uint8)
    opts, res = api.FastqOpts(0, 0, 0, 1, 1, 0, 0), api.FastqResult()
    assert api.lib().h2g_set_reads_fastq(stream.h, buf.ctypes.data, 1 << 32, None, 0, C.byref(opts), C.byref(res)) == -4
    assert b"4 GB" in api.lib().h2g_last_error()
    fill_and_check(stream, *sets["hundred"], "a set that fits, afterwards")


# ---- (5)
@pytest.mark.parametrize("kind", range(len(F.NOT_PLAIN_KINDS)), ids=[k.replace(" ", "_") for k in F.NOT_PLAIN_KINDS])
def test_not_plain_records_are_reported(stream, sets, kind):
    p64 = kind == 6
    a, b = (F.fixed_records(21, 300, phred64=p64), F.fixed_records(22, 300, phred64=p64))
    bad = 217
    for t1, t2 in ((F.text_with_bad_record(a, bad, kind), None), (F.text_of(a), F.text_with_bad_record(b, bad, kind)), (F.text_with_bad_record(a, bad, kind), F.text_with_bad_record(b, bad, kind))):
        fill_and_check(stream, *sets["hundred"], "a full batch first")
        res = stream.set_reads_fastq(t1, t2, phred64=p64)
        assert (res.n_records, res.n_not_plain, res.first_not_plain) == (300, 1, bad), F.NOT_PLAIN_KINDS[kind]
        assert stream.n_reads == 0 and stream.fetch_read_set(0)["offs"].tolist() == [0]
        # the record lies beyond max_records: the call succeeds
        res = stream.set_reads_fastq(t1, t2, phred64=p64, max_records=bad)
        assert (res.n_records, res.n_not_plain, res.first_not_plain) == (bad, 0, bad)
        check_mate(stream, 0, F.expected(a[:bad], phred64=p64), "up to the record that is not plain")
    # two records that are not plain, one in each mate: counted once each, the first one named
    res = stream.set_reads_fastq(F.text_with_bad_record(a, 250, kind), F.text_with_bad_record(b, 31, kind), phred64=p64)
    assert (res.n_not_plain, res.first_not_plain) == (2, 31)


# ---- (6) - (8) the command line
@pytest.fixture(scope="module")
def files(genome, tmp_path_factory):
    return F.cli_fixtures(genome, tmp_path_factory.mktemp("fqcli"))


def run_cli(args, sam, err, p=3, **kw):
    return subprocess.run([CLI, "-p", str(p)] + [str(a) for a in args] + ["-S", str(sam)], stderr=open(err, "w"), **kw)


def both_ways(tmp, tag, args, p=3, want_reads=None):
    """the run without and with --h2g-device-parse: the SAM body and stderr are the same bytes -> the stats of the run with the flag"""
    outs = {}
    for flag in (False, True):
        sam, err, stats = (tmp / f"{tag}.{int(flag)}.{x}" for x in ("sam", "err", "json"))
        run_cli(list(args) + ["--batch", "1000", "--h2g-stats", stats] + (["--h2g-device-parse"] if flag else []), sam, err, p=p, check=True)
        outs[flag] = (SL.body_lines(str(sam)), open(err).read(), json.load(open(stats)))
    assert len(outs[False][0]) > 0
    assert diff_lines(outs[True][0], outs[False][0]) == 0, tag
    assert outs[True][1] == outs[False][1], tag
    st = outs[True][2]
    assert st["reads"] == outs[False][2]["reads"] and st["device_parsed"] + st["host_parsed"] == st["reads"], st
    assert outs[False][2]["device_parsed"] == 0 and outs[False][2]["host_parsed"] == 0
    if want_reads is not None:
        assert st["reads"] == want_reads
    return st, outs[True][0]


CLI_CASES = {
    "U": (lambda f: ["-U", f["u"], "--no-temp-splicesite"], 3, 2000),
    "pairs": (lambda f: ["-1", f["m1"], "-2", f["m2"], "--no-temp-splicesite"], 3, 2000),
    "pairs_and_U": (lambda f: ["-1", f["m1"], "-2", f["m2"], "-U", f["u"], "--no-temp-splicesite"], 3, 4000),
    "gz": (lambda f: ["-1", f["m1_gz"], "-2", f["m2_gz"], "-U", f["u_gz"], "--no-spliced-alignment"], 3, 4000),
    "two_files": (lambda f: ["-1", f["m1_a"] + "," + f["m1_b"], "-2", f["m2_a"] + "," + f["m2_b"], "-U", f["u_a"] + "," + f["u_b"], "--no-temp-splicesite"], 3, 4000),
    "trimmed": (lambda f: ["-1", f["m1"], "-2", f["m2"], "-5", "4", "-3", "7", "--no-temp-splicesite"], 3, 2000),
    "phred64": (lambda f: ["-1", f["m1_64"], "-2", f["m2_64"], "--phred64", "--no-temp-splicesite"], 3, 2000),
    "skip_upto": (lambda f: ["-U", f["u"], "-s", "150", "-u", "900", "--no-temp-splicesite"], 3, 900),
    "temp_splicesites": (lambda f: ["-U", f["u"]], 2, 2000),
    "temp_splicesites_pairs": (lambda f: ["-1", f["m1"], "-2", f["m2"]], 2, 2000),
    "device_plan": (lambda f: ["-1", f["m1"], "-2", f["m2"], "--no-temp-splicesite", "--h2g-device-plan"], 3, 2000),
    "gpus_1": (lambda f: ["-U", f["u"], "--gpus", "1", "--no-temp-splicesite"], 3, 2000),
}


@pytest.mark.parametrize("case", sorted(CLI_CASES))
def test_command_line_writes_the_same_bytes(tmp_path, files, g1_index, case):
    args, p, nreads = CLI_CASES[case]
    st, _ = both_ways(tmp_path, case, ["-x", g1_index] + args(files), p=p, want_reads=nreads)
    # (tests/test_fastq_cpu.py has shown on the CPU that every record of these files is plain)
    assert st["device_parsed"] == st["reads"] and st["host_parsed"] == 0, st


@needs_ref
@pytest.mark.parametrize("case", ["pairs", "U"])
def test_command_line_against_the_reference(tmp_path, files, g1_index, case):
    args = ["-x", g1_index] + CLI_CASES[case][0](files)
    ref_sam, ref_err, sam, err = (tmp_path / x for x in ("ref.sam", "ref.err", "amd.sam", "amd.err"))
    subprocess.run([REF, "-p", "3", "--reorder"] + [str(a) for a in args] + ["-S", str(ref_sam)], check=True, stderr=open(ref_err, "w"))
    run_cli(args + ["--h2g-device-parse", "--batch", "1000"], sam, err, check=True)
    want = SL.body_lines(str(ref_sam))
    assert len(want) >= 2000
    assert diff_lines(SL.body_lines(str(sam)), want) == 0
    assert open(err).read() == open(ref_err).read()


def test_command_line_falls_back_to_the_host_parser(tmp_path, files, g1_index):
    """a record with an empty name (the host names it by its running number): the item that holds it is parsed by the host, the others by the device"""
    lines = open(files["u"]).read().split("\n")
    lines[4 * 1499] = "@"
    path = tmp_path / "noname.fq"
    path.write_text("\n".join(lines))
    st, body = both_ways(tmp_path, "noname", ["-x", g1_index, "-U", path, "--no-temp-splicesite"], want_reads=2000)
    assert (st["device_parsed"], st["host_parsed"]) == (1000, 1000), st
    assert any(l.split("\t")[0] == "1499" for l in body)


def test_command_line_files_that_end_in_blank_lines(tmp_path, files, g1_index):
    """several files per option, every one but the last ending in blank lines (LF, CRLF, a lone blank): the records behind them are parsed as before, all on the device"""
    parts = {}
    for key in ("m1", "m2", "u"):
        lines = open(files[key]).read().split("\n")[:-1]
        cuts = [(0, 300, "\n\n"), (300, 777, "\r\n\r\n"), (777, 1500, "\n \n\n"), (1500, 2000, "")]
        parts[key] = []
        for k, (lo, hi, tail) in enumerate(cuts):
            path = tmp_path / f"{key}_{k}.fq"
            path.write_text("\n".join(lines[4 * lo:4 * hi]) + "\n" + tail)
            parts[key].append(str(path))
    args = ["-x", g1_index, "-1", ",".join(parts["m1"]), "-2", ",".join(parts["m2"]), "-U", ",".join(parts["u"]), "--no-temp-splicesite"]
    st, _ = both_ways(tmp_path, "blank_tails", args, want_reads=4000)
    assert (st["device_parsed"], st["host_parsed"]) == (4000, 0), st


def test_command_line_longer_second_mate_file_and_fallback(tmp_path, files, g1_index):
    """-2 holds more records than -1 (the surplus is never looked at) and the last item falls back to the host parser (an empty name in it)"""
    lines = open(files["m1"]).read().split("\n")[:4 * 1500]
    lines[4 * 1200] = "@"
    path = tmp_path / "m1_short.fq"
    path.write_text("\n".join(lines) + "\n")
    st, _ = both_ways(tmp_path, "surplus", ["-x", g1_index, "-1", path, "-2", files["m2"], "--no-temp-splicesite"], want_reads=1500)
    assert (st["device_parsed"], st["host_parsed"]) == (1000, 500), st


def test_command_line_malformed_record_among_the_skipped(tmp_path, files, g1_index):
    """-s: the skipped records are parsed by the host with and without the flag, so a malformed one among them ends the run with the same message"""
    lines = open(files["u"]).read().split("\n")
    lines[4 * 50 + 3] = lines[4 * 50 + 3][:-5]
    path = tmp_path / "short_skipped.fq"
    path.write_text("\n".join(lines))
    outs = []
    for flag in (False, True):
        err = tmp_path / f"skipped.{int(flag)}.err"
        p = run_cli(["-x", g1_index, "-U", path, "-s", "100", "--no-temp-splicesite", "--batch", "1000"] + (["--h2g-device-parse"] if flag else []), tmp_path / f"skipped.{int(flag)}.sam", err)
        outs.append((p.returncode, open(err).read()))
    assert outs[0] == outs[1] and outs[0][0] == 1 and "has more read characters than quality values" in outs[0][1], outs


def test_command_line_reports_a_malformed_file_as_before(tmp_path, files, g1_index):
    """a truncated quality line: the host parser's message and exit status, with and without the flag"""
    lines = open(files["u"]).read().split("\n")
    lines[4 * 700 + 3] = lines[4 * 700 + 3][:-5]
    path = tmp_path / "short.fq"
    path.write_text("\n".join(lines))
    outs = []
    for flag in (False, True):
        err = tmp_path / f"short.{int(flag)}.err"
        p = run_cli(["-x", g1_index, "-U", path, "--no-temp-splicesite", "--batch", "1000"] + (["--h2g-device-parse"] if flag else []), tmp_path / f"short.{int(flag)}.sam", err)
        outs.append((p.returncode, open(err).read()))
    assert outs[0] == outs[1] and outs[0][0] == 1 and "has more read characters than quality values" in outs[0][1], outs
