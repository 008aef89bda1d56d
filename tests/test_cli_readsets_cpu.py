"""The record stream of hisat2-align-amd, host side (no GPU, no index: `--parse-only` prints records, bases, a checksum over every window of <--batch>
records, and the numbers of pairs and of unpaired reads): --tab5 / --tab6 / --12 / --qseq, -1/-2 together with -U, --solexa-quals / --int-quals, the
reference's quality-count errors, records of 0 and 1 bases with the length-filter warnings they bring (which `--parse-only` writes to stderr as a run does), and the
file names of --un-conc and its kin (which `--parse-only` prints, one line per option)."""
import gzip
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "hisat2_amd", "hisat2-align-amd")
FRONT = os.path.join(ROOT, "hisat2_amd", "hisat2-amd")          # the front end: the read-file options (--un, --al-conc ...) are its own, as in the reference
pytestmark = pytest.mark.skipif(not os.path.exists(CLI), reason="hisat2-align-amd not built (python __graft_entry__.py)")

CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
COMBOS = ((1, 1 << 20), (4, 1 << 20), (7, 700), (3, 1))


def fnv(h, data):
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def codes_of(seq):
    """asc2dna: A C G T N, every other letter reads as A; characters that are not letters are not bases"""
    return bytes(CODE.get(c.upper(), 0) for c in seq if c.isalpha())


def expected(records, batch, windows=None):
    """records: (name1, seq1, qual1, None) for an unpaired read, (name1, seq1, qual1, (name2, seq2, qual2)) for a pair, as they come out of the parser
    (trimmed, default names set).  windows: lists of record indices when the windows are not simply consecutive slices of `batch`."""
    h, bases, npairs = 1469598103934665603, 0, 0
    if windows is None:
        windows = [range(b0, min(len(records), b0 + batch)) for b0 in range(0, len(records), batch)]
    for w in windows:
        recs = [records[i] for i in w]
        a = [(r[0], codes_of(r[1]), r[2]) for r in recs]
        b = [(r[3][0], codes_of(r[3][1]), r[3][2]) for r in recs if r[3] is not None]
        for side in (a, b):
            if not side:
                continue
            h = fnv(h, b"".join(c for _, c, _ in side))
            h = fnv(h, "".join(nm for nm, _, _ in side).encode())
            h = fnv(h, "".join(q for _, _, q in side).encode())
            h = fnv(h, b"".join(np.uint32(len(c)).tobytes() + np.uint32(len(nm.encode())).tobytes() for nm, c, _ in side))
            bases += sum(len(c) for _, c, _ in side)
        npairs += len(b)
    return len(records), bases, h, npairs, len(records) - npairs


def run(args, **kw):
    out = subprocess.run([CLI, "--parse-only", "-x", "unused"] + [str(a) for a in args], check=True, capture_output=True, text=True, **kw).stdout
    t = out.split("\n")[0].split()
    return int(t[0]), int(t[1]), int(t[2], 16), int(t[3]), int(t[4])


def gz(path):
    with open(path, "rb") as fi, gzip.open(str(path) + ".gz", "wb") as fo:
        shutil.copyfileobj(fi, fo)
    return str(path) + ".gz"


def rand_seq(rng, alphabet="ACGTNacgtRY"):
    return "".join(rng.choice(list(alphabet), size=int(rng.integers(30, 160))))


def rand_qual(rng, n):
    return "".join(chr(int(q)) for q in rng.integers(35, 74, size=n))


def trimmed(seq, qual, t5, t3):
    s = seq[min(t5, len(seq)):]
    q = qual[min(t5, len(qual)):]
    k = min(t3, len(s))
    return (s[:len(s) - k], q[:len(q) - k])


def write_formats(tmp_path, names, seqs, quals, eol="\n", tag=""):
    """the same unpaired reads as FASTQ, tab5, tab6 and (names shaped m_r_l_t_x_y_i/m only) QSEQ; in the QSEQ file an N is written as '.'"""
    files = {}
    with open(tmp_path / f"u{tag}.fq", "w", newline="") as f:
        for nm, s, q in zip(names, seqs, quals):
            f.write(f"@{nm}\n{s}\n+\n{q}\n")
    files["fastq"] = tmp_path / f"u{tag}.fq"
    for fmt in ("tab5", "tab6"):
        with open(tmp_path / f"u{tag}.{fmt}", "w", newline="") as f:
            f.write(eol)                                            # leading blank lines are skipped
            for nm, s, q in zip(names, seqs, quals):
                f.write(f"{nm}\t{s}\t{q}{eol}")
        files[fmt] = tmp_path / f"u{tag}.{fmt}"
    if all(nm.count("_") == 6 and nm.count("/") == 1 for nm in names):
        with open(tmp_path / f"u{tag}_qseq.txt", "w", newline="") as f:
            for i, (nm, s, q) in enumerate(zip(names, seqs, quals)):
                head, mate = nm.split("/")
                f.write("\t".join(head.split("_") + [mate, s.replace("N", ".").replace("n", "."), q, "01"[i % 7 != 0]]) + eol)
        files["qseq"] = tmp_path / f"u{tag}_qseq.txt"
    return files


FLAG = {"fastq": ["-q", "-U"], "tab5": ["--tab5"], "tab6": ["--tab6"], "qseq": ["--qseq", "-U"]}


def test_every_format_parses_to_the_same_records(tmp_path):
    """3 000 reads (lower case, IUPAC codes, N / '.'), as FASTQ, tab5, tab6 and QSEQ, plain and gzipped, with LF and CRLF, for several thread counts and
    batch sizes, with -5/-3 and -s/-u: every format gives the line the FASTQ file gives, and that line is what the test computes itself"""
    rng = np.random.default_rng(11)
    n = 3000
    names = [f"M{i % 5}_7_{i % 8}_{1100 + i % 90}_{int(rng.integers(0, 20000))}_{i}_0/1" for i in range(n)]
    seqs = [rand_seq(rng) for _ in range(n)]
    quals = [rand_qual(rng, len(s)) for s in seqs]
    files = write_formats(tmp_path, names, seqs, quals)
    assert set(files) == {"fastq", "tab5", "tab6", "qseq"}
    crlf = write_formats(tmp_path, names, seqs, quals, eol="\r\n", tag="_crlf")
    recs = [(nm, s, q, None) for nm, s, q in zip(names, seqs, quals)]
    for threads, batch in COMBOS:
        want = expected(recs, batch)
        for fmt, path in files.items():
            assert run(FLAG[fmt] + [path, "-p", threads, "--batch", batch]) == want, (fmt, threads, batch)
    want = expected(recs, 1 << 20)
    for fmt, path in files.items():
        assert run(FLAG[fmt] + [gz(path), "-p", 4]) == want, (fmt, "gz")
    for fmt in ("tab5", "tab6", "qseq"):
        assert run(FLAG[fmt] + [crlf[fmt], "-p", 3]) == want, (fmt, "crlf")
    assert run(["--12", files["tab5"]]) == want
    # -5 / -3 apply per read, -s / -u count records
    t5, t3, skip, upto = 3, 5, 100, 500
    trecs = [(nm,) + trimmed(s, q, t5, t3) + (None,) for nm, s, q in zip(names, seqs, quals)][skip:skip + upto]
    want = expected(trecs, 700)
    for fmt, path in files.items():
        assert run(FLAG[fmt] + [path, "-p", 2, "--batch", 700, "-5", t5, "-3", t3, "-s", skip, "-u", upto]) == want, (fmt, "trim")


def short_record_set(rng, n=600, short=(0, 1, 2, 8, 9)):
    """names, sequences and qualities with records of 0, 1, 2, 8 and 9 bases among ordinary ones (-5 3 -3 5 cuts those of 2, 3, 4 and 8 to 0 and those of 9 to 1);
    the shortest kind comes first, twice in a row, and last"""
    names = [f"M{i % 5}_7_{i % 8}_{1100 + i % 90}_{int(rng.integers(0, 20000))}_{i}_0/1" for i in range(n)]
    lens = [int(rng.choice(short)) if rng.random() < 0.4 else int(rng.integers(30, 160)) for _ in range(n)]
    lens[0] = lens[7] = lens[8] = lens[-1] = min(short)
    seqs = ["".join(rng.choice(list("ACGTNacgtRY"), size=k)) for k in lens]
    quals = [rand_qual(rng, k) for k in lens]
    return names, seqs, quals


TRIM5, TRIM3 = 3, 5
TAB_SHORT = (3, 4, 8, 9)      # under -5 3 the reference's tabbed parser aborts on a record of fewer than 3 bases: see test_records_of_zero_and_one_bases


def mixed_short_lines(rng, fmt, n=600, short=(0, 1, 2, 8, 9)):
    """a tabbed file of pairs and unpaired reads whose mates are empty, one base long or ordinary, each on its own -> (lines, records as expected() takes them)"""
    draw = lambda: "".join(rng.choice(list("ACGT"), size=int(rng.choice(short)) if rng.random() < 0.4 else int(rng.integers(30, 160))))   # noqa: E731
    recs, lines = [], []
    for i in range(n):
        nm = "r%d" % i
        s1, s2 = draw(), draw()
        q1, q2 = rand_qual(rng, len(s1)), rand_qual(rng, len(s2))
        if rng.integers(0, 2):
            lines.append(f"{nm}\t{s1}\t{q1}\t{s2}\t{q2}" if fmt == "tab5" else f"{nm}\t{s1}\t{q1}\tm{i}\t{s2}\t{q2}")
            recs.append((nm, s1, q1, (nm if fmt == "tab5" else "m%d" % i, s2, q2)))
        else:
            lines.append(f"{nm}\t{s1}\t{q1}")
            recs.append((nm, s1, q1, None))
    return lines, recs


def length_warnings(recs):
    """the reference's two warnings per read or mate of fewer than 2 bases (hisat2.cpp:3017-3052, :3417-3432), for records as expected() takes them"""
    from ragged_cases import length_warnings as model
    return model([[(r[0], len(codes_of(r[1])))] + ([(r[3][0], len(codes_of(r[3][1])))] if r[3] is not None else []) for r in recs])


def skip_warnings(stderr):
    return [l for l in stderr.split("\n") if l.startswith("Warning: skipping read '") or l.startswith("Warning: skipping mate #")]


def run_warnings(args):
    """the length-filter warnings `--parse-only` writes to stderr: those of a run over the same records"""
    return skip_warnings(subprocess.run([CLI, "--parse-only", "-x", "unused"] + [str(a) for a in args], check=True, capture_output=True, text=True).stderr)


def trim_all(recs):
    t = lambda r: (r[0],) + trimmed(r[1], r[2], TRIM5, TRIM3)      # noqa: E731
    return [t(r) + (None if r[3] is None else t(r[3]),) for r in recs]


def test_records_of_zero_and_one_bases(tmp_path):
    """records without bases and with one base, and -5 / -3 values that cut reads down to 0 or 1 bases, in FASTQ, tab5, tab6, --12 and QSEQ, as mates of tabbed
    pairs and of -1/-2 files, for several thread counts and batch sizes: every record stays a record (none is dropped or merged with its neighbour), with its name
    and an empty sequence.  That this is what the reference does with each of these files is test_the_reference_keeps_records_of_zero_and_one_bases's to show.
    One record kind is left out for the tabbed formats (--tab5, --tab6, --12), and only under -5: a record with fewer bases than -5 takes away.  The reference ends
    such a run with "Error: Read ... has more read characters than quality values." (its tabbed parser trims the sequence while it reads it and then counts the
    qualities against the untrimmed length); the trimmed tabbed runs use records of 3 bases and more (TAB_SHORT), which -5 3 -3 5 still cuts to 0 and 1, and
    the refusal itself is asserted."""
    rng = np.random.default_rng(21)
    names, seqs, quals = short_record_set(rng)
    files = write_formats(tmp_path, names, seqs, quals)
    assert set(files) == {"fastq", "tab5", "tab6", "qseq"}
    recs = [(nm, s, q, None) for nm, s, q in zip(names, seqs, quals)]
    assert sum(1 for s in seqs if len(s) == 0) > 40 and sum(1 for s in seqs if len(s) == 1) > 20
    tn, ts, tq = short_record_set(rng, short=TAB_SHORT)
    tfiles = write_formats(tmp_path, tn, ts, tq, tag="_t")
    trecs = {"fastq": trim_all(recs), "qseq": trim_all(recs)}
    trecs["tab5"] = trecs["tab6"] = trim_all([(nm, s, q, None) for nm, s, q in zip(tn, ts, tq)])
    for t in trecs.values():
        assert sum(1 for x in t if len(x[1]) == 0) > 40 and sum(1 for x in t if len(x[1]) == 1) > 20
    trim = ["-5", TRIM5, "-3", TRIM3]
    for threads, batch in COMBOS:
        for fmt, path in files.items():
            assert run(FLAG[fmt] + [path, "-p", threads, "--batch", batch]) == expected(recs, batch), (fmt, threads, batch)
            tpath = tfiles[fmt] if fmt.startswith("tab") else path
            assert run(FLAG[fmt] + [tpath, "-p", threads, "--batch", batch] + trim) == expected(trecs[fmt], batch), (fmt, threads, batch, "trim")
    assert run(["--12", files["tab5"]]) == expected(recs, 1 << 20)
    assert run(["--12", tfiles["tab5"]] + trim) == expected(trecs["tab5"], 1 << 20)
    # the length-filter warnings: two per read of fewer than 2 bases after trimming, in record order, once each whatever the windows and threads; none with --quiet
    for fmt, path in files.items():
        tpath = tfiles[fmt] if fmt.startswith("tab") else path
        assert run_warnings(FLAG[fmt] + [path, "-p", 3, "--batch", 70]) == length_warnings(recs) != [], fmt
        assert run_warnings(FLAG[fmt] + [tpath, "-p", 3, "--batch", 70] + trim) == length_warnings(trecs[fmt]), (fmt, "trim")
        assert run_warnings(FLAG[fmt] + [path, "--quiet"]) == [], fmt
    assert run(FLAG["fastq"] + [gz(files["fastq"]), "-p", 4]) == expected(recs, 1 << 20)
    for flag in (["--tab5", files["tab5"]], ["--tab6", files["tab6"]], ["--12", files["tab5"]]):     # the reference's refusal, word for word
        p = subprocess.run([CLI, "--parse-only", "-x", "unused"] + [str(a) for a in flag + trim], capture_output=True, text=True)
        assert p.returncode == 1 and f"Error: Read {names[0]} has more read characters than quality values." in p.stderr.split("\n"), p
    for fmt in ("tab5", "tab6"):
        for short, tr in (((0, 1, 2, 8, 9), []), (TAB_SHORT, trim)):
            lines, mrecs = mixed_short_lines(rng, fmt, short=short)
            path = tmp_path / f"mixed_short{len(tr)}.{fmt}"
            path.write_text("\n".join(lines) + "\n")
            want = trim_all(mrecs) if tr else mrecs
            for threads, batch in COMBOS:
                assert run([f"--{fmt}", path, "-p", threads, "--batch", batch] + tr) == expected(want, batch), (fmt, threads, batch, tr)
            assert run_warnings([f"--{fmt}", path, "-p", 2, "--batch", 50] + tr) == length_warnings(want), (fmt, tr)       # "mate #1 of read" / "mate #2 of read" for a pair's
    # -1/-2 with -U: mates and unpaired reads of 0, 1, 2, 8, 9 and more bases as three FASTQ files, plain and trimmed
    _, mrecs = mixed_short_lines(rng, "tab6")
    pairs = [r for r in mrecs if r[3] is not None]
    singles = [r for r in mrecs if r[3] is None]
    for fn, rs in (("s_1.fq", [r[:3] for r in pairs]), ("s_2.fq", [r[3] for r in pairs]), ("s_u.fq", [r[:3] for r in singles])):
        (tmp_path / fn).write_text("".join(f"@{nm}\n{s}\n+\n{q}\n" for nm, s, q in rs))
    args = ["-q", "-1", tmp_path / "s_1.fq", "-2", tmp_path / "s_2.fq", "-U", tmp_path / "s_u.fq"]
    for threads, batch in COMBOS:
        wins = [range(b0, min(len(pairs), b0 + batch)) for b0 in range(0, len(pairs), batch)] + [range(len(pairs) + b0, len(pairs) + min(len(singles), b0 + batch)) for b0 in range(0, len(singles), batch)]
        assert run(args + ["-p", threads, "--batch", batch]) == expected(pairs + singles, batch, wins), (threads, batch)
        assert run(args + ["-p", threads, "--batch", batch] + trim) == expected(trim_all(pairs + singles), batch, wins), (threads, batch, "trim")
    assert run_warnings(args + ["-p", 4, "--batch", 64]) == length_warnings(pairs + singles)
    assert run_warnings(args + ["-p", 4, "--batch", 64] + trim) == length_warnings(trim_all(pairs + singles))


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "hisat2-align-s")), reason="needs oracle/_ref")
def test_the_reference_keeps_records_of_zero_and_one_bases(tmp_path, g1_index):
    """what test_records_of_zero_and_one_bases expects is what the reference does: one run of hisat2-align-s per format, and one with -5 3 -3 5, over the same
    files; its SAM has one line per read or mate, in record order, under the record's name, with the sequence length the test computes ('*' for none).  The
    reference takes an empty record in every one of these formats, also as the first and as the last record of a file (only its FASTA parser drops an empty last
    record; there is no FASTA file here).  What it refuses is a tabbed record of fewer bases than -5 takes away: that run ends with an error, here as there."""
    ref = os.path.join(ROOT, "oracle", "_ref", "hisat2-align-s")
    rng = np.random.default_rng(21)
    names, seqs, quals = short_record_set(rng)
    files = write_formats(tmp_path, names, seqs, quals)
    tn, ts, tq = short_record_set(rng, short=TAB_SHORT)
    tfiles = write_formats(tmp_path, tn, ts, tq, tag="_t")
    trim = ["-5", TRIM5, "-3", TRIM3]

    def ref_run(args):
        return subprocess.run([ref, "-p", "1", "--no-spliced-alignment", "-x", g1_index] + [str(a) for a in args], capture_output=True, text=True)

    def ref_records(args):
        p = ref_run(args)
        assert p.returncode == 0, p.stderr[-500:]
        assert skip_warnings(p.stderr) == run_warnings(args)              # the warnings on stderr: the reference's own, line for line
        return [(t[0], 0 if t[9] == "*" else len(t[9])) for t in (l.split("\t") for l in p.stdout.splitlines() if not l.startswith("@")) if not int(t[1]) & 256]

    def lengths(ns, ss, qs, tr):
        return [(nm, len(codes_of(trimmed(s, q, TRIM5, TRIM3)[0] if tr else s))) for nm, s, q in zip(ns, ss, qs)]

    for fmt, path in list(files.items()) + [("--12", files["tab5"])]:
        flag = ["--12"] if fmt == "--12" else FLAG[fmt]
        tabbed = fmt in ("tab5", "tab6", "--12")
        assert ref_records(flag + [path]) == lengths(names, seqs, quals, False), fmt
        if tabbed:
            p = ref_run(flag + [path] + trim)
            assert p.returncode != 0 and f"Error: Read {names[0]} has more read characters than quality values." in p.stderr.split("\n"), (fmt, p.stderr[-300:])
            assert ref_records(flag + [tfiles["tab5" if fmt == "--12" else fmt]] + trim) == lengths(tn, ts, tq, True), (fmt, "trim")
        else:
            assert ref_records(flag + [path] + trim) == lengths(names, seqs, quals, True), (fmt, "trim")
    strip = lambda nm: nm[:-2] if nm.endswith(("/1", "/2")) else nm      # noqa: E731
    for fmt in ("tab5", "tab6"):
        lines, mrecs = mixed_short_lines(rng, fmt)
        path = tmp_path / f"mixed_short.{fmt}"
        path.write_text("\n".join(lines) + "\n")
        flat = sum(([(r[0], len(r[1]))] + ([(r[3][0], len(r[3][1]))] if r[3] is not None else []) for r in mrecs), [])
        assert [(strip(nm), k) for nm, k in ref_records([f"--{fmt}", path])] == flat, fmt


def test_tabbed_file_mixes_pairs_and_unpaired_reads(tmp_path):
    """a line of a tabbed file is a pair or an unpaired read, decided line by line; an empty name becomes the record's number (for both mates); the second mate of a
    tab5 pair carries the pair's name, that of a tab6 pair its own"""
    rng = np.random.default_rng(12)
    n = 3000
    for fmt in ("tab5", "tab6"):
        recs, lines = [], []
        for i in range(n):
            nm = ("r%d extra words" % i) if i % 3 else ""
            s1, s2 = rand_seq(rng), rand_seq(rng)
            q1, q2 = rand_qual(rng, len(s1)), rand_qual(rng, len(s2))
            shown = nm if nm else str(i)
            if rng.integers(0, 2):
                nm2 = ("m%d" % i) if i % 4 else ""
                if fmt == "tab5":
                    lines.append(f"{nm}\t{s1}\t{q1}\t{s2}\t{q2}")
                    recs.append((shown, s1, q1, (shown, s2, q2)))
                else:
                    lines.append(f"{nm}\t{s1}\t{q1}\t{nm2}\t{s2}\t{q2}")
                    recs.append((shown, s1, q1, (nm2 if nm2 else str(i), s2, q2)))
            else:
                lines.append(f"{nm}\t{s1}\t{q1}")
                recs.append((shown, s1, q1, None))
        path = tmp_path / f"mixed.{fmt}"
        path.write_text("\n".join(lines) + "\n")
        npairs = sum(r[3] is not None for r in recs)
        assert 0.4 * n < npairs < 0.6 * n
        for threads, batch in COMBOS:
            got = run([f"--{fmt}", path, "-p", threads, "--batch", batch])
            assert got == expected(recs, batch), (fmt, threads, batch)
            assert got[3:] == (npairs, n - npairs)
        assert run([f"--{fmt}", gz(path), "-p", 4]) == expected(recs, 1 << 20)
        # -1/-2/-U are ignored when tabbed files are given
        assert run([f"--{fmt}", path, "-U", tmp_path / "no_such_file.fq"]) == expected(recs, 1 << 20)


def test_mates_and_unpaired_reads_together(tmp_path):
    """-1/-2 with -U: all pairs first, then all unpaired reads, whose ids (the default names of nameless reads) start again at 0"""
    rng = np.random.default_rng(13)
    npairs, nsingles = 1300, 900

    def reads(k, tag):
        out = []
        for i in range(k):
            s = rand_seq(rng)
            out.append((f"{tag}{i}" if i % 3 else "", s, rand_qual(rng, len(s))))
        return out

    def write(path, rs):
        with open(path, "w") as f:
            for nm, s, q in rs:
                f.write(f"@{nm}\n{s}\n+\n{q}\n")

    m1a, m1b, m2a, m2b = reads(800, "p"), reads(500, "q"), reads(800, "p"), reads(500, "q")
    ua, ub = reads(600, "u"), reads(300, "v")
    for nm, rs in (("a_1", m1a), ("b_1", m1b), ("a_2", m2a), ("b_2", m2b), ("a_u", ua), ("b_u", ub)):
        write(tmp_path / (nm + ".fq"), rs)
    gz(tmp_path / "b_2.fq"), gz(tmp_path / "b_u.fq")
    named = lambda rs: [(nm if nm else str(i), s, q) for i, (nm, s, q) in enumerate(rs)]
    m1, m2, u = named(m1a + m1b), named(m2a + m2b), named(ua + ub)
    recs = [a + (b,) for a, b in zip(m1, m2)] + [a + (None,) for a in u]
    args = ["-q", "-1", f"{tmp_path}/a_1.fq,{tmp_path}/b_1.fq", "-2", f"{tmp_path}/a_2.fq,{tmp_path}/b_2.fq.gz", "-U", f"{tmp_path}/a_u.fq,{tmp_path}/b_u.fq.gz"]
    for threads, batch in COMBOS:
        # a window never holds records of both segments
        wins = [range(b0, min(npairs, b0 + batch)) for b0 in range(0, npairs, batch)] + [range(npairs + b0, npairs + min(nsingles, b0 + batch)) for b0 in range(0, nsingles, batch)]
        got = run(args + ["-p", threads, "--batch", batch])
        assert got[0] == npairs + nsingles and got[3:] == (npairs, nsingles)
        assert got == expected(recs, batch, wins), (threads, batch)
    # -s / -u count the records of each segment; a -u that ends inside the pairs ends the run there (the reference's worker stops at the first record past it)
    assert run(args + ["-s", 100, "-u", 600]) == expected(recs[100:700], 1 << 20)
    sel = recs[100:npairs] + recs[npairs + 100:]
    assert run(args + ["-s", 100, "-u", 1200]) == expected(sel, 0, [range(0, npairs - 100), range(npairs - 100, len(sel))])
    assert run(args + ["-u", 1300])[3:] == (1300, 900) and run(args + ["-u", 1299])[3:] == (1299, 0)


def solexa_to_phred(sol):
    """Q_phred = 10 log10(10^(Q_solexa / 10) + 1), rounded to the nearest integer (Cock et al. 2010, the FASTQ format paper)"""
    return int(round(10.0 * math.log10(10.0 ** (sol / 10.0) + 1.0)))


def test_quality_encodings(tmp_path):
    """the same qualities as Phred+33, Phred+64, Solexa+64, Phred integers and Solexa integers give the same checksum, in FASTQ, tab5 and QSEQ"""
    rng = np.random.default_rng(14)
    n = 400
    names = [f"M_1_2_3_4_{i}_0/1" for i in range(n)]
    seqs = ["".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=int(rng.integers(30, 120)))) for _ in range(n)]
    sol = [rng.integers(-5, 41, size=len(s)) for s in seqs]
    phred = [[solexa_to_phred(int(x)) for x in q] for q in sol]
    assert {solexa_to_phred(s) for s in (-5, -1, 0, 1, 5, 9, 10, 20, 40)} == {1, 3, 4, 6, 10, 20, 40}
    enc = {
        "phred33": ([], ["".join(chr(33 + x) for x in q) for q in phred]),
        "phred64": (["--phred64"], ["".join(chr(64 + x) for x in q) for q in phred]),
        "solexa": (["--solexa-quals"], ["".join(chr(64 + int(x)) for x in q) for q in sol]),
        "int": (["--int-quals"], [" ".join(str(x) for x in q) for q in phred]),
        "solexa_int": (["--solexa-quals", "--integer-quals"], [" ".join(str(int(x)) for x in q) for q in sol]),
    }
    want = expected([(nm, s, "".join(chr(33 + x) for x in q), None) for nm, s, q in zip(names, seqs, phred)], 1 << 20)
    for tag, (opts, quals) in enc.items():
        files = write_formats(tmp_path, names, seqs, quals, tag="_" + tag)
        for fmt, path in files.items():
            if fmt == "tab6":
                continue
            assert run(FLAG[fmt] + [path] + opts) == want, (tag, fmt)
    # the encodings are told apart: the Phred+64 file read as Phred+33 gives other qualities
    assert run(["-q", "-U", tmp_path / "u_phred64.fq"]) != want


@pytest.mark.parametrize("what", ["too_few_tab5", "too_few_tab6_mate2", "too_few_fastq", "too_few_qseq", "too_many_fastq", "space_tab5", "space_fastq"])
def test_quality_count_errors(tmp_path, what):
    """the reference's messages (pat.cpp:1505-1523) and exit status 1"""
    seq = "ACGTACGTACGTACGTACGTACGTACGTACGTAC"
    q = "I" * len(seq)
    few = "Error: Read r1 has more read characters than quality values."
    many = "Error: Read r1 has more quality values than read characters."
    space = ("Error: Encountered one or more spaces while parsing the quality string for read r1.  If this is a FASTQ file with integer (non-ASCII-encoded) "
             "qualities, try re-running with the --integer-quals option.")
    cases = {
        "too_few_tab5": (["--tab5"], f"r0\t{seq}\t{q}\nr1\t{seq}\t{q[:-2]}\n", few),
        "too_few_tab6_mate2": (["--tab6"], f"r0\t{seq}\t{q}\nr0\t{seq}\t{q}\tr1\t{seq}\t{q[:-1]}\n", few),
        "too_few_fastq": (["-q", "-U"], f"@r0\n{seq}\n+\n{q}\n@r1\n{seq}\n+\n{q[:-1]}\n", few),
        "too_few_qseq": (["--qseq", "-U"], "\t".join(["M", "1", "2", "3", "4", "5", "6", "1", seq, q[:-3], "1"]) + "\n", few.replace("r1", "M_1_2_3_4_5_6/1")),
        "too_many_fastq": (["-q", "-U"], f"@r0\n{seq}\n+\n{q}\n@r1\n{seq}\n+\n{q}II\n", many),
        "space_tab5": (["--tab5"], f"r1\t{seq}\t{q[:10]} {q[11:]}\n", space),
        "space_fastq": (["-q", "-U"], f"@r1\n{seq}\n+\n{q[:10]} {q[11:]}\n", space),
    }
    opts, text, msg = cases[what]
    path = tmp_path / "bad.txt"
    path.write_text(text)
    p = subprocess.run([CLI, "--parse-only", "-x", "unused"] + opts + [str(path)], capture_output=True, text=True)
    assert p.returncode == 1, p
    assert msg in p.stderr.split("\n"), p.stderr


def test_read_file_names(tmp_path):
    """--un-conc <arg> and its kin write two files named after <arg>: every % becomes 1 / 2; else .1 / .2 goes before the last extension; else it is appended;
    a directory gets un-conc-mate.1 / .2 (un-seqs, al-seqs for the unpaired kinds)"""
    d = tmp_path / "outdir"
    d.mkdir()
    fq = tmp_path / "r.fq"
    fq.write_text("@r\nACGTACGTACGTACGTACGTACGTACGTACGTAC\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n")
    table = [
        ("--un-conc", f"{tmp_path}/x%y%.fq", (f"{tmp_path}/x1y1.fq", f"{tmp_path}/x2y2.fq")),
        ("--al-conc-gz", f"{tmp_path}/reads.fq.gz", (f"{tmp_path}/reads.fq.1.gz", f"{tmp_path}/reads.fq.2.gz")),
        ("--al-conc-disc", f"{tmp_path}/noext", (f"{tmp_path}/noext.1", f"{tmp_path}/noext.2")),
        ("--un-conc-gz", str(d), (f"{d}/un-conc-mate.1", f"{d}/un-conc-mate.2")),
        ("--al-conc", "plain.fastq", ("plain.1.fastq", "plain.2.fastq")),
        ("--un", str(d), (f"{d}/un-seqs",)),
        ("--al-gz", f"{tmp_path}/al.fq.gz", (f"{tmp_path}/al.fq.gz",)),
    ]
    for opt, arg, names in table:
        out = subprocess.run([FRONT, "--parse-only", "-x", "unused", "-q", "-U", str(fq), opt, arg], check=True, capture_output=True, text=True).stdout.split("\n")
        assert out[1].split("\t") == [opt] + list(names), (opt, arg, out)
    for opt in ("--un-bz2", "--al-conc-lz4"):
        p = subprocess.run([FRONT, "--parse-only", "-x", "unused", "-q", "-U", str(fq), opt, str(d)], capture_output=True, text=True)
        assert p.returncode == 1 and opt in p.stderr and "-bz2 / -lz4" in p.stderr, p
    p = subprocess.run([FRONT, "-x", "unused", "-c", "-U", "ACGTACGTACGTACGTACGTACGTACGT", "--un", str(d)], capture_output=True, text=True)
    assert p.returncode == 1 and "-c / -r" in p.stderr, p
    # the binary on its own refuses them, as hisat2-align-s does
    p = subprocess.run([CLI, "--parse-only", "-x", "unused", "-q", "-U", str(fq), "--al-conc-gz", str(d)], capture_output=True, text=True)
    assert p.returncode == 1 and "--al-conc-gz is not built into hisat2-align-amd itself" in p.stderr and "hisat2-amd" in p.stderr, p


def test_golden_read_sets_are_regenerable():
    """tests/golden/readsets_pe_in_{1,2}.fq.gz and readsets_tab_in.tab5.gz are what readsets_util.golden_inputs() generates from the golden genome (the other
    readsets_* files are what the reference's `hisat2` script wrote for them: tests/test_gpu_readsets.py)"""
    import readsets_util as R
    gold = os.path.join(ROOT, "tests", "golden")
    pe, tab = R.golden_inputs(R.load_genome(gold))
    text = lambda fn: gzip.open(os.path.join(gold, fn), "rt").read()
    assert text("readsets_pe_in_1.fq.gz") == "".join(f"@{r[0]}\n{r[1]}\n+\n{r[2]}\n" for r in pe)
    assert text("readsets_pe_in_2.fq.gz") == "".join(f"@{r[0]}\n{r[3]}\n+\n{r[4]}\n" for r in pe)
    assert text("readsets_tab_in.tab5.gz") == "".join("\t".join(r) + "\n" for r in tab)
