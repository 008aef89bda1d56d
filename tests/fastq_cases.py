"""FASTQ record sets for the device-parse tests (tests/test_fastq_cpu.py, tests/test_gpu_fastq.py): records as (name, sequence, qualities) byte strings, their text,
and the arrays a parser makes of them (the rules of Reader::parse_record, csrc/h2g_cli_reads.h), built here with numpy from the records, not from the text."""
import numpy as np

RAGGED = (0, 1, 15, 16, 17, 63, 64, 65, 100, 128, 129, 250)
CODE = np.zeros(256, np.uint8)              # '.' and n are N, c g t 1 2 3, every other letter A
for _c, _v in ((b"c", 1), (b"g", 2), (b"t", 3), (b"n", 4)):
    CODE[_c[0]] = CODE[_c.upper()[0]] = _v
CODE[ord(".")] = 4
NOT_PLAIN_KINDS = ("empty name", "digit in the sequence", "missing +", "one quality short", "two qualities over", "blank in the qualities", "below 64 under phred64")


def _rand_bytes(rng, alphabet, n):
    a = np.frombuffer(alphabet, np.uint8)
    return a[rng.integers(0, len(a), size=n)].tobytes()


def ragged_records(seed, n, phred64=False):
    """lengths 0 .. 250 and one of 1 000, names of 1 .. 200 bytes, some '.', IUPAC letters and lower case, some records with one quality more than bases"""
    rng = np.random.default_rng(seed)
    plain, odd = b"ACGT", b"ACGTNn.acgtRYKMSWBDHVxU"
    q0 = 64 if phred64 else 33
    recs = []
    for i in range(n):
        L = 1000 if i == n // 2 else RAGGED[int(rng.integers(0, len(RAGGED)))]
        nlen = int(rng.integers(1, 201)) if i % 40 == 0 else int(rng.integers(1, 30))
        name = (b"r%d" % i + _rand_bytes(rng, b"_/:abcXYZ 019", nlen))[:nlen]
        seq = _rand_bytes(rng, odd if i % 8 == 0 else plain, L)
        qual = (rng.integers(q0, q0 + 41, size=L + (1 if i % 11 == 0 else 0), dtype=np.uint8)).tobytes()
        recs.append((name, seq, qual))
    return recs


def fixed_records(seed, n, length=100, phred64=False):
    rng = np.random.default_rng(seed)
    q0 = 64 if phred64 else 33
    return [(b"read_%d" % i, _rand_bytes(rng, b"ACGT", length), rng.integers(q0, q0 + 41, size=length, dtype=np.uint8).tobytes()) for i in range(n)]


def text_of(recs, crlf=False, last_newline=True):
    e = b"\r\n" if crlf else b"\n"
    t = b"".join(b"@" + nm + e + s + e + b"+" + e + q + e for nm, s, q in recs)
    return t if last_newline or not recs else t[:-len(e)]


def expected(recs, trim5=0, trim3=0, phred64=False):
    """dict(codes, offs, quals, names, name_offs, max_len) of the records as a parser leaves them"""
    seqs, quals, lens = [], [], []
    for nm, s, q in recs:
        t5 = min(trim5, len(s))
        L = len(s) - t5 - min(trim3, len(s) - t5)
        seqs.append(s[t5:t5 + L]); quals.append(q[t5:t5 + L]); lens.append(L)
    qual = np.frombuffer(b"".join(quals), np.uint8)
    return {"codes": CODE[np.frombuffer(b"".join(seqs), np.uint8)], "offs": np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.uint32),
            "quals": (qual - 31).astype(np.uint8) if phred64 else qual, "names": b"".join(r[0] for r in recs),
            "name_offs": np.concatenate([[0], np.cumsum([len(r[0]) for r in recs], dtype=np.int64)]).astype(np.uint32), "max_len": max(lens, default=0)}


def break_record(rec, kind, phred64=False):
    """the record made not plain in way `kind` (index into NOT_PLAIN_KINDS) -> its four lines as bytes (LF)"""
    nm, s, q = rec
    assert len(s) >= 30 and len(q) == len(s)
    plus = b"+"
    if kind == 0:
        nm = b""
    elif kind == 1:
        s = s[:7] + b"3" + s[8:]
    elif kind == 2:
        plus = b"-"
    elif kind == 3:
        q = q[:-1]
    elif kind == 4:
        q = q + q[:2]
    elif kind == 5:
        q = q[:11] + b" " + q[12:]
    elif kind == 6:
        q = q[:20] + b"5" + q[21:]
    return b"@" + nm + b"\n" + s + b"\n" + plus + b"\n" + q + b"\n"


def text_with_bad_record(recs, at, kind, phred64=False):
    return text_of(recs[:at]) + break_record(recs[at], kind, phred64) + text_of(recs[at + 1:])


def cli_fixtures(genome, tmp):
    """The read files of the command-line tests: 2 000 pairs and 2 000 unpaired reads (a third of them cross introns), also gzipped, cut into two files (the first
    without a last newline) and with Phred+64 qualities.  Every record of them is plain: tests/test_fastq_cpu.py counts that with the checker, on the CPU.
    -> {key: path}"""
    import gzip
    import os
    import readsets_util as R
    pairs = R.make_records(genome, 901, 2000, pair_frac=1.0, name="p")
    singles = R.make_records(genome, 902, 1400, pair_frac=0.0, name="u") + [r[:3] for r in R.spliced_records(genome, 903, 600, name="s")]
    order = np.random.default_rng(904).permutation(len(singles))
    singles = [singles[i] for i in order]
    text = lambda reads, shift=0: "".join(f"@{nm}\n{s}\n+\n{''.join(chr(ord(c) + shift) for c in q)}\n" for nm, s, q in reads)
    sets = {"m1": [(r[0] + "/1", r[1], r[2]) for r in pairs], "m2": [(r[0] + "/2", r[3], r[4]) for r in pairs], "u": singles}
    out = {}
    for key, reads in sets.items():
        files = {key: text(reads), key + "_a": text(reads[:777])[:-1], key + "_b": text(reads[777:]), key + "_64": text(reads, 31)}
        for k, t in files.items():
            out[k] = os.path.join(str(tmp), k + ".fq")
            with open(out[k], "w") as f:
                f.write(t)
        out[key + "_gz"] = os.path.join(str(tmp), key + ".fq.gz")
        with gzip.open(out[key + "_gz"], "wt") as f:
            f.write(files[key])
    return out
