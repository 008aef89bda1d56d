"""Helpers of the -F <len>,<step> tests (test_windows_cpu.py, test_gpu_windows.py): a pure-Python restatement of the reference's window source, the checksum of
`hisat2-align-amd --parse-only`, and small FASTA inputs that hold every case the source treats on its own."""
import gzip
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "hisat2_amd", "hisat2-align-amd")
REF = os.path.join(ROOT, "oracle", "_ref")

CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
# asc2dnacat (alphabet.cpp:36-58): 1 = DNA, 2 = IUPAC, 3 = '-'; everything else 0
DNACAT = {c: 1 for c in "ACGTacgt"}
DNACAT.update({c: 2 for c in "BDHKMNRSVWXYbdhkmnrsvwxy"})
DNACAT["-"] = 3


def restate(files, length, step):
    """FastaContinuousPatternSource::read (pat.h:1233-1336) character by character over `files` (bytes each), with the counters the reference keeps: readCnt_ runs on
    across files, the ring / name / eat state restarts at every '>' and every file.  -> [(name, sequence, rdid)] in the order the reads are handed out."""
    out = []
    read_cnt = 0
    for data in files:
        txt = data.decode("latin-1")
        eat, beginning, name, sub = length - 1, True, "", read_cnt        # resetForNextFile()
        ring = []
        i, n = 0, len(txt)
        while i < n:
            c = txt[i]
            i += 1
            if c == ">":
                eat, beginning, name, sub = length - 1, True, "", read_cnt
                ring = []
                saw_space = False
                while i < n and txt[i] not in "\n\r":
                    if not saw_space:
                        saw_space = txt[i] in " \t\n\v\f\r"
                    if not saw_space:
                        name += txt[i]
                    i += 1
                while i < n and txt[i] in "\n\r":
                    i += 1
                name += "_"
                continue
            cat = DNACAT.get(c, 0)
            if cat == 0:
                continue
            ring.append("N" if cat >= 2 else c.upper())
            if len(ring) > 1024:
                ring.pop(0)
            if eat > 0:
                eat -= 1
                if not beginning:
                    read_cnt += 1
                continue
            out.append((name + str(read_cnt - sub), "".join(ring[-length:]), read_cnt))
            eat = (step - 1) & 0xFFFFFFFFFFFFFFFF                         # size_t: a step of 0 never runs out again within a record
            read_cnt += 1
            beginning = False
    return out


def fnv(h, data):
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def expected(reads, batch):
    """what `--parse-only` prints first for `reads` [(name, sequence, rdid)] in windows of `batch`: records, bases, checksum, pairs, unpaired (the checksum of
    test_cli_readsets_cpu.py for unpaired reads without qualities); and the (first, last) rdid of every window"""
    h, bases, ids = 1469598103934665603, 0, []
    for b0 in range(0, len(reads), batch):
        w = reads[b0:b0 + batch]
        codes = [bytes(CODE[c] for c in s) for _, s, _ in w]
        h = fnv(h, b"".join(codes))
        h = fnv(h, "".join(nm for nm, _, _ in w).encode())
        h = fnv(h, b"".join(np.uint32(len(c)).tobytes() + np.uint32(len(nm.encode())).tobytes() for (nm, _, _), c in zip(w, codes)))
        bases += sum(len(c) for c in codes)
        ids.append((w[0][2], w[-1][2]))
    return (len(reads), bases, h, 0, len(reads)), ids


def select(reads, skip, upto):
    """-s / -u on Read::rdid (hisat2.cpp:3319, :3634)"""
    return [r for r in reads if skip <= r[2] < skip + upto]


def sample_files(rng):
    """Two FASTA files (bytes) with: text before the first header, a header with a description, a tab after the name, lowercase, IUPAC letters, a run of N, junk lines
    (digits, '*', blanks; '-' counts as a base that reads N), a record shorter than any window, an empty record, '\\r\\n' line ends, and records long enough for
    1024-base windows."""
    def seq(n, alphabet="ACGT"):
        return "".join(rng.choice(list(alphabet), size=n))

    def wrap(s, w=60, eol="\n"):
        return eol.join(s[k:k + w] for k in range(0, len(s), w)) + eol
    a = wrap(seq(95))                                                     # text before the first '>': names 0, 10, ...
    a += ">qa some description here\n" + wrap(seq(700) + "NNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN" + seq(500))
    a += ">short\nACGTAC\n"
    a += ">empty\n"
    a += ">tab\tafter the name\n" + wrap(seq(300, "ACGTacgtRYKMSWN"), 70)
    a += "-*12\n 34 *\n" + wrap(seq(130)) + "1234\n\n" + wrap(seq(41))
    b = ">qb\r\n" + wrap(seq(1500), 80, "\r\n")
    b += ">qc x\n" + wrap(seq(2300, "ACGTn"), 100)
    return [a.encode(), b.encode()]


def write_files(tmp_path, files, gz_last=True):
    paths = []
    for k, data in enumerate(files):
        p = os.path.join(str(tmp_path), f"w{k}.fa")
        if gz_last and k == len(files) - 1:
            p += ".gz"
            with gzip.open(p, "wb") as f:
                f.write(data)
        else:
            with open(p, "wb") as f:
                f.write(data)
        paths.append(p)
    return paths
