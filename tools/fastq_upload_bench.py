#!/usr/bin/env python3
"""Times the two ways of making FASTQ pairs resident on a stream: h2g_set_reads_fastq (the text uploaded, parsed on the device) against the path without it — the
command line's host parser over the same bytes (tools/fastq_host_parse.cpp, built here as a shared library and called from this process: Source / Reader as the parser
thread runs them, <threads> threads per mate file) plus h2g_set_reads + h2g_set_read_names + h2g_set_mates on host-made arrays — all three in this one process,
alternating (device call, host parse, three calls, ...), after a warm-up of each.  Records the medians
and spread, the bytes each path uploads, the HIP-event time of the parse kernels and their store rate.  Needs a GPU; prints one JSON line and writes it to --out.

    python tools/fastq_upload_bench.py --index <ht2 base> [--pairs 1000000] [--repeats 7] [--threads 16] [--out file.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hisat2_amd import api, synth


def host_arrays(reads, start_id, suffix, text):
    """the arrays a parser makes of the file written by synth.write_reads_fastq (fixed length: the qualities sit at fixed places of every record of one id width)"""
    n, L = reads.shape
    names = [b"%d" % (start_id + i) + suffix for i in range(n)]
    noffs = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.uint32)
    t = np.frombuffer(text, dtype=np.uint8)
    quals = np.empty((n, L), dtype=np.uint8)
    at, lo = 0, 0
    while lo < n:
        w = len(str(start_id + lo))
        hi = min(n, 10 ** w - start_id)
        rec = 1 + w + len(suffix) + 1 + L + 3 + L + 1
        quals[lo:hi] = t[at:at + (hi - lo) * rec].reshape(hi - lo, rec)[:, rec - 1 - L:rec - 1]
        at += (hi - lo) * rec
        lo = hi
    codes, offs = synth.flatten_reads(reads)
    return codes, offs, quals.reshape(-1), (b"".join(names), noffs)


def host_parser(tmp):
    """the command line's parser as a function of this process: (f1, f2, threads) -> seconds for one pass over the two files"""
    so = os.path.join(tmp, "libfastq_host_parse.so")
    libdir = os.path.join(ROOT, "hisat2_amd")      # (the record stream's -F branch names the window planner of libh2g.so)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "fastq_host_parse.cpp"), "-L" + libdir, "-lh2g", "-Wl,-rpath," + libdir,
                    "-lpthread", "-lz"], check=True)
    lib = C.CDLL(so)
    os.remove(so)
    f = lib.fastq_host_parse
    f.restype = C.c_double
    f.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]

    def parse(f1, f2, threads):
        n, nb = C.c_uint64(), C.c_uint64()
        dt = f(f1.encode(), f2.encode(), threads, 1 << 20, C.byref(n), C.byref(nb))
        return dt, n.value, nb.value
    return parse


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index", required=True)
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, L = a.pairs, 101
    rng = np.random.default_rng(5)
    contigs = [rng.integers(0, 4, size=2_000_000, dtype=np.uint8)]
    m1, m2 = synth.make_pairs(contigs, n, L, 7)
    tmp = tempfile.mkdtemp(prefix="fqbench")
    f1, f2 = (os.path.join(tmp, x) for x in ("r1.fq", "r2.fq"))
    synth.write_reads_fastq(f1, m1, seed=1, suffix=b"/1")
    synth.write_reads_fastq(f2, m2, seed=2, suffix=b"/2")
    t1, t2 = open(f1, "rb").read(), open(f2, "rb").read()
    h1, h2 = host_arrays(m1, 0, b"/1", t1), host_arrays(m2, 0, b"/2", t2)
    ix = api.Index(a.index)
    st = api.Stream(ix, max_reads=n, max_bases=n * L)

    def device():
        return st.set_reads_fastq(t1, t2)

    def three():
        st.set_reads(h1[0], h1[1], h1[2])
        st.set_read_names(h1[3])
        st.set_mates(h2[0], h2[1], h2[3], h2[2])
    parse = host_parser(tmp)

    def host():
        dt, nrec, nb = parse(f1, f2, a.threads)
        assert nrec == n and nb == 2 * n * L, (nrec, nb)
        return dt
    for f in (device, host, three, device, host, three):       # warm-up: code objects, the buffers' first allocation and first touch, the files mapped and faulted in
        f()
    td, t3, tk, tp = [], [], [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter(); res = device(); td.append(time.perf_counter() - t0)
        tk.append(st.fastq_stats().kernel_ms)
        tp.append(host())
        t0 = time.perf_counter(); three(); t3.append(time.perf_counter() - t0)
    res = device()
    s = st.fastq_stats()
    ok = res.n_records == n and res.n_not_plain == 0
    for mate, h in ((0, h1), (1, h2)):
        got = st.fetch_read_set(mate)
        ok = ok and bool(np.array_equal(got["codes"], h[0]) and np.array_equal(got["offs"], h[1]) and np.array_equal(got["quals"], h[2]) and got["names"] == h[3][0]
                         and np.array_equal(got["name_offs"], h[3][1]))
    st.close()
    ix.close()
    med = lambda v: float(np.median(v))
    row = {"pairs": n, "read_len": L, "identical_to_host_arrays": bool(ok), "repeats": a.repeats,
           "device_call_ms_median": med(td) * 1e3, "device_call_ms_min": min(td) * 1e3, "device_call_ms_max": max(td) * 1e3,
           "kernel_ms_median": med(tk), "kernel_ms_min": float(min(tk)), "kernel_ms_max": float(max(tk)),
           "kernel_bytes_written": int(s.bytes_written), "kernel_store_GBps": s.bytes_written / (med(tk) * 1e-3) / 1e9,
           "three_calls_ms_median": med(t3) * 1e3, "three_calls_ms_min": min(t3) * 1e3, "three_calls_ms_max": max(t3) * 1e3,
           "host_parse_threads": a.threads, "host_parse_ms_median": med(tp) * 1e3, "host_parse_ms_min": min(tp) * 1e3, "host_parse_ms_max": max(tp) * 1e3,
           "parent_path_ms_median": (med(tp) + med(t3)) * 1e3,
           "bytes_uploaded_device": int(s.bytes_uploaded), "bytes_uploaded_three_calls": int(sum(x.nbytes for h in (h1, h2) for x in h[:3]) + sum(len(h[3][0]) + h[3][1].nbytes for h in (h1, h2)))}
    print(json.dumps(row))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(row, f, indent=1)
    for x in (f1, f2):
        os.remove(x)
    os.rmdir(tmp)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
