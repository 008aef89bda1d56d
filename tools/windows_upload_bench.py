#!/usr/bin/env python3
"""Times the two ways of making a -F window set resident on a stream: h2g_set_reads_windows (the text uploaded once, expanded on the device) against
h2g_set_reads + h2g_set_read_names + h2g_set_read_ids on the host-expanded arrays, in one process, alternating, after a warm-up of both.  Per (len, step):
the HIP-event time of the expansion kernels, the wall time of each path up to its synchronise (both paths end in one), the bytes each uploads and the
kernels' store bandwidth.  Needs a GPU; prints one JSON line per (len, step) and writes them to --out.

    python tools/windows_upload_bench.py --index <ht2 base> [--windows 1000000] [--repeats 7] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hisat2_amd import api


def measure(ix, n, length, step, repeats):
    rng = np.random.default_rng(length * 1000 + step)
    text = rng.integers(0, 4, size=(n - 1) * step + length, dtype=np.uint8)
    pre = b"chr1_"
    segs = np.array([(0, 0, 0, n, 0, len(pre), 0)], dtype=api.WINDOW_SEG_DTYPE)
    st = api.Stream(ix, max_reads=n, max_bases=n * length)
    t0 = time.perf_counter()
    codes, offs, names, noffs, ids = api.expand_windows(text, segs, length, step, pre)
    t_expand = time.perf_counter() - t0

    def windows():
        st.set_reads_windows(text, segs, length, step, pre)

    def three():
        st.set_reads(codes, offs)
        st.set_read_names((names, noffs))
        st.set_read_ids(ids)
    for f in (windows, three, windows, three):     # warm-up: code objects, the name buffers' first allocation, first-touch of the device buffers
        f()
    tw, t3, tk = [], [], []
    for _ in range(repeats):
        t0 = time.perf_counter(); windows(); tw.append(time.perf_counter() - t0)
        s = st.windows_stats()
        tk.append(s.kernel_ms)
        t0 = time.perf_counter(); three(); t3.append(time.perf_counter() - t0)
    windows()
    got = st.fetch_reads()
    ok = bool(np.array_equal(got["codes"], codes) and got["names"] == names and np.array_equal(got["ids"], ids))
    s = st.windows_stats()
    st.close()
    med = lambda v: float(np.median(v))
    return {"len": length, "step": step, "windows": n, "identical_to_host_expansion": ok,
            "kernel_ms_median": med(tk), "kernel_ms_min": float(min(tk)), "kernel_ms_max": float(max(tk)),
            "kernel_bytes_written": int(s.bytes_written), "kernel_store_GBps": s.bytes_written / (med(tk) * 1e-3) / 1e9,
            "windows_call_ms_median": med(tw) * 1e3, "windows_call_ms_min": min(tw) * 1e3, "windows_call_ms_max": max(tw) * 1e3,
            "three_calls_ms_median": med(t3) * 1e3, "three_calls_ms_min": min(t3) * 1e3, "three_calls_ms_max": max(t3) * 1e3,
            "bytes_uploaded_windows": int(s.bytes_uploaded), "bytes_uploaded_three_calls": int(codes.nbytes + offs.nbytes + len(names) + noffs.nbytes + ids.nbytes),
            "host_expansion_numpy_ms": t_expand * 1e3, "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index", required=True)
    ap.add_argument("--windows", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ix = api.Index(a.index)
    rows = [measure(ix, a.windows, length, step, a.repeats) for length, step in ((100, 1), (100, 50))]
    ix.close()
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    return 0 if all(r["identical_to_host_expansion"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
