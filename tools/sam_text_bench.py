#!/usr/bin/env python3
"""Times the three ways from a finished paired run to its SAM text, in one process, alternating, after a warm-up of each:
  (a) h2g_align_pairs_fetch_compact + h2g_sam_format_paired_compact on the host at 1, 8 and 32 threads — the path the command line takes by default;
  (b) h2g_align_pairs_fetch_compact + h2g_sam_plan_paired_compact (host, same thread counts) + h2g_sam_text_paired (device), split into plan / the text call's
      upload + copy-back (its wall time less its kernels) / kernels (HIP events; the write kernel alone as well);
  (c) h2g_align_pairs_fetch_compact + h2g_sam_text_paired_planned: plain pairs classified and planned on the device, the host planner (same thread counts) over the
      handed-on pairs only, merged on the device — its wall time, the planner + merge kernels, the host subset's time and share, the bytes uploaded, the share handed on.
Medians of --repeats rounds into --out (for the host's format call the smallest and the largest round as well: their distance is the margin a comparison of two
builds has to allow), with the write kernel's store rate against the bytes it writes and the planner's share of (b).  --legs a times (a) alone.  --key <name> keeps
the result under that name beside the other names --out already holds (two builds of the library, H2G_LIB, side by side: one name per commit).  Needs a GPU.

    python tools/sam_text_bench.py --index <ht2 base> --genome <fasta[.gz]> [--pairs 1000000] [--repeats 7] [--legs abc] [--key <name>] [--out profiles/sam_text.json]"""
import argparse
import ctypes as C
import gzip
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hisat2_amd import api, synth

CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    CODE[_c] = CODE[_c + 32] = _i


def load_fasta(path):
    op = gzip.open if path.endswith(".gz") else open
    contigs, cur = [], []
    with op(path, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                if cur:
                    contigs.append(CODE[np.frombuffer(b"".join(cur), dtype=np.uint8)])
                cur = []
            else:
                cur.append(line.strip())
    if cur:
        contigs.append(CODE[np.frombuffer(b"".join(cur), dtype=np.uint8)])
    return contigs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index", required=True)
    ap.add_argument("--genome", required=True)
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--threads", default="1,8,32")
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--key", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_text.json"))
    a = ap.parse_args()
    n = a.pairs
    contigs = load_fasta(a.genome)
    m1, m2 = synth.make_pairs(contigs, n, 101, 20261020, frag_mean=300, frag_sd=30, sub_rate=0.01)
    c1, o1 = synth.flatten_reads(np.stack(m1)); c2, o2 = synth.flatten_reads(np.stack(m2))
    rng = np.random.default_rng(1)
    q1 = rng.integers(33, 74, size=c1.size, dtype=np.uint8); q2 = rng.integers(33, 74, size=c2.size, dtype=np.uint8)
    nb, no = api.Stream.pack_names(["read%d" % i for i in range(n)])
    ix = api.Index(a.index, device=0)
    st = api.Stream(ix, max_reads=n, max_bases=c1.size)
    st.set_reads(c1, o1, q1); st.set_read_names((nb, no)); st.set_mates(c2, o2, (nb, no), q2)
    p = st.align_params()
    st.align_pairs_run(p)
    L = api.lib()
    vp, sz = C.c_void_p, C.c_size_t
    L.h2g_sam_open.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.h2g_sam_set_threads.argtypes = [vp, C.c_int]
    L.h2g_sam_format_paired_compact.argtypes = [vp] * 11 + [sz] + [vp] * 5 + [C.c_uint32, vp, sz, C.POINTER(sz)]
    h = vp()
    assert L.h2g_sam_open(a.index.encode(), C.byref(h)) == 0
    pool = api.PinnedPool()
    s1, s2 = (c1, o1, q1, nb, no), (c2, o2, q2, nb, no)
    ptrs = [api._ptr(x) for x in s1 + s2]
    cap = 1400 * n + 4096
    text_buf = pool.array("text", cap)
    khits = int(p.khits)

    def fetch():
        t0 = time.perf_counter()
        r = st.align_pairs_fetch_compact(pinned=pool)
        return r, time.perf_counter() - t0

    def host(threads):
        L.h2g_sam_set_threads(h, threads)
        (res, r1, b1, r2, b2), tf = fetch()
        used = sz(0)
        t0 = time.perf_counter()
        assert L.h2g_sam_format_paired_compact(h, *ptrs, n, res.ctypes.data, r1.ctypes.data, b1.ctypes.data, r2.ctypes.data, b2.ctypes.data, khits, text_buf.ctypes.data, cap, C.byref(used)) == 0
        return {"fetch": tf, "format": time.perf_counter() - t0, "bytes": used.value}, text_buf[:used.value].tobytes() if threads == 1 else None

    plan_bufs = {"lines": np.zeros(2 * n + 16, dtype=api.SAM_LINE_DTYPE), "aux": np.zeros(64 * n + 4096, dtype=np.uint8)}
    dev_buf = pool.array("devtext", cap)

    def device(threads):
        L.h2g_sam_set_threads(h, threads)
        (res, r1, b1, r2, b2), tf = fetch()
        nl, na, used = sz(0), sz(0), sz(0)
        plan = lambda: L.h2g_sam_plan_paired_compact(h, *ptrs, n, res.ctypes.data, r1.ctypes.data, b1.ctypes.data, r2.ctypes.data, b2.ctypes.data, khits, plan_bufs["lines"].ctypes.data,
                                                     len(plan_bufs["lines"]), C.byref(nl), plan_bufs["aux"].ctypes.data, len(plan_bufs["aux"]), C.byref(na), None)
        t0 = time.perf_counter()
        rc = plan()
        if rc == api.H2G_ERR_ARG and (nl.value > len(plan_bufs["lines"]) or na.value > len(plan_bufs["aux"])):      # (the warm-up round sizes the buffers; nothing was counted)
            plan_bufs["lines"] = np.zeros(nl.value + nl.value // 8, dtype=api.SAM_LINE_DTYPE); plan_bufs["aux"] = np.zeros(na.value + na.value // 8 + 64, dtype=np.uint8)
            t0 = time.perf_counter()
            rc = plan()
        assert rc == 0, rc
        lines, aux = plan_bufs["lines"], plan_bufs["aux"]
        t1 = time.perf_counter()
        loffs = pool.array("loffs", (nl.value + 1) * 8, np.uint64)
        t1b = time.perf_counter()
        assert L.h2g_sam_text_paired(st.h, h, lines.ctypes.data, nl.value, aux.ctypes.data, na.value, dev_buf.ctypes.data, cap, C.byref(used), loffs.ctypes.data) == 0
        t2 = time.perf_counter()
        s = st.sam_text_stats()
        whole = int(((lines["bits"][:nl.value] & api.SAM_LINE_WHOLE_LINE) != 0).sum())
        simple = int(((lines["bits"][:nl.value] & (api.SAM_LINE_WHOLE_LINE | api.SAM_LINE_AUX_CIGAR_MDZ)) == 0).sum())
        return {"fetch": tf, "plan": t1 - t0, "text_call": t2 - t1b, "kernels": s.kernel_ms * 1e-3, "write_kernel": s.write_kernel_ms * 1e-3, "upload_copyback": t2 - t1b - s.kernel_ms * 1e-3,
                "bytes": used.value, "bytes_uploaded": int(s.bytes_uploaded), "lines": nl.value, "aux_bytes": na.value, "whole_lines": whole, "simple_lines": simple}, \
            dev_buf[:used.value].tobytes() if threads == 1 else None

    plan_buf = pool.array("plantext", cap)
    L.h2g_sam_text_paired_planned.argtypes = [vp] * 12 + [sz] + [vp] * 5 + [C.c_uint32, vp, sz, C.POINTER(sz), vp, sz, C.POINTER(sz), vp]
    lcap = {"n": 2 * n + 64}

    def planned(threads):
        L.h2g_sam_set_threads(h, threads)
        (res, r1, b1, r2, b2), tf = fetch()
        used, nl = sz(0), sz(0)
        loffs = pool.array("ploffs", (lcap["n"] + 1) * 8, np.uint64)
        ends = pool.array("pends", n * 8, np.uint64)
        call = lambda lo, lc: L.h2g_sam_text_paired_planned(st.h, h, *ptrs, n, res.ctypes.data, r1.ctypes.data, b1.ctypes.data, r2.ctypes.data, b2.ctypes.data, khits, plan_buf.ctypes.data, cap,
                                                            C.byref(used), lo.ctypes.data, lc, C.byref(nl), ends.ctypes.data)
        t0 = time.perf_counter()
        rc = call(loffs, lcap["n"])
        if rc == api.H2G_ERR_ARG and nl.value > lcap["n"]:            # (the warm-up round sizes the line array; nothing was counted)
            lcap["n"] = nl.value + nl.value // 8
            loffs = pool.array("ploffs", (lcap["n"] + 1) * 8, np.uint64)
            t0 = time.perf_counter()
            rc = call(loffs, lcap["n"])
        assert rc == 0, rc
        t1 = time.perf_counter()
        ps, _ = st.sam_plan_stats()
        s = st.sam_text_stats()
        return {"fetch": tf, "text_call": t1 - t0, "plan_kernels": ps.plan_kernel_ms * 1e-3, "host_subset": ps.host_plan_ms * 1e-3, "text_kernels": s.kernel_ms * 1e-3, "write_kernel": s.write_kernel_ms * 1e-3,
                "bytes": used.value, "bytes_uploaded": int(ps.bytes_uploaded), "lines": nl.value, "device_planned": int(ps.device_planned), "host_planned": int(ps.host_planned)}, \
            plan_buf[:used.value].tobytes() if threads == 1 else None

    threads = [int(t) for t in a.threads.split(",")]
    ref_text = host(1)[1]
    identical = device(1)[1] == ref_text if "b" in a.legs else None               # warm-up of each, and the check that they write the same bytes
    identical_planned = planned(1)[1] == ref_text if "c" in a.legs else None
    rounds = {("host", t): [] for t in threads}
    rounds.update({("device", t): [] for t in threads})
    rounds.update({("planned", t): [] for t in threads})
    for _ in range(a.repeats):
        for t in threads:
            rounds[("host", t)].append(host(t)[0])
            if "b" in a.legs:
                rounds[("device", t)].append(device(t)[0])
            if "c" in a.legs:
                rounds[("planned", t)].append(planned(t)[0])
    med = lambda rows, k: float(np.median([r[k] for r in rows]))
    out = {"pairs": n, "read_length": 101, "repeats": a.repeats, "identical_text": identical, "identical_text_planned": identical_planned,
           "text_bytes": rounds[("host", threads[0])][0]["bytes"], "host": {}, "device": {}, "planned": {}}
    for t in threads:
        hr, dr = rounds[("host", t)], rounds[("device", t)]
        out["host"][str(t)] = {"fetch_ms": med(hr, "fetch") * 1e3, "format_ms": med(hr, "format") * 1e3, "total_ms": (med(hr, "fetch") + med(hr, "format")) * 1e3,
                               "format_min_ms": min(r["format"] for r in hr) * 1e3, "format_max_ms": max(r["format"] for r in hr) * 1e3}
        if "b" not in a.legs or "c" not in a.legs:
            continue
        d = {k + "_ms": med(dr, k) * 1e3 for k in ("fetch", "plan", "text_call", "kernels", "write_kernel", "upload_copyback")}
        d["total_ms"] = d["fetch_ms"] + d["plan_ms"] + d["text_call_ms"]
        d["planner_share_of_plan_plus_text"] = d["plan_ms"] / (d["plan_ms"] + d["text_call_ms"])
        d["write_kernel_store_GBps"] = dr[0]["bytes"] / (med(dr, "write_kernel") or 1e-9) / 1e9
        d.update({k: dr[0][k] for k in ("lines", "aux_bytes", "whole_lines", "simple_lines", "bytes_uploaded")})
        out["device"][str(t)] = d
        pr = rounds[("planned", t)]
        c = {k + "_ms": med(pr, k) * 1e3 for k in ("fetch", "text_call", "plan_kernels", "host_subset", "text_kernels", "write_kernel")}
        c["total_ms"] = c["fetch_ms"] + c["text_call_ms"]
        c["host_subset_share_of_text_call"] = c["host_subset_ms"] / c["text_call_ms"]
        c.update({k: pr[0][k] for k in ("lines", "bytes_uploaded", "device_planned", "host_planned")})
        c["share_handed_on"] = pr[0]["host_planned"] / float(n)
        out["planned"][str(t)] = c
        tot = {"a": out["host"][str(t)]["total_ms"], "b": d["total_ms"], "c": c["total_ms"]}
        c["fastest"] = min(tot, key=tot.get)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.key:
        held = json.load(open(a.out)) if os.path.exists(a.out) else {}
        out = dict({k: v for k, v in held.items() if isinstance(v, dict) and "pairs" in v}, **{a.key: out})
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    L.h2g_sam_close.argtypes = [vp]
    L.h2g_sam_close(h); pool.close(); st.close(); ix.close()


if __name__ == "__main__":
    main()
