#!/usr/bin/env python3
"""A/B of the fast pass of SPLICED runs (h2g_k_go_fast_spl.hip): N pairs drawn uniformly from a spliced transcript model over the cached benchmark genome, the same
resident batch run K times per process, in alternating repeats of three configurations —
  on      H2G_FAST_SPLICED=1: the pass on,
  off     H2G_FAST_SPLICED=0: the spliced general machine alone (this build),
  parent  the parent commit's libh2g.so loaded through H2G_LIB (when --parent-lib is given)
— each in a process of its own (the library and its switches are read once per process; both switches are set by name, whatever the library's default is).  Reports the share of pairs with a junction, per configuration the ms per
run of every repeat with median / min / max, the completed / handed-on counts and the bail histogram, and the verdict of the acceptance rule: the pass stays on by
default only if its median beats the parent's by more than the parent's own min-max spread.
usage: spliced_fast_ab.py [--genome 4.9e6] [--pairs 1000000] [--repeats 5] [--steps 5] [--parent-lib PATH] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))

RDLEN = 101


def transcript_pairs(contigs, n, seed, sub=0.005):
    """exons of 150..900 bases separated by introns of 60..9000 over every contig; fragments of 180..420 bases uniform over the spliced transcript, --fr mates
    -> m1, m2 (n, 101), share of pairs with a mate that crosses a junction"""
    rng = np.random.default_rng(seed)
    tx, jun, off = [], [], 0
    for g in contigs:
        pos = 1000
        while pos + 12000 < len(g):
            e = int(rng.integers(150, 900))
            tx.append(g[pos:pos + e]); off += e; jun.append(off)
            pos += e + int(rng.choice([60, 90, 150, 400, 1200, 5000, 9000]))
    tx = np.concatenate(tx)
    assert not (tx > 3).any(), "the transcript model needs a genome without N (the junction offsets are offsets into the exons as they are)"
    jun = np.asarray(jun[:-1], dtype=np.int64)
    fl = rng.integers(180, 420, size=n)
    s = rng.integers(0, len(tx) - 420, size=n)
    ar = np.arange(RDLEN)
    left = tx[s[:, None] + ar]
    right = 3 - tx[(s + fl - 1)[:, None] - ar]                 # reverse complement of the fragment's last 101 bases
    for m in (left, right):
        mask = rng.random(m.shape) < sub
        m[mask] = (m[mask] + rng.integers(1, 4, size=int(mask.sum()))) & 3
    flip = rng.random(n) < 0.5
    m1 = np.where(flip[:, None], right, left).astype(np.uint8)
    m2 = np.where(flip[:, None], left, right).astype(np.uint8)

    def crosses(a):                                            # a junction j with a < j < a + 101
        k = np.searchsorted(jun, a, side="right")
        return (k < len(jun)) & (jun[np.minimum(k, len(jun) - 1)] < a + RDLEN)
    return m1, m2, float((crosses(s) | crosses(s + fl - RDLEN)).mean())


def child(base, npz, steps):
    import bench
    from hisat2_amd import api
    d = np.load(npz)
    m1, m2 = d["m1"], d["m2"]
    n = len(m1)
    from hisat2_amd import synth
    c1, o1 = synth.flatten_reads(m1); c2, o2 = synth.flatten_reads(m2)
    ix = api.Index(base, device=0)
    st = api.Stream(ix, max_reads=n, max_bases=n * RDLEN + 64)
    names = [str(i) for i in range(n)]
    st.set_reads(c1, o1); st.set_read_names(names); st.set_mates(c2, o2, names)
    p = st.align_params()
    p.no_spliced_alignment = 0; p.no_temp_splicesite = 1
    for _ in range(2):
        st.align_pairs_run(p)
    st.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        st.align_pairs_run(p)
    st.sync()
    ms = (time.perf_counter() - t0) / steps * 1e3
    c = st.counters()
    out = {"ms_per_run": round(ms, 3), "fast": int(c.n_fast), "handed_on": int(c.n_fast_bail), "aligned": int(c.n_aligned), "overflow": int(c.n_overflow),
           "ms_fast_kernel": round(float(c.ms_fast_kernel), 3)}
    out["bails"] = bench.fast_bail_reasons(api, st) or {}
    st.close(); ix.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=float, default=4.9e6)
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.steps)
    import bench
    glen = int(a.genome)
    import build_bench_index as BB                             # the benchmark's genome profile at this size, cached where bench.py caches its indexes
    base, contigs = BB.build(glen, cache=bench.bench_cache_dir()), BB.genome(glen)
    m1, m2, share = transcript_pairs(contigs, a.pairs, bench.SEED + 909)
    tmp = tempfile.mkdtemp(prefix="h2splab")
    npz = os.path.join(tmp, "pairs.npz")
    np.savez(npz, m1=m1, m2=m2)
    configs = [("on", {"H2G_FAST_SPLICED": "1"}), ("off", {"H2G_FAST_SPLICED": "0"})]
    if a.parent_lib:
        configs.append(("parent", {"H2G_LIB": os.path.abspath(a.parent_lib)}))
    runs = {k: [] for k, _ in configs}
    for rep in range(a.repeats):
        for k, env in configs:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--child", base, npz], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit("configuration %s failed (exit %d): %s" % (k, r.returncode, r.stderr[-1500:]))
            runs[k].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps({"repeat": rep, "config": k, **runs[k][-1]}), flush=True)
    res = {"genome_bp": glen, "pairs": a.pairs, "share_with_junction": round(share, 4), "steps_per_process": a.steps, "configs": {}}
    for k, _ in configs:
        ms = [x["ms_per_run"] for x in runs[k]]
        res["configs"][k] = {"ms": ms, "median": round(statistics.median(ms), 3), "min": min(ms), "max": max(ms), "fast": runs[k][-1]["fast"], "handed_on": runs[k][-1]["handed_on"],
                             "aligned": runs[k][-1]["aligned"], "bails": runs[k][-1].get("bails", {})}
    if res["configs"]["on"]["fast"] == 0 or res["configs"]["off"]["fast"] != 0:
        raise SystemExit("no verdict: the pass completed %d pairs in configuration 'on' and %d in 'off' — the switch did not reach the library: %s" % (res["configs"]["on"]["fast"], res["configs"]["off"]["fast"], json.dumps(res)))
    ref = res["configs"].get("parent") or res["configs"]["off"]
    res["reference"] = "parent" if "parent" in res["configs"] else "off"
    res["reference_spread_ms"] = round(ref["max"] - ref["min"], 3)
    res["gain_ms"] = round(ref["median"] - res["configs"]["on"]["median"], 3)
    res["stays_on"] = res["gain_ms"] > res["reference_spread_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
