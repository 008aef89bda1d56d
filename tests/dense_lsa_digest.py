"""Digests of go() over a batch around the moment the dense table of local rows becomes usable, one JSON line (tests/test_gpu_dense_lsa.py; H2G_DENSE_LSA is
read when the index is loaded).  Runs are queued straight after the load — on whichever side of the switch each falls, and a drain launch may adopt a slot
that a fast launch without the table stored in the middle of a walk — fetched, then the build is waited for (h2g_stream_sync, h2g_index_dense_lsa_check)
and the runs are repeated.  usage: dense_lsa_digest.py index_base reads.npz"""
import json
import sys

import numpy as np

from hisat2_amd import api, synth
from fast_digest import pairs_digest, run_counters


def main():
    base, npz = sys.argv[1], sys.argv[2]
    d = np.load(npz)
    m1, m2 = d["m1"], d["m2"]
    n = len(m1)
    c1, o1 = synth.flatten_reads(m1)
    c2, o2 = synth.flatten_reads(m2)
    names = [str(i) for i in range(n)]
    ix = api.Index(base, device=0)
    st = api.Stream(ix, max_reads=n, max_bases=c1.size + 64)
    st.set_reads(c1, o1); st.set_read_names(names); st.set_mates(c2, o2, names)
    p = st.align_params(); p.no_spliced_alignment = 1
    out = {"sha": [], "fast": [], "aligned": [], "device_bytes": int(ix.info.device_bytes), "len": int(ix.info.len), "nLocal": int(ix.info.nLocal)}

    def fetch():
        out["sha"].append(pairs_digest(st, n)[0])
        c = run_counters(st)
        out["fast"].append(c["fast"]); out["aligned"].append(c["aligned"])

    for rep in range(4):                                          # each run fetched on its own: any of them may be the first with the table
        st.align_pairs_run(p)
        fetch()
    st.sync()
    out["table"], _ = ix.dense_lsa()
    out["sa_table"], _ = ix.dense_sa()
    for rep in range(2):
        st.align_pairs_run(p)
    fetch()
    st.close(); ix.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
