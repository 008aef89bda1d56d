"""Three resident batches of 5 000, 300 and 1 pairs on one stream, nine paired runs queued over them without a sync (tests/test_gpu_ps0.py runs it with
H2G_FAST_PS0=0 and =1: the record tables of the pre-pass rotate with the fast slot pools, and a small batch behind a large one shares pool 0 with it).
usage: ps0_batches.py index_base reads.npz    (m1, m2 as (n, L) arrays, n >= 5301) -> one JSON line: the digest of each batch after the last run"""
import json
import sys

import numpy as np

from hisat2_amd import api, synth
import fast_digest as FD

SIZES = (5000, 300, 1)


def main():
    base, npz = sys.argv[1], sys.argv[2]
    d = np.load(npz)
    m1, m2 = d["m1"], d["m2"]
    ix = api.Index(base, device=0)
    st = api.Stream(ix, max_reads=max(SIZES), max_bases=max(SIZES) * m1.shape[1] + 64)
    at = 0
    for k, n in enumerate(SIZES):
        st.select_batch(k)
        c1, o1 = synth.flatten_reads(m1[at:at + n]); c2, o2 = synth.flatten_reads(m2[at:at + n])
        names = [str(i) for i in range(n)]
        st.set_reads(c1, o1); st.set_read_names(names); st.set_mates(c2, o2, names)
        at += n
    p = st.align_params(); p.no_spliced_alignment = 1
    for rep in range(3):
        for k in range(len(SIZES)):
            st.select_batch(k)
            st.align_pairs_run(p)
    st.sync()
    out = {"sha": [], "aligned": []}
    for k, n in enumerate(SIZES):
        st.select_batch(k)
        sha, a1, n1, a2, n2 = FD.pairs_digest(st, n)
        out["sha"].append(sha); out["aligned"].append(n1 + n2)
    st.close(); ix.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
