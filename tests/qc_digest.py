"""Digest of go() over a batch of pairs with --qc-filter bytes (h2g_set_read_filter), printed as one JSON line.  tests/test_gpu_readsets.py runs it with the
fast pass on and off (H2G_GO_FAST is read once per process).  usage: qc_digest.py index_base reads.npz"""
import hashlib
import json
import sys

import numpy as np

from fast_digest import aln_bytes
from hisat2_amd import api, synth


def main():
    base, npz = sys.argv[1], sys.argv[2]
    d = np.load(npz)
    m1, m2, p1, p2 = d["m1"], d["m2"], d["pass1"], d["pass2"]
    n = len(m1)
    ix = api.Index(base, device=0)
    c1, o1 = synth.flatten_reads(m1)
    c2, o2 = synth.flatten_reads(m2)
    names = [str(i) for i in range(n)]
    st = api.Stream(ix, max_reads=n, max_bases=max(c1.size, c2.size) + 64)
    p = st.align_params(); p.no_spliced_alignment = 1
    out = {}
    for tag in ("filtered", "cleared"):
        st.set_reads(c1, o1); st.set_read_names(names); st.set_mates(c2, o2, names)       # (set_reads clears the bytes of the run before)
        if tag == "filtered":
            st.set_read_filter(p1, p2)
        st.align_pairs_run(p)
        res, a1, f1, a2, f2 = st.align_pairs_fetch_dense()
        h = hashlib.sha256()
        h.update(bytes(res)); h.update(f1.tobytes()); h.update(f2.tobytes()); h.update(aln_bytes(a1, int(f1[n]))); h.update(aln_bytes(a2, int(f2[n])))
        c = st.counters()
        nres = np.array([[r.nres[0], r.nres[1], r.npairs] for r in res])
        out[tag] = {"sha": h.hexdigest(), "fast": int(c.n_fast), "handed_on": int(c.n_fast_bail), "overflow": int(c.n_overflow),
                    "filtered_with_alignment": int((nres[p1 == 0, 0] > 0).sum() + (nres[p2 == 0, 1] > 0).sum() + (nres[(p1 == 0) | (p2 == 0), 2] > 0).sum()),
                    "passing_mate_aligned": int((nres[(p1 == 0) & (p2 != 0), 1] > 0).sum() + (nres[(p2 == 0) & (p1 != 0), 0] > 0).sum()),
                    "aligned": int(((nres[:, 0] > 0) | (nres[:, 1] > 0)).sum())}
    st.close(); ix.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
