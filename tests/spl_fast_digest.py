"""Digest of every result of go() over a batch in a SPLICED run, printed as one JSON line (tests/test_gpu_spl_fast.py runs it with the fast pass on and with
H2G_GO_FAST=0: the switch is read once per process).  fast_digest.py's three back-to-back runs and SHA-256, with spliced alignment on, every read independent
of the others (no_temp_splicesite = 1), optionally a splice-site file loaded into the index's database, and the number of records that hold a splice edit.
usage: spl_fast_digest.py index_base reads.npz [--sites file] [reference options, e.g. --dta]"""
import ctypes as C
import json
import sys

import numpy as np

from fast_digest import ALN_DT, flat_of, pairs_digest, reads_digest, run_counters
from hisat2_amd import api

EDIT_SPL = 5


def spliced_records(arr, n):
    a = np.frombuffer(arr, dtype=ALN_DT, count=n)
    keep = np.arange(32)[None, :] < a["nedits"][:, None]
    return int(((a["edits"]["type"] == EDIT_SPL) & keep).any(axis=1).sum())


def main():
    base, npz, rest = sys.argv[1], sys.argv[2], sys.argv[3:]
    sites = None
    if rest and rest[0] == "--sites":
        sites, rest = rest[1], rest[2:]
    d = np.load(npz)
    out = {}
    ix = api.Index(base, device=0)
    if sites:
        lst = [(0, int(t[1]), int(t[2]), t[3]) for t in (l.split() for l in open(sites)) if len(t) >= 4]      # (one contig: tests/spl_fast_cases.py)
        L = api.lib()
        L.h2g_index_set_splice_sites.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32]
        assert L.h2g_index_set_splice_sites(ix.h, api.splice_site_array(lst, True), len(lst), 0) == 0
    (c1, o1), (c2, o2), (rc, ro) = flat_of(d, "m1"), flat_of(d, "m2"), flat_of(d, "reads")
    n, nrd = len(o1) - 1, len(ro) - 1
    names = [str(i) for i in range(n)]
    st = api.Stream(ix, max_reads=max(n, nrd), max_bases=max(c1.size, c2.size, rc.size) + 64)
    st.set_reads(c1, o1); st.set_read_names(names); st.set_mates(c2, o2, names)
    p = st.align_params()
    assert not p.apply_options(list(rest))
    p.no_spliced_alignment = 0; p.no_temp_splicesite = 1
    for rep in range(3):                                         # back-to-back runs: the machine passes of earlier runs overlap the later fast passes
        st.align_pairs_run(p)
    sha, a1, n1, a2, n2 = pairs_digest(st, n)
    out["pairs"] = {"sha": sha, **run_counters(st), "spliced_records": spliced_records(a1, n1) + spliced_records(a2, n2)}
    st.set_reads(rc, ro); st.set_read_names([str(i) for i in range(nrd)])
    for rep in range(3):
        st.align_run(p)
    sha, aln, nrec = reads_digest(st, nrd)
    out["reads"] = {"sha": sha, **run_counters(st), "spliced_records": spliced_records(aln, nrec)}
    st.close(); ix.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
