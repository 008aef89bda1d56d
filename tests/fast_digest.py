"""Digest of every result of go() over a batch, printed as one JSON line (tests/test_gpu_fast_pass.py runs it twice: the fast pass on / off,
H2G_GO_FAST is read once per process).  usage: fast_digest.py index_base reads.npz [alignment options of the reference ...]
The npz holds m1, m2, reads as (n, L) arrays, or — a ragged batch — each as flat codes plus offsets: m1_codes / m1_offs, m2_codes / m2_offs, reads_codes / reads_offs;
and, for FASTQ input, m1_quals / m2_quals / reads_quals: flat phred+33 bytes over the same offsets.  The trailing options (tests/option_cases.py) are applied to the run's
block with AlignParams.apply_options.  Without options and qualities the output is what it always was.

A record beyond 32 edits keeps its list in the stream's long-edit area and the area's offset in edits[0].pos; where a record lands in the area follows the timing of the
passes.  Such a record is hashed with its slots zeroed and its list — fetched through align_fetch_long_edits — behind the records; with options or qualities given, the
number of such records is reported as "long_edits"."""
import hashlib
import json
import sys

import numpy as np

from hisat2_amd import api, synth

ALN_DT = np.dtype([("fw", "<u4"), ("tidx", "<u4"), ("toff", "<u4"), ("len", "<u4"), ("trim5", "<u4"), ("trim3", "<u4"), ("nedits", "<u4"), ("spl", "<u4"),
                   ("score", "<i8"), ("edits", [("pos", "<u4"), ("chr", "u1"), ("qchr", "u1"), ("type", "u1"), ("pad", "u1"), ("snp", "<u4")], 32)])


EDIT_BYTES = 12


def aln_bytes(arr, n, st=None, count=None):
    """st: the stream the records came from (without it a long record is hashed as its slots stand, as it always was); count: a one-element list that receives the
    number of records beyond 32 edits"""
    a = np.frombuffer(arr, dtype=ALN_DT, count=n).copy()
    long_ = (a["nedits"] > 32) & (st is not None)
    at = a["edits"]["pos"][:, 0].copy()
    keep = (np.arange(32)[None, :] < a["nedits"][:, None]) & ~long_[:, None]
    for f in ("pos", "chr", "qchr", "type", "pad", "snp"):      # edit slots past nedits are not part of a record
        a["edits"][f][~keep] = 0
    if count is not None:
        count[0] += int(long_.sum())
    if not long_.any():
        return a.tobytes()
    led, used = st.align_fetch_long_edits()
    buf = bytes(led)
    lists = []
    for k in np.nonzero(long_)[0]:
        off, ne = int(at[k]), int(a["nedits"][k])
        assert off + ne <= used, (off, ne, used)
        lists.append(buf[off * EDIT_BYTES:(off + ne) * EDIT_BYTES])
    return a.tobytes() + b"".join(lists)


def pairs_digest(st, n, long_edits=None):
    """the paired run's dense results of st's n pairs -> (SHA-256 of headers, both offset arrays, both record arrays; mate-1 records, their number, mate-2
    records, their number).  long_edits: a one-element list — records beyond 32 edits are hashed with their lists fetched from the stream, and their number is
    added to it (aln_bytes); None: as their slots stand"""
    res, a1, f1, a2, f2 = st.align_pairs_fetch_dense()
    n1, n2 = int(f1[n]), int(f2[n])
    lst = st if long_edits is not None else None
    h = hashlib.sha256()
    h.update(bytes(res)); h.update(f1.tobytes()); h.update(f2.tobytes()); h.update(aln_bytes(a1, n1, lst, long_edits)); h.update(aln_bytes(a2, n2, lst, long_edits))
    return h.hexdigest(), a1, n1, a2, n2


def reads_digest(st, n, long_edits=None):
    """the unpaired run's dense results of st's n reads -> (SHA-256 of headers, offsets, records; the records, their number); long_edits as pairs_digest's"""
    res, aln, offs = st.align_fetch_dense()
    nrec = int(offs[n])
    h = hashlib.sha256()
    h.update(res.tobytes()); h.update(offs.tobytes()); h.update(aln_bytes(aln, nrec, st if long_edits is not None else None, long_edits))
    return h.hexdigest(), aln, nrec


def run_counters(st):
    c = st.counters()
    return {"fast": int(c.n_fast), "handed_on": int(c.n_fast_bail), "aligned": int(c.n_aligned), "overflow": int(c.n_overflow), "adopted": int(c.n_adopted)}


def flat_of(d, key):
    """(codes, offsets) of read set `key` of the npz, stacked or flat"""
    if key in d.files:
        return synth.flatten_reads(d[key])
    return np.ascontiguousarray(d[key + "_codes"], dtype=np.uint8), np.ascontiguousarray(d[key + "_offs"], dtype=np.uint32)


def save_ragged(path, m1, m2, reads):
    """the npz of a ragged batch: lists of read arrays of any lengths"""
    def flat(lst):
        return np.concatenate([np.asarray(r, dtype=np.uint8) for r in lst]), np.concatenate([[0], np.cumsum([len(r) for r in lst])]).astype(np.uint32)
    kw = {}
    for key, lst in (("m1", m1), ("m2", m2), ("reads", reads)):
        kw[key + "_codes"], kw[key + "_offs"] = flat(lst)
    np.savez(path, **kw)


def main():
    base, npz, opts = sys.argv[1], sys.argv[2], sys.argv[3:]
    d = np.load(npz)
    quals = {k: np.ascontiguousarray(d[k + "_quals"], dtype=np.uint8) if k + "_quals" in d.files else None for k in ("m1", "m2", "reads")}
    extended = bool(opts) or any(q is not None for q in quals.values())
    out = {}
    ix = api.Index(base, device=0)
    (c1, o1), (c2, o2), (rc, ro) = flat_of(d, "m1"), flat_of(d, "m2"), flat_of(d, "reads")
    n, nrd = len(o1) - 1, len(ro) - 1
    names = [str(i) for i in range(n)]
    st = api.Stream(ix, max_reads=max(n, nrd), max_bases=max(c1.size, c2.size, rc.size) + 64)
    st.set_reads(c1, o1, quals["m1"]); st.set_read_names(names); st.set_mates(c2, o2, names, quals["m2"])
    p = st.align_params(); p.no_spliced_alignment = 1
    rest = p.apply_options(opts)
    assert not rest, rest
    for rep in range(3):                                         # back-to-back runs: the machine passes of earlier runs overlap the later fast passes
        st.align_pairs_run(p)
    nlong = [0]
    out["pairs"] = {"sha": pairs_digest(st, n, nlong)[0], **run_counters(st)}
    if extended:
        out["pairs"]["long_edits"] = nlong[0]
    st.set_reads(rc, ro, quals["reads"]); st.set_read_names([str(i) for i in range(nrd)])
    for rep in range(3):
        st.align_run(p)
    nlong = [0]
    out["reads"] = {"sha": reads_digest(st, nrd, nlong)[0], **run_counters(st)}
    if extended:
        out["reads"]["long_edits"] = nlong[0]
    st.close(); ix.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
