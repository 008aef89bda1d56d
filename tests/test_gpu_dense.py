"""go() on the in-edge-rich graph gdense (tests/dense_cases.py): the 2000 reads and 1000 pairs of 101 bases from its alternate haplotype.
1. the fast pass on against off (tests/fast_digest.py, one process per digest): equal SHA-256 over every result and record, equal `aligned`;
2. the fast pass off against the reference binary's SAM (tests/golden/ref_gdense_{se,pe}.sam.gz), line by line;
3. with the pass on, reads leave it for the group walk's capacities (the by-reason counters of the last pass, read as bench.py's fast_bail_reasons reads them)."""
import ctypes as C
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import h2o_py as H
import parity_cases as PC
import sam_util as SU
from hisat2_amd import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FB_GWALK = 21               # h2g_fast.h: position of FB_GWALK among the hand-on reasons


@pytest.fixture(scope="module")
def dense(tmp_path_factory, golden_dir):
    d = tmp_path_factory.mktemp("gdense_go")
    base = PC.unpack_index(golden_dir, "gdense", d)
    sets = {t: H.read_fasta_reads(os.path.join(golden_dir, f"reads_gdense_{t}.fa.gz"))[1] for t in ("se", "pe_1", "pe_2")}
    npz = str(d / "reads.npz")
    np.savez(npz, m1=np.stack(sets["pe_1"]), m2=np.stack(sets["pe_2"]), reads=np.stack(sets["se"]))
    return base, sets, npz


def _digest(base, npz, fast):
    env = dict(os.environ, H2G_GO_FAST=fast, H2G_FAST_TAIL="0", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fast_digest.py"), base, npz], env=env, capture_output=True, text=True, timeout=300)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in r.stderr:
        pytest.exit("a digest process faulted (status %d): nothing more is started on this device\n%s" % (r.returncode, r.stderr[-2000:]), returncode=3)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_fast_pass_on_against_off(dense):
    base, sets, npz = dense
    off, on = _digest(base, npz, "0"), _digest(base, npz, "1")
    print("off", off, "on", on)
    for k, n in (("pairs", len(sets["pe_1"])), ("reads", len(sets["se"]))):
        assert off[k]["fast"] == 0 and on[k]["fast"] > 0 and on[k]["fast"] + on[k]["handed_on"] == n, (k, on[k])
        assert on[k]["sha"] == off[k]["sha"] and on[k]["aligned"] == off[k]["aligned"] and on[k]["overflow"] == off[k]["overflow"], (k, off[k], on[k])


def _stream(base, seqs, names, mates=None):
    codes = np.concatenate(seqs).astype(np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint32)
    ix = api.Index(base, device=0)
    st = api.Stream(ix, max_reads=len(seqs), max_bases=int(codes.size))
    st.set_reads(codes, offs)
    st.set_read_names(names)
    if mates is not None:
        st.set_mates(np.concatenate(mates).astype(np.uint8), offs, names)
    return ix, st


def _gwalk_hand_ons(st):
    v = (C.c_ulonglong * 136)()
    L = api.lib()
    L.h2g_go_fast_prof.argtypes = [C.c_void_p, C.c_void_p]
    assert L.h2g_go_fast_prof(st.h, v) == 0
    return int(v[48 + FB_GWALK])


def test_reads_equal_the_reference_and_leave_the_pass_for_the_group_walk(dense, golden_dir, monkeypatch):
    base, sets, _ = dense
    seqs = sets["se"]
    names = [str(i) for i in range(len(seqs))]
    refnames, want = SU.parse_sam(os.path.join(golden_dir, "ref_gdense_se.sam.gz"))
    refnames = refnames or ["chrD"]          # (the committed SAM is the body only)
    gw = {}
    for fast in ("0", "1"):
        monkeypatch.setenv("H2G_GO_FAST", fast)
        ix, st = _stream(base, seqs, names)
        p = st.align_params()
        p.no_spliced_alignment = 1
        st.align_run(p)
        res, aln = st.align_fetch()
        got = SU.render_selected(res, aln, refnames, seqs, names)
        if fast == "1":
            gw["reads"] = _gwalk_hand_ons(st)
        st.close(); ix.close()
        assert (res["overflow"] == 0).all()
        for q in names:
            assert got[q] == want[q], (fast, q)
    print("group-walk hand-ons", gw)
    assert gw["reads"] > 0


def test_pairs_equal_the_reference(dense, golden_dir, monkeypatch):
    import fuzz_pairs as F
    import pe_sink as PS
    base, sets, _ = dense
    s1, s2 = sets["pe_1"], sets["pe_2"]
    with tempfile.NamedTemporaryFile("w", suffix=".sam", delete=False) as t:
        t.write(gzip.open(os.path.join(golden_dir, "ref_gdense_pe.sam.gz"), "rt").read())
    refnames, want = F.parse_pe_sam(t.name)
    os.unlink(t.name)
    if not refnames:
        refnames = ["chrD"]
    q = [str(i) for i in range(len(s1))]
    monkeypatch.setenv("H2G_GO_FAST", "0")
    ix, st = _stream(base, s1, q, mates=s2)
    p = st.align_params()
    p.no_spliced_alignment = 1
    st.align_pairs_run(p)
    res, a1, a2 = st.align_pairs_fetch()
    st.close(); ix.close()
    for i in range(len(s1)):
        assert res[i].overflow == 0
        assert PS.finish_pair(res[i], a1, a2, i * api.PAIR_RES_CAP, refnames, (s1[i], s2[i])) == want[q[i]], i
