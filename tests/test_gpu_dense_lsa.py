"""The dense table of local rows on the device (H2G_DENSE_LSA, include/h2g.h): the table k_lsa_dense_build writes equals the canonical walk for every row
of every local index of an 8 Mbp linear index; go() gives byte-identical results — work counters included — with the table and without it, with the
global table beside it or alone, and whichever side of the end of the build a run is queued on (a drain launch may then adopt a slot that a fast launch
without the table stored in the middle of a local walk).

As in test_gpu_dense_sa.py, how many pairs the fast pass completes itself is compared exactly only with the tail policy of paired batches off
(H2G_FAST_TAIL=0): under the default policy that split follows the timing of the launch."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from hisat2_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "oracle", "_ref", "hisat2-build-s")
needs_builder = pytest.mark.skipif(not os.path.exists(BUILD), reason="needs oracle/_ref/hisat2-build-s")


def _build(contigs, prefix):
    tmp = tempfile.mkdtemp(prefix=prefix)
    fa = os.path.join(tmp, "g.fa")
    synth.write_fasta(fa, contigs)
    base = os.path.join(tmp, "g")
    subprocess.run([BUILD, "-q", "-p", "16", fa, base], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return tmp, base


@pytest.fixture(scope="module")
def repeat8():
    """the 8 Mbp repeat-structured index of test_gpu_dense_sa.py (same builder call), with 30 000 pairs over it"""
    contigs = synth.make_repeat_genome([5000000, 2000000, 1000000], 75)
    tmp, base = _build(contigs, "h2lsa8")
    m1, m2 = synth.make_pairs(contigs, 30000, 101, 76, frag_mean=300, frag_sd=40, sub_rate=0.005)
    npz = os.path.join(tmp, "reads.npz")
    np.savez(npz, m1=np.stack(m1), m2=np.stack(m2))
    return base, npz


@pytest.fixture(scope="module")
def small2():
    """2 Mbp in three contigs with N gaps, 30 000 pairs and 30 000 single reads"""
    contigs = synth.make_genome([1500000, 400000, 100000], 81, n_gaps=3, gap_len=300, repeats=80, repeat_len=600)
    tmp, base = _build(contigs, "h2lsa2")
    m1, m2 = synth.make_pairs(contigs, 30000, 101, 82, frag_mean=300, frag_sd=40, sub_rate=0.005)
    reads, _ = synth.make_reads(contigs, 30000, 101, 83, sub_rate=0.01, indel_rate=0.001, n_rate=0.001)
    npz = os.path.join(tmp, "reads.npz")
    np.savez(npz, m1=np.stack(m1), m2=np.stack(m2), reads=np.asarray(reads))
    return base, npz


def _run(script, base, npz, lsa, **knobs):
    env = dict(os.environ, H2G_DENSE_LSA=lsa, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"), **knobs)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", script), base, npz], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@needs_builder
def test_device_built_table_equals_the_walk_on_every_local_row(repeat8, monkeypatch):
    base, _ = repeat8
    monkeypatch.delenv("H2G_DENSE_SA", raising=False)
    for mode in ("2", "1"):
        monkeypatch.setenv("H2G_DENSE_LSA", mode)
        ix = api.Index(base, device=0)
        assert ix.info.linear and ix.info.len >= 5000000 and ix.info.nLocal > 100
        has, differ = ix.dense_lsa(verify=True)
        assert has and differ == 0, (mode, has, differ)
        ix.close()
    monkeypatch.setenv("H2G_DENSE_LSA", "0")
    ix = api.Index(base, device=0)
    assert ix.dense_lsa(verify=True) == (False, 0)
    assert ix.dense_sa()[0]                                    # (the global table does not follow H2G_DENSE_LSA)
    ix.close()


def test_unset_follows_the_global_knob(g1_index, monkeypatch):
    monkeypatch.delenv("H2G_DENSE_LSA", raising=False)
    for sa, want in (("0", False), ("2", True)):
        monkeypatch.setenv("H2G_DENSE_SA", sa)
        ix = api.Index(g1_index, device=0)
        assert ix.dense_lsa(verify=True) == (want, 0)
        ix.close()


def test_graph_index_has_no_table(g1s_index, monkeypatch):
    monkeypatch.setenv("H2G_DENSE_LSA", "2")
    ix = api.Index(g1s_index, device=0)
    assert ix.dense_lsa() == (False, None)
    ix.close()


def _same(a, b, fields):
    for k in ("pairs", "reads"):
        for f in fields:
            assert a[k][f] == b[k][f], (k, f, a[k], b[k])
        assert a[k]["fast"] + a[k]["handed_on"] == b[k]["fast"] + b[k]["handed_on"] and b[k]["fast"] > 0


@needs_builder
def test_results_are_the_same_with_and_without_the_table(small2):
    base, npz = small2
    got = {m: _run("fast_digest.py", base, npz, m) for m in ("0", "2")}
    print(got)
    _same(got["0"], got["2"], ("sha", "aligned"))
    # with the tail policy of paired batches off, which reads the fast pass completes is a property of the code: equal exactly
    got = {m: _run("fast_digest.py", base, npz, m, H2G_FAST_TAIL="0") for m in ("0", "2")}
    print(got)
    _same(got["0"], got["2"], ("sha", "fast", "handed_on", "aligned"))


@needs_builder
def test_results_are_the_same_with_the_local_table_alone(small2):
    base, npz = small2
    got = {m: _run("fast_digest.py", base, npz, m, H2G_DENSE_SA="0", H2G_FAST_TAIL="0") for m in ("0", "2")}
    print(got)
    _same(got["0"], got["2"], ("sha", "fast", "handed_on", "aligned"))


@needs_builder
def test_runs_around_the_end_of_the_build_and_bytes_counted(repeat8):
    """mode 1: runs queued straight after the load and runs queued after the build, each against mode 0's"""
    base, npz = repeat8
    m0, m1 = _run("dense_lsa_digest.py", base, npz, "0"), _run("dense_lsa_digest.py", base, npz, "1")
    print(m0, m1)
    assert not m0["table"] and m1["table"] and m0["sa_table"] and m1["sa_table"]
    assert len(set(m0["sha"])) == 1 and m1["sha"] == m0["sha"] and m1["aligned"] == m0["aligned"]
    # h2g_index_info.device_bytes counts the table: 4 bytes per local row.  Every base lies in at least one local index and an index of n bases has n + 1
    # rows, so there are at least len + nLocal rows.
    assert m1["device_bytes"] - m0["device_bytes"] >= 4 * (m0["len"] + m0["nLocal"])
