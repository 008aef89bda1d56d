"""The dense SA table on the device (H2G_DENSE_SA, include/h2g.h): the table k_sa_dense_build writes equals the canonical walk for every row of an
8 Mbp linear index; go() gives byte-identical results — work counters included — with the table (modes 1 and 2) and without it (mode 0), whichever
side of the end of the build a run is queued on; h2g_sa_resolve and the seed stage stay pinned to the goldens and the oracle with the table in use.

How many pairs the fast pass completes itself and how many it hands on is compared exactly with the tail policy of paired batches off (H2G_FAST_TAIL=0): under the default
policy that split follows the timing of the launch and differs between two processes of the same mode (measured: 140 632 / 140 663 pairs completed in two runs without the
table, 140 584 / 140 609 in two runs with it, SHA-256 and `aligned` equal throughout; 143 613 in all four with the policy off — profiles/r07_dense_sa.md §8)."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import h2o_py as H
import parity_cases as PC
from hisat2_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "oracle", "_ref", "hisat2-build-s")
needs_builder = pytest.mark.skipif(not os.path.exists(BUILD), reason="needs oracle/_ref/hisat2-build-s")

# the batches of tests/test_gpu_fast_pass.py: its first two cases and its repeat-genome case
CASES = [
    dict(seed=71, npairs=150000, nreads=150000, rdlen=101, sub=0.005),
    dict(seed=72, npairs=60000, nreads=60000, rdlen=76, sub=0.03, indel=0.002, nrate=0.002),
    dict(seed=75, npairs=120000, nreads=60000, rdlen=101, sub=0.005, repeat_genome=True),
]


def _stage(case):
    tmp = tempfile.mkdtemp(prefix="h2dsa")
    if case.get("repeat_genome"):
        contigs = synth.make_repeat_genome([5000000, 2000000, 1000000], case["seed"])
    else:
        contigs = synth.make_genome([1500000, 400000, 100000], case["seed"], n_gaps=3, gap_len=300, repeats=80, repeat_len=600)
    fa = os.path.join(tmp, "g.fa")
    synth.write_fasta(fa, contigs)
    base = os.path.join(tmp, "g")
    subprocess.run([BUILD, "-q", "-p", "16", fa, base], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    m1, m2 = synth.make_pairs(contigs, case["npairs"], case["rdlen"], case["seed"] + 1, frag_mean=300, frag_sd=40, sub_rate=case["sub"])
    reads, _ = synth.make_reads(contigs, case["nreads"], case["rdlen"], case["seed"] + 2, sub_rate=case["sub"], indel_rate=case.get("indel", 0.0), n_rate=case.get("nrate", 0.0))
    npz = os.path.join(tmp, "reads.npz")
    np.savez(npz, m1=np.stack(m1), m2=np.stack(m2), reads=np.asarray(reads))
    return base, npz


def _run(script, base, npz, mode, **knobs):
    env = dict(os.environ, H2G_DENSE_SA=mode, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"), **knobs)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", script), base, npz], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@needs_builder
@pytest.mark.parametrize("case", CASES)
def test_results_are_the_same_with_and_without_the_table(case):
    base, npz = _stage(case)
    got = {m: _run("fast_digest.py", base, npz, m) for m in ("0", "2")}
    print(got)
    for k in ("pairs", "reads"):
        for f in ("sha", "aligned"):
            assert got["0"][k][f] == got["2"][k][f], (k, f)
        assert got["0"][k]["fast"] + got["0"][k]["handed_on"] == got["2"][k]["fast"] + got["2"][k]["handed_on"] and got["2"][k]["fast"] > 0
    # Which reads the fast pass completes and which it hands on is decided by the table or the walk for no read — but with the tail policy of paired
    # batches (FastArgs::tail: a workgroup hands on the reads it still holds when the batch runs out) that split follows the timing of the launch and
    # differs from process to process without any change.  It is a property of the code with the policy off, and there it has to be equal exactly.
    got = {m: _run("fast_digest.py", base, npz, m, H2G_FAST_TAIL="0") for m in ("0", "2")}
    print(got)
    for k in ("pairs", "reads"):
        for f in ("sha", "fast", "handed_on", "aligned"):
            assert got["0"][k][f] == got["2"][k][f], (k, f)
    if case.get("repeat_genome"):
        # mode 1: runs queued straight after the load and runs queued after the build, each against mode 0's
        m0, m1 = _run("dense_sa_digest.py", base, npz, "0"), _run("dense_sa_digest.py", base, npz, "1")
        print(m0, m1)
        assert not m0["table"] and m1["table"]
        assert len(set(m0["sha"])) == 1 and m1["sha"] == m0["sha"] and m1["aligned"] == m0["aligned"]
        assert m0["device_bytes_after"] == m0["device_bytes"]
        assert m1["device_bytes_after"] - m0["device_bytes"] >= 5 * 8000000           # h2g_index_info.device_bytes counts the table


@needs_builder
def test_device_built_table_equals_the_walk_on_every_row(monkeypatch):
    contigs = synth.make_repeat_genome([5000000, 2000000, 1000000], 75)
    tmp = tempfile.mkdtemp(prefix="h2dsa")
    fa = os.path.join(tmp, "g.fa")
    synth.write_fasta(fa, contigs)
    base = os.path.join(tmp, "g")
    subprocess.run([BUILD, "-q", "-p", "16", fa, base], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    for mode in ("2", "1"):
        monkeypatch.setenv("H2G_DENSE_SA", mode)
        ix = api.Index(base, device=0)
        assert ix.info.linear and ix.info.len >= 5000000
        has, differ = ix.dense_sa(verify=True)
        assert has and differ == 0, (mode, has, differ)
        ix.close()
    monkeypatch.setenv("H2G_DENSE_SA", "0")
    ix = api.Index(base, device=0)
    assert ix.dense_sa(verify=True) == (False, 0)
    ix.close()


def test_graph_index_has_no_table(g1s_index, monkeypatch):
    monkeypatch.setenv("H2G_DENSE_SA", "2")
    ix = api.Index(g1s_index, device=0)
    assert ix.dense_sa() == (False, None)
    ix.close()


@pytest.fixture()
def gpu2(g1_index, golden_dir, monkeypatch):
    monkeypatch.setenv("H2G_DENSE_SA", "2")
    ix = api.Index(g1_index, device=0)
    assert ix.dense_sa(verify=True) == (True, 0)
    reads, offs = PC.load_reads(golden_dir)
    st = api.Stream(ix, max_reads=200000, max_bases=200000 * 101)
    st.set_reads(reads.reshape(-1), offs)
    yield st
    st.close()
    ix.close()


def test_coords_golden_through_the_table(gpu2, golden_dir):
    assert PC.check_coords(gpu2, golden_dir) > 300


def test_sa_resolve_steps_equal_the_walk(gpu2, g1_index, monkeypatch):
    """h2g_sa_resolve over seeded row ranges: coordinates and nsteps with the table == without it"""
    rng = np.random.default_rng(3)
    n = gpu2.ix.info.gbwtLen
    tops = rng.integers(0, n - 8, size=20000)
    qs = [api.SaQuery(int(t), int(t) + int(w), int(w), 20, 0) for t, w in zip(tops, rng.integers(1, 6, size=len(tops)))]
    co2, res2 = gpu2.sa_resolve(qs, cap=8)
    monkeypatch.setenv("H2G_DENSE_SA", "0")
    ix0 = api.Index(g1_index, device=0)
    st0 = api.Stream(ix0, max_reads=1000, max_bases=101000)
    co0, res0 = st0.sa_resolve(qs, cap=8)
    assert bytes(co0) == bytes(co2) and bytes(res0) == bytes(res2)
    assert sum(r.nsteps for r in res2) > 10 * len(qs)
    st0.close(); ix0.close()


def test_seed_stage_vs_oracle_through_the_table(gpu2, oracle_lib, g1_index, golden_dir):
    contigs = PC.load_contigs(golden_dir)
    reads, _ = synth.make_reads(contigs, 3000, 101, 78, sub_rate=0.02, indel_rate=0.001, n_rate=0.002)
    codes, offs = synth.flatten_reads(reads)
    gpu2.set_reads(codes, offs)
    oix = H.load_index(oracle_lib, g1_index)
    for nospl in (True, False):
        p = gpu2.seed_params(no_spliced=nospl)
        gpu2.seed_extend_run(p)
        got = gpu2.seed_extend_fetch()
        want = PC.oracle_seed_extend(oracle_lib, oix, reads, p.pseudogeneStop)
        PC.assert_seed_equal(got, want)
    assert gpu2.counters().n_sa_steps == int(got["nsteps"].sum()) > 0
