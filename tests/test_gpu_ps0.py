"""The fast pass's first partial searches in a pre-pass kernel (hisat2_amd/csrc/h2g_k_ps0.hip; H2G_FAST_PS0 / h2g_stream_tune "ps0"): go() gives the same
bytes — tests/fast_digest.py's SHA-256 covers every record and the per-read work counters — with the pre-pass (1) and without it (0, the code path of
before) on a 2 Mbp linear index built by the reference builder.

As in tests/test_gpu_dense_sa.py, how many reads the pass completes itself and how many it hands on is compared exactly with the tail policy of paired
batches off (H2G_FAST_TAIL=0); under the default policy that split follows the timing of the launch, and sha, aligned and fast + handed_on are compared."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from hisat2_amd import synth
import fast_digest as FD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "oracle", "_ref", "hisat2-build-s")
needs_builder = pytest.mark.skipif(not os.path.exists(BUILD), reason="needs oracle/_ref/hisat2-build-s")
FTAB = 10                                # ftabChars of an index of this size (asserted below)
PK_MAXLEN = 128                          # H2G_PK_MAXLEN


@pytest.fixture(scope="module")
def staged():
    """the 2 Mbp index of test_gpu_dense_sa.py::_stage, 20 000 pairs + 20 000 reads of 101 bp, and the ragged batch"""
    tmp = tempfile.mkdtemp(prefix="h2ps0")
    contigs = synth.make_genome([1500000, 400000, 100000], 71, n_gaps=3, gap_len=300, repeats=80, repeat_len=600)
    fa = os.path.join(tmp, "g.fa")
    synth.write_fasta(fa, contigs)
    base = os.path.join(tmp, "g")
    subprocess.run([BUILD, "-q", "-p", "16", fa, base], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    m1, m2 = synth.make_pairs(contigs, 20000, 101, 72, frag_mean=300, frag_sd=40, sub_rate=0.005)
    reads, _ = synth.make_reads(contigs, 20000, 101, 73, sub_rate=0.005)
    npz = os.path.join(tmp, "reads.npz")
    np.savez(npz, m1=np.stack(m1), m2=np.stack(m2), reads=np.asarray(reads))
    # the ragged batch: pairs and reads of 129 bases cut to the edge lengths, unequal and empty mates, Ns inside and beyond the first ftabChars bases of
    # either strand's search; 1 003 pairs and 1 001 reads (no multiple of 64)
    lens = [0, 1, FTAB, FTAB + 1, FTAB + 2, 30, 101, PK_MAXLEN, PK_MAXLEN + 1]
    l1, l2 = synth.make_pairs(contigs, 1003, PK_MAXLEN + 1, 74, frag_mean=320, frag_sd=40, sub_rate=0.005)
    lr, _ = synth.make_reads(contigs, 1001, PK_MAXLEN + 1, 75, sub_rate=0.005)
    rng = np.random.default_rng(76)

    def cut(r, i, shift):
        r = np.array(r[:lens[(i // 3 + shift) % len(lens)] if i % 3 else 101], dtype=np.uint8)      # a third at 101: most of the batch stays in the pass
        if i % 7 == 0 and len(r) > 2 * FTAB + 12:
            r[[3, len(r) - 4, len(r) // 2, FTAB + 5][int(rng.integers(4))]] = 4
        return r
    rm1 = [cut(r, i, 0) for i, r in enumerate(l1)]
    rm2 = [cut(r, i, 4) for i, r in enumerate(l2)]                                              # unequal mates; an empty mate on either side
    rr = [cut(r, i, 0) for i, r in enumerate(lr)]
    assert any(len(a) == 0 and len(b) > 0 for a, b in zip(rm1, rm2)) and any(len(b) == 0 and len(a) > 0 for a, b in zip(rm1, rm2))
    ragged = os.path.join(tmp, "ragged.npz")
    FD.save_ragged(ragged, rm1, rm2, rr)
    return base, npz, ragged


def _run(script, base, npz, ps0, opts=(), **knobs):
    env = dict(os.environ, H2G_FAST_PS0=ps0, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"), **knobs)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", script), base, npz, *opts], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _same_with_and_without(base, npz, opts=(), **knobs):
    got = {m: _run("fast_digest.py", base, npz, m, opts, **knobs) for m in ("0", "1")}
    print(got)
    for k in ("pairs", "reads"):
        for f in ("sha", "aligned"):
            assert got["0"][k][f] == got["1"][k][f], (k, f)
        assert got["0"][k]["fast"] + got["0"][k]["handed_on"] == got["1"][k]["fast"] + got["1"][k]["handed_on"] and got["1"][k]["fast"] > 0
    exact = {m: _run("fast_digest.py", base, npz, m, opts, H2G_FAST_TAIL="0", **knobs) for m in ("0", "1")}
    print(exact)
    for k in ("pairs", "reads"):
        for f in ("sha", "fast", "handed_on", "aligned"):
            assert exact["0"][k][f] == exact["1"][k][f], (k, f)
    return got, exact


@needs_builder
def test_pairs_and_reads(staged):
    base, npz, _ = staged
    got, _ = _same_with_and_without(base, npz)
    assert got["1"]["pairs"]["aligned"] > 15000 and got["1"]["reads"]["aligned"] > 15000


@needs_builder
def test_ragged_batch(staged):
    base, _, ragged = staged
    from hisat2_amd import api
    ix = api.Index(base, device=0)
    assert ix.info.ftabChars == FTAB
    ix.close()
    _same_with_and_without(base, ragged)


@needs_builder
def test_drain_launch_reads_the_table(staged):
    """an adopted read that still has fresh strands takes its first searches from the table in the drain launch"""
    base, npz, _ = staged
    got, exact = _same_with_and_without(base, npz, H2G_FAST_ORPHAN="64", H2G_DRAIN_GRID="4")
    for r in (got, exact):
        assert r["1"]["pairs"]["adopted"] > 0 and r["0"]["pairs"]["adopted"] > 0


@needs_builder
@pytest.mark.parametrize("opts", [("--no-anchorstop",), ("-k", "1")])
def test_options_the_search_depends_on(staged, opts):
    base, npz, _ = staged
    _same_with_and_without(base, npz, opts)


@needs_builder
def test_batches_and_pools(staged):
    """three resident batches of 5 000, 300 and 1 pairs, nine runs queued without a sync: every batch's digest is the one it has with the pre-pass off"""
    base, npz, _ = staged
    got = {m: _run("ps0_batches.py", base, npz, m) for m in ("0", "1")}
    print(got)
    assert got["0"] == got["1"]
    assert len(set(got["1"]["sha"])) == 3 and got["1"]["aligned"][0] > 4000
