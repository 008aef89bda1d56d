"""Lanes and machine streams (h2g_kernels.hip): a run is lane gen % 8 — the parts of the overflow, long-edit and XL areas, the per-run buffers — and its machine
pass runs on HIP stream lane % S, where S (machine streams in rotation) follows the load.  Whatever S is and however it changes between queued runs, every
result is what a stream that only ever ran that batch returns."""
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
needs_build = pytest.mark.skipif(not os.path.exists(BUILD), reason="needs oracle/_ref/hisat2-build-s")

ALN_DT = np.dtype([("fw", "<u4"), ("tidx", "<u4"), ("toff", "<u4"), ("len", "<u4"), ("trim5", "<u4"), ("trim3", "<u4"), ("nedits", "<u4"), ("spl", "<u4"),
                   ("score", "<i8"), ("edits", [("pos", "<u4"), ("chr", "u1"), ("qchr", "u1"), ("type", "u1"), ("pad", "u1"), ("snp", "<u4")], 32)])


def _recs(arr, n):
    """n dense records with the edit entries a record does not use zeroed (they are whatever the row held before)"""
    a = np.frombuffer(arr, dtype=ALN_DT, count=n).copy()
    keep = np.arange(32)[None, :] < a["nedits"][:, None]
    for f in ("pos", "chr", "qchr", "type", "pad", "snp"):
        a["edits"][f][~keep] = 0
    return a.tobytes()


def _dense(st):
    res, a1, f1, a2, f2 = st.align_pairs_fetch_dense()
    return bytes(res), _recs(a1, int(f1[-1])), f1.tobytes(), _recs(a2, int(f2[-1])), f2.tobytes()


def _index(contigs, prefix):
    tmp = tempfile.mkdtemp(prefix=prefix)
    fa = os.path.join(tmp, "g.fa")
    synth.write_fasta(fa, contigs)
    base = os.path.join(tmp, "g")
    subprocess.run([BUILD, "-q", "-p", "16", fa, base], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return tmp, base


def _load(st, m1, m2, names):
    c1, o1 = synth.flatten_reads(m1); c2, o2 = synth.flatten_reads(m2)
    st.set_reads(c1, o1); st.set_read_names(names); st.set_mates(c2, o2, names)


def _params(st):
    p = st.align_params(); p.no_spliced_alignment = 1
    return p


def _alone(ix, m1, m2, names, tune=()):
    """the batch on a stream that only ever ran it: (dense results, counters)"""
    st = api.Stream(ix, max_reads=len(m1), max_bases=m1.size + 64)
    for k, v in tune:
        st.tune(k, v)
    _load(st, m1, m2, names)
    st.align_pairs_run(_params(st))
    out = _dense(st)
    c = st.counters()
    st.close()
    return out, c


# ---- 1. the same results for every S
@needs_build
@pytest.mark.parametrize("case", [
    dict(seed=75, npairs=120000, nreads=60000, rdlen=101, sub=0.005, repeat_genome=True),
    dict(seed=71, npairs=150000, nreads=150000, rdlen=101, sub=0.005),
])
def test_same_results_for_every_rotation(case):
    if case.get("repeat_genome"):
        contigs = synth.make_repeat_genome([5000000, 2000000, 1000000], case["seed"])
    else:
        contigs = synth.make_genome([1500000, 400000, 100000], case["seed"], n_gaps=3, gap_len=300, repeats=80, repeat_len=600)
    tmp, base = _index(contigs, "h2ms")
    m1, m2 = synth.make_pairs(contigs, case["npairs"], case["rdlen"], case["seed"] + 1, frag_mean=300, frag_sd=40, sub_rate=case["sub"])
    reads, _ = synth.make_reads(contigs, case["nreads"], case["rdlen"], case["seed"] + 2, sub_rate=case["sub"])
    npz = os.path.join(tmp, "reads.npz")
    np.savez(npz, m1=np.stack(m1), m2=np.stack(m2), reads=np.asarray(reads))
    arms = {"light1": {"H2G_MSTREAMS_LIGHT": "1"}, "light2": {"H2G_MSTREAMS_LIGHT": "2"}, "light3": {"H2G_MSTREAMS_LIGHT": "3"}, "pinned8": {"H2G_MSTREAMS": "8"}, "default": {}}
    got = {}
    for name, extra in arms.items():
        env = {k: v for k, v in os.environ.items() if k not in ("H2G_MSTREAMS", "H2G_MSTREAMS_LIGHT")}
        env.update(H2G_GO_FAST="1", H2G_FAST_ORPHAN="200", H2G_DRAIN_GRID="8", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"), **extra)   # (the drain launch forced)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fast_digest.py"), base, npz], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got[name] = json.loads(r.stdout.strip().splitlines()[-1])
    print(got)
    for k, total in (("pairs", case["npairs"]), ("reads", case["nreads"])):
        for name in arms:
            g = got[name][k]
            assert g["fast"] + g["handed_on"] == total, (name, k, g)
            assert g["fast"] + g["handed_on"] == got["pinned8"][k]["fast"] + got["pinned8"][k]["handed_on"]
            assert g["adopted"] > 0, (name, k, g)                                       # the drain launch ran
            assert g["aligned"] == got["pinned8"][k]["aligned"], (name, k)
            assert g["sha"] == got["pinned8"][k]["sha"], (name, k)


# ---- 2. the parts of the areas keep their rotation of eight when two machine streams are in rotation
@needs_build
def test_area_parts_rotate_by_eight_lanes_on_two_streams():
    """Three resident batches with pairs that exceed their fixed rows (pair_slots = 2: their records live in the stream's overflow area, one part per LANE; the drain launch
    forced as in test_gpu_fast_pass.py, so that a batch of this size hands on less than 1.5 % and the stream stays in the light regime).  Run A, then seven further
    runs over the other batches, then fetch A: its part must still hold its records — with parts rotating by machine stream (two) the third run would have overwritten them."""
    contigs = synth.make_repeat_genome([5000000, 2000000, 1000000], 75)      # (its pairs keep the fast pass's hand-ons below 1.5 %: the light regime)
    _, base = _index(contigs, "h2ml")
    n = 60000
    tune = (("pair_slots", 2), ("orphan", 200), ("drain_grid", 8))
    sets = []
    for k in range(3):
        m1, m2 = synth.make_pairs(contigs, n, 101, 516 + k, frag_mean=300, frag_sd=40, sub_rate=0.005)
        sets.append((np.stack(m1), np.stack(m2), ["p%d_%d" % (k, i) for i in range(n)]))
    ix = api.Index(base, device=0)
    want, cnt = zip(*[_alone(ix, m1, m2, names, tune=tune) for m1, m2, names in sets])
    f1 = np.frombuffer(want[0][2], dtype=np.uint64); f2 = np.frombuffer(want[0][4], dtype=np.uint64)
    beyond = int(((np.diff(f1) > 2) | (np.diff(f2) > 2)).sum())
    bails = [int(c.n_fast_bail) for c in cnt]
    print("pairs of batch A beyond two rows per mate:", beyond, "hand-ons per batch:", bails)
    assert beyond > 0, "the batch must use the overflow area"
    assert want[0] != want[1]
    assert all(b * 1000 <= n * 15 for b in bails), "the batches must stay in the light regime: " + str(bails)
    st = api.Stream(ix, max_reads=n, max_bases=max(m1.size for m1, _, _ in sets) + 64)
    for k, v in tune + (("mstreams_light", 2),):
        st.tune(k, v)
    for k, s_ in enumerate(sets):
        st.select_batch(k)
        _load(st, *s_)
    p = _params(st)
    st.select_batch(0); st.align_pairs_run(p)                          # run A: lane 0
    for k in (1, 2, 1, 2, 1, 2, 1):                                     # seven further runs: lanes 1 .. 7 (on two streams, passes in order on each)
        st.select_batch(k); st.align_pairs_run(p)
    assert st.probe("lanes") == 8 and st.probe("mstreams_rotation") == 2 and st.probe("mstreams_used") == 2
    st.select_batch(0)
    assert _dense(st) == want[0], "batch A after seven further runs"
    for k in (2, 1):
        st.select_batch(k)
        assert _dense(st) == want[k], "batch %d" % k
    st.close(); ix.close()


# ---- 3. the rotation changes while runs are queued
@needs_build
def test_rotation_follows_the_hand_on_load_in_flight():
    """A batch of which the fast pass hands on little and a batch of hard reads, alternated on one stream.  A run's plan sees the count the previous run's policy read, so with
    a sync after each of the first two runs those two are light (nothing was known when they were planned) and the fourth at the latest has seen the hard batch's count: all
    eight machine streams, created then and only then."""
    contigs = synth.make_genome([1500000, 400000, 100000], 71, n_gaps=3, gap_len=300, repeats=80, repeat_len=600)
    _, base = _index(contigs, "h2mr")
    n = 60000
    e1, e2 = synth.make_pairs(contigs, n, 101, 72, frag_mean=300, frag_sd=40, sub_rate=0.005)
    h1, h2 = synth.make_pairs(contigs, n, 76, 73, frag_mean=300, frag_sd=40, sub_rate=0.03)
    sets = [(np.stack(e1), np.stack(e2), ["e%d" % i for i in range(n)]), (np.stack(h1), np.stack(h2), ["h%d" % i for i in range(n)])]
    ix = api.Index(base, device=0)
    want, cnt = zip(*[_alone(ix, *s_) for s_ in sets])
    bails = [int(c.n_fast_bail) for c in cnt]
    print("hand-ons of", n, "pairs: easy", bails[0], "hard", bails[1])
    assert n * 15 < bails[1] * 1000 and bails[0] < bails[1], bails
    st = api.Stream(ix, max_reads=n, max_bases=max(s_[0].size for s_ in sets) + 64)
    for k, s_ in enumerate(sets):
        st.select_batch(k)
        _load(st, *s_)
    p = _params(st)
    seen = []
    for run in range(8):
        st.select_batch(run % 2); st.align_pairs_run(p)
        seen.append((st.probe("mstreams_rotation"), st.probe("mstreams_used")))
        if run < 2:
            st.sync()
    print(seen)
    assert seen[0] == (2, 2) and seen[1] == (2, 2)
    assert seen[2] in ((2, 2), (8, 8)) and seen[3] == (8, 8)
    assert all(c == 8 for _, c in seen[3:])                             # the stream count grew once
    for k in (1, 0):
        st.select_batch(k)
        assert _dense(st) == want[k], "batch %d" % k
    st.close(); ix.close()


# ---- 4. the machine streams' empty first launches next to a list that holds an earlier run's count
@needs_build
def test_warm_up_launches_beside_a_deferred_list():
    """Large batches (>= 200 000 pairs) on repeat-structured sequence: the first run defers reads to its second pass, so its overflow list holds a count when the
    second run's warm-up launches go out on the other machine streams (all eight pinned, the setting under which every stream is warmed)."""
    contigs = synth.make_repeat_genome([5000000, 2000000, 1000000], 75)
    _, base = _index(contigs, "h2mw")
    n = 200000
    sets = []
    for k in range(2):
        m1, m2 = synth.make_pairs(contigs, n, 101, 76 + k, frag_mean=300, frag_sd=40, sub_rate=0.005)
        sets.append((np.stack(m1), np.stack(m2), ["w%d_%d" % (k, i) for i in range(n)]))
    ix = api.Index(base, device=0)
    want, cnt = zip(*[_alone(ix, *s_) for s_ in sets])
    print("reads deferred to the second pass:", [int(c.n_second_pass) for c in cnt])
    assert int(cnt[0].n_second_pass) > 0, "the first batch must defer reads to its second pass"
    for pinned in (8, 0):
        st = api.Stream(ix, max_reads=n, max_bases=max(s_[0].size for s_ in sets) + 64)
        if pinned:
            st.tune("mstreams", pinned)
        for k, s_ in enumerate(sets):
            st.select_batch(k)
            _load(st, *s_)
        p = _params(st)
        st.select_batch(0); st.align_pairs_run(p)
        st.sync()
        assert int(st.counters().n_second_pass) > 0
        assert st.probe("mstreams_used") == (8 if pinned else 2) and st.probe("pools") == 2      # a caller with one batch pays for one stream's pools
        st.select_batch(1); st.align_pairs_run(p)
        created = st.probe("mstreams_used")
        assert st.probe("pools") == 2 * created
        for k in (0, 1):
            st.select_batch(k)
            assert _dense(st) == want[k], "pinned %d, batch %d" % (pinned, k)
        st.close()
    ix.close()
