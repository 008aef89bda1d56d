"""GPU: the lifetime of what a stream and an index own (csrc/h2g_dev.h: every device buffer, event and HIP stream is a handle).  Streams created, used and freed over and
over on one index; a stream freed with work queued; buffers that grow in place (names, mates' names, result rows, the extra-large unit's pools); an index loaded and freed
twice, its splice-site buffers replaced in place.  64 golden pairs (max_reads 64): the smallest batch that still allocates every pool.  The failure paths (an allocation
that fails half way through a context) need no device: tests/test_dev_handles_cpu.py."""
import os

import numpy as np
import pytest

import h2o_py as H
from hisat2_amd import api, synth

pytestmark = pytest.mark.gpu
N = 64


@pytest.fixture(scope="module")
def sets(golden_dir):
    """two batches of N pairs: (mate 1, mate 2, names)"""
    _, s1 = H.read_fasta_reads(os.path.join(golden_dir, "reads_pe_1.fa.gz"))
    _, s2 = H.read_fasta_reads(os.path.join(golden_dir, "reads_pe_2.fa.gz"))
    assert len(s1) >= 2 * N and max(len(r) for r in s1[:2 * N] + s2[:2 * N]) <= 101
    return [(np.stack(s1[k * N:(k + 1) * N]), np.stack(s2[k * N:(k + 1) * N]), ["lifecycle_batch%d_pair_%03d" % (k, i) for i in range(N)]) for k in range(2)]


def _stream(ix, sets):
    return api.Stream(ix, max_reads=N, max_bases=max(m1.size for m1, _, _ in sets) + 64)


def _fill(st, k, one):
    m1, m2, names = one
    st.select_batch(k)
    c1, o1 = synth.flatten_reads(m1); c2, o2 = synth.flatten_reads(m2)
    st.set_reads(c1, o1); st.set_mates(c2, o2, names); st.set_read_names(names)


def _compact(st):
    res, r1, o1, r2, o2 = st.align_pairs_fetch_compact()
    return res.tobytes(), r1[:int(o1[-1])].tobytes(), o1.tobytes(), r2[:int(o2[-1])].tobytes(), o2.tobytes()


def _cycle(ix, sets):
    """a stream's whole life: both batches filled and run, fetched compactly, the stream freed"""
    st = _stream(ix, sets)
    _fill(st, 0, sets[0]); st.align_pairs_run()
    _fill(st, 1, sets[1]); st.align_pairs_run()
    out = []
    for k in (0, 1):
        st.select_batch(k)
        out.append(_compact(st))
    st.close()
    return out


@pytest.fixture(scope="module")
def index(g1_index):
    ix = api.Index(g1_index, device=0)
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def first(index, sets):
    """the first cycle's bytes: what every later stream on the index must return"""
    out = _cycle(index, sets)
    assert out[0] != out[1] and len(out[0][1]) > N * 40      # (two different batches, and most pairs aligned)
    return out


def test_streams_created_and_freed_in_turn(index, sets, first):
    for rep in range(5):                                 # (cycles two to six: `first` was the first)
        assert _cycle(index, sets) == first, "cycle %d" % (rep + 2)


def test_free_waits_for_queued_work(index, sets, first):
    """the contract of h2g_stream_free: a run still queued or under way ends before its buffers, events and streams go"""
    st = _stream(index, sets)
    _fill(st, 0, sets[0])
    st.align_pairs_run()
    st.close()                                           # no fetch, no sync
    assert _cycle(index, sets) == first


def _k(st, k):
    p = st.align_params()
    assert not p.apply_options(["-k", str(k)])
    return p


def test_buffers_grow_in_place(index, sets, first):
    m1, m2, names = sets[0]
    c1, o1 = synth.flatten_reads(m1); c2, o2 = synth.flatten_reads(m2)
    short = ["s%d" % i for i in range(N)]
    assert sum(map(len, short)) < sum(map(len, names))
    # what a fresh stream returns for -k 40 (the extra-large unit)
    st = _stream(index, sets)
    _fill(st, 0, sets[0]); st.align_pairs_run(_k(st, 40))
    want40 = _compact(st)
    st.close()

    st = _stream(index, sets)
    st.set_reads(c1, o1)
    for nm in (short, names):                            # the second set is longer: the name buffers are replaced
        st.set_read_names(nm)
        got = st.fetch_reads()
        assert got["names"] == "".join(nm).encode() and got["name_offs"].tolist() == api.Stream.pack_names(nm)[1].tolist()
        assert got["codes"].tobytes() == c1.tobytes() and got["offs"].tolist() == o1.tolist()
    for nm in (short, names):                            # mate 2's names: allocated for every set
        st.set_mates(c2, o2, nm)
        got = st.fetch_read_set(1)
        assert bytes(got["names"]) == "".join(nm).encode() and np.asarray(got["codes"]).tobytes() == c2.tobytes()
    pools = []
    for k, want in ((5, first[0]), (40, want40), (5, first[0])):      # the rows grow, the extra-large unit's pools appear, and stay
        st.align_pairs_run(_k(st, k))
        assert _compact(st) == want, "-k %d" % k
        pools.append(st.probe("pools"))
    assert pools[2] == pools[1] >= pools[0] >= 1
    st.close()


def test_index_loaded_twice_and_splice_sites_replaced(g1_index, sets):
    L = api.lib()
    sites = [(0, 1000 + 700 * i, 1000 + 700 * i + 150 + 10 * i, "+-"[i & 1]) for i in range(12)]
    arr = api.splice_site_array(sites, True)
    runs = []
    for load in range(2):
        ix = api.Index(g1_index, device=0)
        st = _stream(ix, sets)
        _fill(st, 0, sets[0])
        p = st.align_params()
        p.no_spliced_alignment = 0; p.no_temp_splicesite = 1
        for call in range(2):                            # the same call twice: the database's device buffers are written in place
            assert L.h2g_index_set_splice_sites(ix.h, arr, len(sites), 0) == 0
            st.align_pairs_run(p)
            runs.append(_compact(st))
        st.close()
        ix.close()
    assert runs[0] == runs[1] == runs[2] == runs[3] and len(runs[0][1]) > N * 40
