"""GPU parity tests (run with -m gpu on an MI355X): every call goes through the C ABI of libh2g.so and is
compared bit-for-bit with the golden vectors of the real reference and with the C oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import h2o_py as H
import parity_cases as PC
from hisat2_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu(g1_index, golden_dir):
    ix = api.Index(g1_index, device=0)
    reads, offs = PC.load_reads(golden_dir)
    st = api.Stream(ix, max_reads=200000, max_bases=200000 * 101)
    st.set_reads(reads.reshape(-1), offs)
    yield st
    st.close()
    ix.close()


def test_index_info(gpu, golden_dir):
    kv = H.glines(golden_dir, "probe_params.txt.gz")[0].split()
    d = dict(zip(kv[0::2], map(int, kv[1::2])))
    info = gpu.ix.info
    for k in ("len", "gbwtLen", "numNodes", "lineRate", "offRate", "ftabChars", "eftabLen", "linear", "sideSz",
              "sideGbwtSz", "sideGbwtLen", "numSides", "offsLen", "nPat", "nFrag"):
        assert getattr(info, k) == d[k], k


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_rank_golden(gpu, golden_dir, variant):
    PC.check_rank(lambda r, c: gpu.rank(r, c, variant=variant)[0], golden_dir)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_rank_vs_oracle_random(gpu, oracle_lib, g1_index, variant):
    oix = H.load_index(oracle_lib, g1_index)
    g = C.byref(oix.contents.g)
    rng = np.random.default_rng(5 + variant)
    n = 50001   # ragged tail: not a multiple of any group size
    rows = rng.integers(0, gpu.ix.info.gbwtLen, size=n, dtype=np.uint32)
    rows[:4] = [0, 1, gpu.ix.info.gbwtLen - 1, 191]
    cs = rng.integers(0, 4, size=n, dtype=np.uint8)
    got, _ = gpu.rank(rows, cs, variant=variant)
    want = np.array([oracle_lib.h2o_rank(g, int(r), int(c)) for r, c in zip(rows, cs)], dtype=np.uint32)
    assert np.array_equal(got, want)


def test_rank_variants_agree_on_grch38_scale_sides():
    """Size-independent property at roofline scale: three differently-organised kernels give the same
    checksum over 2^24 queries on a 1 GB synthetic side array, and rank(row, c) summed over c == row."""
    ix = api.Index(synth_sides=15_300_000, seed=7)
    st = api.Stream(ix)
    n = 1 << 24
    cks = [st.rank_synth(n, 20260925, variant=v)[1] for v in (0, 1, 2)]
    assert cks[0] == cks[1] == cks[2] and cks[0] != 0
    rng = np.random.default_rng(1)
    rows = rng.integers(0, ix.info.gbwtLen, size=4096, dtype=np.uint32)
    tot = np.zeros(len(rows), dtype=np.uint64)
    for c in range(4):
        r, _ = st.rank(rows, np.full(len(rows), c, dtype=np.uint8), variant=1)
        tot += r
    # sum_c rank(row,c) = sum_c fchr[c] + row  (every symbol before `row` is one of A,C,G,T)
    base = int(tot[0]) - int(rows[0])
    assert np.array_equal(tot, rows.astype(np.uint64) + np.uint64(base))
    st.close()
    ix.close()


def test_fm_search_golden(gpu, golden_dir):
    assert PC.check_fm_search(gpu, golden_dir, "probe_psearch.txt.gz", 0) == 800
    assert PC.check_fm_search(gpu, golden_dir, "probe_psearch_spliced.txt.gz", 1) == 800


def test_coords_golden(gpu, golden_dir):
    assert PC.check_coords(gpu, golden_dir) > 300


def test_extend_golden(gpu, golden_dir):
    assert PC.check_extend(gpu, golden_dir) > 1000


def test_seed_stage_vs_oracle(gpu, oracle_lib, g1_index, golden_dir):
    contigs = PC.load_contigs(golden_dir)
    reads, _ = synth.make_reads(contigs, 3000, 101, 78, sub_rate=0.02, indel_rate=0.001, n_rate=0.002)
    codes, offs = synth.flatten_reads(reads)
    gpu.set_reads(codes, offs)
    oix = H.load_index(oracle_lib, g1_index)
    for nospl in (True, False):
        p = gpu.seed_params(no_spliced=nospl)
        assert p.pseudogeneStop == (0 if nospl else 1)
        gpu.seed_extend_run(p)
        got = gpu.seed_extend_fetch()
        want = PC.oracle_seed_extend(oracle_lib, oix, reads, p.pseudogeneStop)
        PC.assert_seed_equal(got, want)
    c = gpu.counters()
    assert c.n_rank == int(got["hit"]["nrank"].sum()) and c.n_side == int(got["hit"]["nside"].sum())
    assert c.n_sa_steps == int(got["nsteps"].sum())


def test_ragged_and_edge_reads(gpu, oracle_lib, g1_index, golden_dir):
    """Reads of different lengths in one batch: shorter than the ftab window, all-N, N inside the ftab window,
    very long (250 bp)."""
    contigs = PC.load_contigs(golden_dir)
    g = contigs[0]
    seqs = [g[100:105], g[200:210], g[300:311], np.full(40, 4, dtype=np.uint8), g[1000:1250].copy(), g[5000:5101].copy(),
            H.revcomp(g[7000:7101])]
    seqs[5][95] = 4
    seqs.append(g[20000:20030])
    codes = np.concatenate(seqs)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint32)
    gpu.set_reads(codes, offs)
    qs = [api.FmQuery(i, 0, fw, 0, 0, 1) for i in range(len(seqs)) for fw in (1, 0)]
    out = gpu.fm_search(qs)
    oix = H.load_index(oracle_lib, g1_index)
    for q, o in zip(qs, out):
        s = np.ascontiguousarray(seqs[q.read] if q.fw else H.revcomp(seqs[q.read]))
        w = H.BwtHit()
        oracle_lib.h2o_partial_search(oix, s.ctypes.data, len(s), 0, 0, 1, 5, C.byref(w))
        assert [getattr(o, f) for f in api.FM_HIT_FIELDS] == [getattr(w, f) for f in api.FM_HIT_FIELDS], (q.read, q.fw)


def test_bad_arguments_are_rejected(gpu):
    with pytest.raises(api.H2GError):
        gpu.fm_search([api.FmQuery(10 ** 7, 0, 1, 0, 0, 1)])
    with pytest.raises(api.H2GError):
        gpu.sa_resolve([api.SaQuery(5, 5, 1, 20, 0)])
    with pytest.raises(api.H2GError):
        api.Index("/nonexistent/base")


def test_full_size_properties(tmp_path):
    """Config-2-sized workload (4.9 Mbp linear index, 200 k reads): error-free reads must come back as one
    full-length, score-0 extension at the position they were drawn from (size-independent property; the
    oracle is too slow to sweep this size in a test)."""
    build = os.path.join(ROOT, "oracle", "_ref", "hisat2-build-s")
    if not os.path.exists(build):
        pytest.skip("oracle/_ref/hisat2-build-s not available to build the large index")
    contigs = synth.make_genome([4_900_000], 20260925 + 2)
    fa = tmp_path / "big.fa"
    synth.write_fasta(str(fa), contigs)
    subprocess.run([build, "-q", str(fa), str(tmp_path / "big")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    n = 200_000
    reads, truth = synth.make_reads(contigs, n, 101, 99, sub_rate=0.0)
    codes, offs = synth.flatten_reads(reads)
    ix = api.Index(str(tmp_path / "big"))
    st = api.Stream(ix, max_reads=n, max_bases=codes.size)
    st.set_reads(codes, offs)
    st.seed_extend_run(st.seed_params(True))
    res = st.seed_extend_fetch()
    strand = np.where(truth[:, 2] == 1, 0, 1)          # fw reads align on the fw strand entry
    rec = res[np.arange(n) * 2 + strand]
    one = rec["ncoords"] >= 1
    assert one.mean() > 0.999
    e0 = rec["ext"][:, 0]
    okpos = (e0["toff"] == truth[:, 1]) & (e0["len"] == 101) & (e0["rdoff"] == 0) & (e0["score"] == 0) & (e0["tidx"] == 0)
    assert (okpos | ~one | (rec["ncoords"] > 1)).mean() > 0.9999
    # idempotence: a second run over the resident batch gives identical bytes
    st.seed_extend_run(st.seed_params(True))
    assert res.tobytes() == st.seed_extend_fetch().tobytes()
    st.close()
    ix.close()


# ---------------------------------------------------------------- graph (GFM) index: 128 B sides, F/M bit vectors
@pytest.fixture(scope="module")
def ggpu(g1s_index, golden_dir):
    ix = api.Index(g1s_index, device=0)
    reads, offs = PC.load_snp_reads(golden_dir)
    st = api.Stream(ix, max_reads=1000, max_bases=1000 * 101)
    st.set_reads(reads.reshape(-1), offs)
    yield st
    st.close()
    ix.close()


def test_graph_index_info(ggpu, golden_dir):
    kv = H.glines(golden_dir, "probe_g1s_params.txt.gz")[0].split()
    d = dict(zip(kv[0::2], map(int, kv[1::2])))
    info = ggpu.ix.info
    assert info.linear == 0 and info.sideSz == 128
    for k in ("len", "gbwtLen", "numNodes", "lineRate", "sideSz", "sideGbwtSz", "sideGbwtLen", "numSides", "offsLen"):
        assert getattr(info, k) == d[k], k


@pytest.mark.parametrize("variant", [0, 1])
def test_graph_rank_golden(ggpu, golden_dir, variant):
    assert PC.check_graph_rank(lambda r, c: ggpu.rank(r, c, variant=variant)[0], golden_dir) == 3000


@pytest.mark.parametrize("variant", [0, 1])
def test_graph_rank_vs_oracle_random(ggpu, oracle_lib, g1s_index, variant):
    oix = H.load_index(oracle_lib, g1s_index)
    g = C.byref(oix.contents.g)
    rng = np.random.default_rng(15 + variant)
    n = 30001
    rows = rng.integers(0, ggpu.ix.info.gbwtLen, size=n, dtype=np.uint32)
    rows[:5] = [0, 1, ggpu.ix.info.gbwtLen - 1, 207, 208]
    cs = rng.integers(0, 4, size=n, dtype=np.uint8)
    got, _ = ggpu.rank(rows, cs, variant=variant)
    want = np.array([oracle_lib.h2o_rank(g, int(r), int(c)) for r, c in zip(rows, cs)], dtype=np.uint32)
    assert np.array_equal(got, want)


def test_graph_lf_golden(ggpu, golden_dir):
    assert PC.check_graph_lf(ggpu, golden_dir) == 6000


def test_graph_fm_search_golden(ggpu, golden_dir):
    assert PC.check_graph_fm_search(ggpu, golden_dir) == 600
    # h2g_fm_search on a graph index forwards to the graph search with kseeds = max(5, 2 khits)
    qs = [api.FmQuery(r, 0, fw, 0, 0, 1) for r in range(50) for fw in (1, 0)]
    a = ggpu.fm_search(qs, khits=10)
    b, _ = ggpu.fm_search_graph(qs, khits=10, kseeds=20)
    for x, y in zip(a, b):
        assert [getattr(x, f) for f in api.FM_HIT_FIELDS[:13]] == [getattr(y, f) for f in api.FM_HIT_FIELDS[:13]]


def test_graph_genome_coords_golden(ggpu, golden_dir):
    n, multi = PC.check_graph_coords(ggpu, golden_dir, "probe_g1s_coords.txt.gz")
    assert n > 250 and multi >= 4
    n, multi = PC.check_graph_coords(ggpu, golden_dir, "probe_g1s_coords_short.txt.gz")
    assert n > 3000 and multi >= 100


def test_graph_extend_with_alts_golden(ggpu, golden_dir):
    assert PC.check_graph_extend(ggpu, golden_dir) > 1000


def test_graph_adjust_with_alt_golden(ggpu, golden_dir):
    assert PC.check_graph_adjust(ggpu, golden_dir, "probe_g1s_adjust.txt.gz") > 250


# ---- the in-edge-rich graph gdense (tests/dense_cases.py) through the C-ABI primitives: the DEFAULT capacities (in-edge lists of 24, 24 nodes, 40 states), so
# a result is the reference's or flagged, and only a case that, by the oracle's walk of it, does not fit those capacities may be flagged
@pytest.fixture(scope="module")
def dgpu(tmp_path_factory, golden_dir):
    import dense_cases as DC
    base = PC.unpack_index(golden_dir, "gdense", tmp_path_factory.mktemp("gdense"))
    ix = api.Index(base, device=0)
    codes, offs = DC.load_kmers(golden_dir)
    st = api.Stream(ix, max_reads=len(offs) - 1, max_bases=int(codes.size))
    st.set_reads(codes, offs)
    st.base = base
    yield st
    st.close()
    ix.close()


def test_dense_genome_coords_equal_or_flagged(dgpu, oracle_lib, golden_dir):
    import dense_cases as DC
    cases = PC.parse_graph_coords(golden_dir, "probe_gdense_coords.txt.gz")
    needs = DC.coords_needs(oracle_lib, H.load_index(oracle_lib, dgpu.base), cases)
    n, nflag = DC.check_coords_abi(dgpu, cases, needs, DC.CAPS["gdef"])
    print("gdense coordinates on the device:", n, "cases,", nflag, "flagged")
    assert n > 1500 and 0 < nflag == sum(1 for x in needs if not DC.fits(x, DC.CAPS["gdef"]))


def test_dense_partial_search_extend_adjust(dgpu, golden_dir):
    import dense_cases as DC
    n, nlong = DC.check_psearch_abi(dgpu, golden_dir)
    assert n == 6000
    n, nflag = DC.check_extend_abi(dgpu, golden_dir)
    assert n > 10000 and nflag == 0          # (no extension of a k-mer comes near 24 new edits)
    n, nflag = DC.check_adjust_abi(dgpu, golden_dir)
    assert n > 2500 and nflag == 0


def test_graph_lf_vs_oracle_random(ggpu, oracle_lib, g1s_index):
    oix = H.load_index(oracle_lib, g1s_index)
    g = C.byref(oix.contents.g)
    glen = oix.contents.g.p.gbwtLen
    rng = np.random.default_rng(199)
    qs = []
    for _ in range(30000):
        top = int(rng.integers(0, glen - 2))
        spread = int(rng.integers(2, 7)) if rng.random() < 0.5 else int(rng.integers(2, 600))
        if min(glen, top + spread) > top + 1:
            qs.append(api.GlfQuery(top, min(glen, top + spread), int(rng.integers(0, 4)), 0))
    res, ie = ggpu.graph_lf(qs, k=20)
    u32 = C.c_uint32
    nie = 0
    for q, r, e in zip(qs, res, ie):
        a, b, na, nb, n = u32(), u32(), u32(), u32(), u32()
        buf = (u32 * 128)()
        ok = oracle_lib.h2o_map_glf(g, q.top, q.bot, q.c, 20, a, b, na, nb, buf, 64, n)
        assert bool(ok) == bool(r.ok)
        if ok:
            assert (r.top, r.bot, r.node_top, r.node_bot) == (a.value, b.value, na.value, nb.value)
            assert e.n == n.value and e.pairs() == [(buf[2 * i], buf[2 * i + 1]) for i in range(min(n.value, 24))]
            nie += n.value > 0
    assert nie > 10


def test_graph_rank_variants_agree_on_large_synthetic_sides():
    """1 GB of synthetic 128 B graph sides: both kernels give the same checksum; sum_c rank(row, c) == row + const"""
    ix = api.Index(synth_sides=8_000_000, seed=11, graph=True)
    assert ix.info.linear == 0 and ix.info.sideSz == 128
    st = api.Stream(ix)
    n = 1 << 23
    cks = [st.rank_synth(n, 20260925, variant=v)[1] for v in (0, 1)]
    assert cks[0] == cks[1] and cks[0] != 0
    rng = np.random.default_rng(2)
    rows = rng.integers(0, ix.info.gbwtLen, size=4096, dtype=np.uint32)
    tot = np.zeros(len(rows), dtype=np.uint64)
    for c in range(4):
        r, _ = st.rank(rows, np.full(len(rows), c, dtype=np.uint8), variant=1)
        tot += r
    base = int(tot[0]) - int(rows[0])
    assert np.array_equal(tot, rows.astype(np.uint64) + np.uint64(base))
    st.close()
    ix.close()


def test_rank_synth_sampled_vs_oracle(oracle_lib):
    """the micro-benchmark's own query stream (h2g_rank_bench_synth: rows drawn on the device) on the synthetic side array, every 256th output of every kernel variant
    against the ORACLE's mapLF over the same array rebuilt on the host (SURVEY §8(d)'s sampled check; bench.py does the same at 2^28 queries / 2^20 samples).  Variant 10
    keeps no output stream (every result into the checksum, every 256th stored): its checksum must be variant 0's."""
    import rank_synth_check as RC
    nsides, seed, n, stride = 300_000, 20260925, 1 << 22, 256
    want = RC.sampled_expect(oracle_lib, nsides, seed, n, stride, n // stride)
    ix = api.Index(synth_sides=nsides, seed=seed, device=0)
    st = api.Stream(ix)
    cks = {}
    for variant in (0, 1, 2, 10):
        _, cks[variant] = st.rank_synth(n, seed, variant=variant, repeats=1)
        got = st.rank_synth_sample(stride, n // stride)
        assert int((want != got).sum()) == 0, variant
    assert len(set(cks.values())) == 1, cks
    st.close(); ix.close()
