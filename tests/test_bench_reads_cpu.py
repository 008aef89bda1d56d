"""bench.py's set-up on the host: the read batches its worker processes make are the ones synth.make_pairs makes with each batch's seed (and the
names are the packed decimal ids), and expected_headline_total names, before any build, the genome size headline_index then settles on.  No
device and no index builder are needed."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench                                    # noqa: E402
import build_bench_index as BB                  # noqa: E402  (bench.py puts tools/ on the path)
from hisat2_amd import api, synth               # noqa: E402


@pytest.mark.parametrize("workers", [1, 2, 3])
def test_read_batches_equal_make_pairs(workers):
    contigs = synth.make_genome([6000, 4000, 3000], 11)
    npairs, nbatch, n_global, lo, rank = 37, 3, 74, 37, 1
    got = list(bench.ReadBatches(contigs, npairs, nbatch, n_global, lo, rank, workers))
    assert [g[0] for g in got] == list(range(nbatch))
    for b, m1, m2, packed in got:
        w1, w2 = synth.make_pairs(contigs, npairs, 101, bench.SEED + 7 + 1000 * rank + 100003 * b, sub_rate=0.005)
        assert m1.shape == (npairs, 101) and np.array_equal(m1, w1) and np.array_equal(m2, w2)
        names, offs = api.Stream.pack_names([str(b * n_global + lo + i) for i in range(npairs)])
        assert packed[0] == names and np.array_equal(packed[1], offs)


def test_read_batches_worker_failure_raises():
    """a worker that cannot make its batch ends the iteration with an error instead of leaving the caller waiting"""
    with pytest.raises(RuntimeError, match="read batch"):
        list(bench.ReadBatches([np.zeros(10, np.uint8)], 5, 2, 5, 0, 0, 2))        # a contig too short to draw pairs from


def _fake_index(cache, total):
    base = BB.index_base(total, cache)
    for k in range(1, 9):
        open("%s.%d.ht2" % (base, k), "w").close()
    return base


@pytest.fixture
def no_builds(monkeypatch):
    """BB.build records the size asked for and 'builds' empty files instead of running the reference's builder"""
    asked = []

    def build(total, threads=None, timeout=None, cache=None):
        asked.append(total)
        return _fake_index(cache, total)
    monkeypatch.setattr(BB, "build", build)
    monkeypatch.delenv("H2G_BENCH_BUILD_BUDGET", raising=False)
    monkeypatch.setenv("H2G_BENCH_FALLBACK_GENOME", "2e6")
    return asked


def _agree(cache, want):
    planned = bench.expected_headline_total(cache, want)
    base, total, how = bench.headline_index(cache, want)
    assert planned == total and base == BB.index_base(total, cache)
    return total, how


def test_expected_total_nothing_staged(tmp_path, no_builds):
    assert _agree(str(tmp_path), 5_000_000)[0] == 5_000_000 and no_builds == [5_000_000]


def test_expected_total_staged_exact_and_larger(tmp_path, no_builds):
    cache = str(tmp_path)
    _fake_index(cache, 9_000_000)
    assert _agree(cache, 5_000_000) == (9_000_000, "staged")             # the largest staged index above the wanted size
    _fake_index(cache, 5_000_000)
    assert _agree(cache, 5_000_000) == (5_000_000, "staged")             # exactly the wanted size when it is there
    assert _agree(cache, 3_000_000) == (9_000_000, "staged")             # not exact: the largest
    assert no_builds == []


def test_expected_total_over_budget_marker(tmp_path, no_builds):
    cache = str(tmp_path)
    with open(BB.index_base(5_000_000, cache) + ".over_budget", "w") as f:
        f.write("1250\n")
    total, how = _agree(cache, 5_000_000)
    assert total == 2_000_000 and how.startswith("FALLBACK") and no_builds == [2_000_000]
