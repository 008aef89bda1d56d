"""CPU: the two queries of the transcriptome policy (--avoid-pseudogene, h2g_core.h) — ss_any_in (SpliceSiteDB::hasSpliceSites with
includeNovel, splice_site.cpp:436-506) and exon_inside (SpliceSiteDB::insideExon, :508-526) — compiled with the host compiler into a small
harness, the way tests/emul instantiates the H2G_HD code, against a Python restatement of the reference's two functions on random site and
exon sets.  The exon sets include overlapping exons, where insideExon's backward walk stops at the first exon that ends before the read
although an earlier, longer one would hold it: the device query must give the reference's answer there, not the full scan's."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hisat2_amd", "csrc")

HARNESS = r"""
#include <cstdio>
#include <vector>
#include "h2g_core.h"
#include "h2g_splice_db_host.h"
using namespace h2g;
// stdin: nPat nsites nexons nq, sites (tidx left right dir), exons (tidx left right; already sorted), queries (tidx a b)
// stdout per query: ss_any_in(tidx, a, b) exon_inside(tidx, a, b)
int main() {
	unsigned nPat, ns, ne, nq;
	if(scanf("%u %u %u %u", &nPat, &ns, &ne, &nq) != 4) return 1;
	std::vector<h2g_splice_site> s(ns);
	for(auto& x : s) { unsigned d; if(scanf("%u %u %u %u", &x.tidx, &x.left, &x.right, &d) != 4) return 1; x.dir = (uint8_t)d; x.readid = 0; x.fromfile = 1; x.known = 1; x.editdist = 0; }
	HostSpliceDB h;
	if(ns) build_splice_db(s.data(), s.size(), nPat, h);
	DSpliceDB db;
	if(ns) { db.fw = h.fw.data(); db.bw = h.bw.data(); db.fw_first = h.fw_first.data(); db.bw_first = h.bw_first.data(); db.n = (uint32_t)h.fw.size(); }
	std::vector<DExon> ex(ne);
	for(auto& e : ex) if(scanf("%u %u %u", &e.tidx, &e.left, &e.right) != 3) return 1;
	DExonTbl t; t.e = ex.data(); t.n = ne;
	for(unsigned i = 0; i < nq; i++) {
		unsigned tidx, a, b;
		if(scanf("%u %u %u", &tidx, &a, &b) != 3) return 1;
		printf("%d %d\n", (int)ss_any_in(db, tidx, a, b), (int)exon_inside(t, tidx, a, b));
	}
	return 0;
}
"""


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("tq")
    src, exe = os.path.join(str(d), "tq.cpp"), os.path.join(str(d), "tq")
    open(src, "w").write(HARNESS)
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", CSRC, "-o", exe, src], check=True)
    return exe


def has_splice_sites(sites, ref, L, R):
    """hasSpliceSites(ref, L, R, L, R, true): a site of `ref` with its right end (_bwIndex key) or its left end (_fwIndex key) in [L, R]"""
    if not sites:
        return False                                   # !_read: the empty database
    if L < R and any(t == ref and L <= r <= R for t, l, r, _ in sites):
        return True
    return L < R and any(t == ref and L <= l <= R for t, l, r, _ in sites)


def inside_exon(exons, ref, left, right):
    """insideExon: lower bound of Exon(ref, left + 1, 0) in the sorted list, then backwards until the first exon ending before `left`"""
    if not exons:
        return False
    key = (ref, left + 1, 0)
    i = 0
    while i < len(exons) and exons[i] < key:
        i += 1
    while i > 0:
        t, l, r = exons[i - 1]
        if r < left:
            break
        if l <= left and right <= r:
            return True
        i -= 1
    return False


def full_scan(exons, ref, left, right):
    return any(t == ref and l <= left and right <= r for t, l, r in exons)


def run(harness, npat, sites, exons, queries):
    txt = ["%d %d %d %d" % (npat, len(sites), len(exons), len(queries))]
    txt += ["%d %d %d %d" % s for s in sites]
    txt += ["%d %d %d" % e for e in exons]
    txt += ["%d %d %d" % q for q in queries]
    out = subprocess.run([harness], input="\n".join(txt) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return [tuple(int(v) for v in l.split()) for l in out if l.strip()]


def random_case(seed, npat=3, span=60000, nsites=40, nexons=60):
    rng = np.random.default_rng(seed)
    sites = []
    for _ in range(nsites):
        t = int(rng.integers(0, npat))
        l = int(rng.integers(0, span))
        sites.append((t, l, l + int(rng.integers(30, 8000)), int(rng.choice([2, 3]))))
    exons = []
    for _ in range(nexons):
        t = int(rng.integers(0, npat))
        l = int(rng.integers(0, span))
        exons.append((t, l, l + int(rng.integers(20, 3000))))
        if rng.random() < 0.3:                          # a short exon inside a long one: the early break matters
            ll = l + int(rng.integers(0, 1500))
            exons.append((t, ll, ll + int(rng.integers(5, 200))))
    exons.sort()
    queries = []
    for _ in range(400):
        t = int(rng.integers(0, npat))
        if rng.random() < 0.5 and exons:                # near an exon
            e = exons[int(rng.integers(0, len(exons)))]
            a = max(0, e[1] + int(rng.integers(-50, 300)))
            t = e[0]
        else:
            a = int(rng.integers(0, span))
        b = a + int(rng.integers(40, 300))
        L, R = (a - 10000 if a > 10000 else 0), b + 10000
        queries.append((t, L, R) if rng.random() < 0.5 else (t, a, b))
    return sites, exons, queries


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_queries_match_the_reference_restatement(harness, seed):
    sites, exons, queries = random_case(seed)
    got = run(harness, 3, sites, exons, queries)
    assert len(got) == len(queries)
    want = [(int(has_splice_sites(sites, t, a, b)), int(inside_exon(exons, t, a, b))) for t, a, b in queries]
    assert got == want
    assert 0 < sum(g[0] for g in got) < len(got) and 0 < sum(g[1] for g in got) < len(got)


def test_early_break_differs_from_a_full_scan(harness):
    """(0, 100, 5000) holds [1000, 1100], but (0, 500, 600) sorts after it and ends before 1000: the walk stops there"""
    exons = sorted([(0, 100, 5000), (0, 500, 600), (1, 0, 90000)])
    queries = [(0, 1000, 1100), (0, 200, 300), (0, 520, 580), (1, 10, 20), (0, 5001, 5002)]
    got = [g[1] for g in run(harness, 2, [], exons, queries)]
    assert got == [int(inside_exon(exons, *q)) for q in queries] == [0, 1, 1, 1, 0]
    assert full_scan(exons, 0, 1000, 1100)                                      # ... which a full scan would have found
    # the random sets hold such cases too
    n = 0
    for seed in range(1, 5):
        _, ex, qs = random_case(seed)
        n += sum(1 for t, a, b in qs if full_scan(ex, t, a, b) and not inside_exon(ex, t, a, b))
    assert n > 0


def test_walk_crosses_into_the_previous_text(harness):
    """the reference walks its one sorted list without a text check: an exon of text 0 can answer for text 1"""
    exons = sorted([(0, 0, 100000), (1, 50000, 50100)])
    q = (1, 1000, 1100)
    assert inside_exon(exons, *q)
    assert run(harness, 2, [], exons, [q])[0][1] == 1


def test_empty_database_and_table(harness):
    assert run(harness, 2, [], [], [(0, 0, 100), (1, 5, 50000)]) == [(0, 0), (0, 0)]
