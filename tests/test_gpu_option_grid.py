"""The option grid (tests/option_cases.py) on the device: go() under the scoring options' edges.

1. every case with the fast pass on against off (tests/fast_digest.py with the case's options and qualities; one process per digest, H2G_FAST_TAIL=0 so that which units
   the pass completes is a property of the code): equal SHA-256 over every result and record — a record beyond 32 edits with its list from the long-edit area —, equal
   `aligned`; a `takes` case completes at least the table's floor of the batch in the pass, a `bails_whole` case hands every unit on.  Pairs and reads on the 2 Mbp linear
   index.  Three cases (qualities, the 16-bit edge, long records) again through the drain launch and with alignMate in the pass.
2. the device against the reference binary for the cases no other device test compares: every SAM line of 5000 reads and of 5000 pairs.
3. the run's own refusals: a hand-filled block with a penalty go() divides by (or counts down with) below 1 is H2G_ERR_ARG by name before anything is launched, and the
   stream runs the next good block as if nothing had happened.

The host side of the same table is tests/test_option_grid_cpu.py (there the machine is pinned to the reference for every case)."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import option_cases as OC
import sam_util as SU
from hisat2_amd import api, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
needs_ref = pytest.mark.skipif(not os.path.exists(os.path.join(REF, "hisat2-align-s")), reason="needs oracle/_ref")
N = OC.N_DEVICE
DIGEST_TIMEOUT = 300
# the cases no other device test holds against the reference: the four --score-min forms, --mp 40,0 on FASTQ, --ignore-quals, --np 40, the gap extremes, --sp 1 / 40, -X 120 / 100000
REFERENCE_CASES = ("l-3", "s-5-4", "g-20-8", "mp1-l-0.6", "mp40-0-fastq", "ignore-quals", "np40", "gaps1", "gaps40-20", "sp1", "sp40", "x120", "x100000")
N_REFERENCE = 5000
H2G_ERR_ARG = -4            # include/h2g.h


def _build(contigs, variants=None):
    tmp = tempfile.mkdtemp(prefix="h2optd")
    fa, base = os.path.join(tmp, "g.fa"), os.path.join(tmp, "g")
    synth.write_fasta(fa, contigs)
    snp = []
    if variants:
        synth.write_snps(os.path.join(tmp, "g.snp"), variants)
        snp = ["--snp", os.path.join(tmp, "g.snp")]
    subprocess.run([os.path.join(REF, "hisat2-build-s"), "-q", "-p", "16"] + snp + [fa, base], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return tmp, base


@pytest.fixture(scope="module")
def indexes():
    """the module's index builds: DEVICE_GENOME as a linear index and, made when first asked for, as a SNP graph -> kind -> (tmp, base, contigs the reads come from, records, variants)"""
    made = {}

    def get(kind):
        if kind not in made:
            if kind == "linear":
                contigs = OC.make_genome(OC.DEVICE_GENOME)
                made[kind] = _build(contigs) + (contigs, contigs, None)
            else:
                contigs, var, alt = OC.make_graph(OC.DEVICE_GENOME)
                made[kind] = _build(contigs, var) + (alt, contigs, var)
        return made[kind]
    return get


_NPZ, _OFF = {}, {}


def _npz(c, idx, kind):
    """the case's batch as fast_digest.py reads it (flat codes and offsets, qualities for FASTQ); one file per read set"""
    tmp, _, src = idx[:3]
    s = OC.read_set(c, src, N, OC.DEVICE_GENOME["seed"])
    key = (kind, id(s), c.device_pairs)
    if key not in _NPZ:
        kw = {}
        for k, q in (("m1", "q1"), ("m2", "q2"), ("reads", "qr")):
            lst = s[k] if k == "reads" else s[k][:c.device_pairs]
            kw[k + "_codes"], kw[k + "_offs"] = OC._flat(lst)
            if s[q] is not None:
                kw[k + "_quals"] = s[q][:kw[k + "_codes"].size]
        _NPZ[key] = os.path.join(tmp, "reads%d.npz" % len(_NPZ))
        np.savez(_NPZ[key], **kw)
    return _NPZ[key]


def _digest(base, npz, opts, fast, **knobs):
    env = dict(os.environ, H2G_GO_FAST=fast, H2G_FAST_TAIL="0", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"), **knobs)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fast_digest.py"), base, npz] + list(opts), env=env, capture_output=True, text=True, timeout=DIGEST_TIMEOUT)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in r.stderr:
        pytest.exit("a digest process faulted (status %d): nothing more is started on this device\n%s" % (r.returncode, r.stderr[-2000:]), returncode=3)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _off(c, idx, kind):
    if (c.name, kind) not in _OFF:
        _OFF[(c.name, kind)] = _digest(idx[1], _npz(c, idx, kind), c.opts, "0")
    return _OFF[(c.name, kind)]


def _check(c, off, on, what):
    print(c.name, what, "off", off, "on", on)
    for i, k in enumerate(("pairs", "reads")):
        n = c.device_pairs if k == "pairs" else N
        assert off[k]["fast"] == 0
        if c.name in OC.DEVICE_MACHINE_ONLY:            # the plan keeps the run off the fast pass: the two processes ran the same passes
            assert on[k]["fast"] == 0 and on[k]["handed_on"] == 0 and on[k]["sha"] == off[k]["sha"] and on[k]["aligned"] == off[k]["aligned"], (c.name, what, k, on[k])
            continue
        assert on[k]["fast"] + on[k]["handed_on"] == n, (c.name, what, k, on[k])
        assert on[k]["aligned"] == off[k]["aligned"], (c.name, what, k)
        assert on[k]["overflow"] == off[k]["overflow"] and (c.flags or on[k]["overflow"] == 0), (c.name, what, k, on[k])
        assert on[k]["long_edits"] == off[k]["long_edits"], (c.name, what, k)
        assert on[k]["sha"] == off[k]["sha"], (c.name, what, k)
        if c.expect == "bails_whole":
            assert on[k]["fast"] == 0 and on[k]["handed_on"] == n, (c.name, what, k, on[k])
        else:
            assert on[k]["fast"] >= c.floors[i] * n, (c.name, what, k, on[k])


# The SNP-graph half of the grid (one case per group: OC.GRAPH_CASES) runs on the host only (tests/test_option_grid_cpu.py).  On the device its first case,
# --mp 300,300 --score-min C,-29000 with the fast pass on, ended in an illegal memory access whose cause is not found: the in-edge-list overrun of gw_advance that a
# host sanitizer build of that unit's capacities showed is closed (tests/test_graph_caps_cpu.py), but this case's own input runs clean through the sanitized fast lane at
# those capacities with and without that fix, so it is not shown to be the cause.  Until the cause is found, no case of the grid runs through k_go_fast_graph here.
GRID = [(c, "linear") for c in OC.CASES]


@needs_ref
@pytest.mark.parametrize("c,kind", GRID, ids=[f"{c.name}-{k}" for c, k in GRID])
def test_fast_pass_on_against_off(indexes, c, kind):
    idx = indexes(kind)
    _check(c, _off(c, idx, kind), _digest(idx[1], _npz(c, idx, kind), c.opts, "1"), kind)


@needs_ref
@pytest.mark.parametrize("knobs", [dict(H2G_FAST_ORPHAN="64", H2G_DRAIN_GRID="8"), dict(H2G_FAST_AM="1")], ids=["drain", "align-mate"])
@pytest.mark.parametrize("name", OC.DEVICE_EXTRA_CASES)
def test_fast_pass_through_the_drain_launch_and_with_align_mate(indexes, name, knobs):
    c, idx = OC.BY_NAME[name], indexes("linear")
    on = _digest(idx[1], _npz(c, idx, "linear"), c.opts, "1", **knobs)
    _check(c, _off(c, idx, "linear"), on, "+".join(knobs))
    if "H2G_DRAIN_GRID" in knobs:
        assert on["pairs"]["adopted"] + on["reads"]["adopted"] > 0, on          # the drain launch did take slots over


def test_the_long_edit_case_has_long_records(indexes):
    """(reads the digests of the cases above: no run of its own)"""
    if not os.path.exists(os.path.join(REF, "hisat2-align-s")):
        pytest.skip("needs oracle/_ref")
    c, idx = OC.BY_NAME[OC.DEVICE_EXTRA_CASES[2]], indexes("linear")
    off = _off(c, idx, "linear")
    assert off["reads"]["long_edits"] >= 50 and off["pairs"]["long_edits"] >= 50, off


# ---------------------------------------------------------------- the device against the reference binary
class _LongRec:
    """a record beyond 32 edits with its list out of the long-edit area, in the shape sam_util / pe_sink read"""
    def __init__(self, r, led):
        for f in ("fw", "tidx", "toff", "len", "trim5", "trim3", "nedits", "score"):
            setattr(self, f, getattr(r, f))
        at = r.edits[0].pos
        self.edits = [led[at + k] for k in range(r.nedits)]


class _Recs:
    def __init__(self, rows, st):
        self.rows = rows
        self.led, self.used = st.align_fetch_long_edits()
        self.nlong = 0

    def row(self, j):
        return self.rows[j]

    def __getitem__(self, j):
        r = self.row(j)
        if r.nedits <= api.MAX_EDITS:
            return r
        assert r.edits[0].pos + r.nedits <= self.used
        self.nlong += 1
        return _LongRec(r, self.led)


class _DenseRecs(_Recs):
    """the dense fetch's records of one mate set, addressed as the comparison addresses fixed rows: [pair * DENSE_STRIDE + k]"""
    def __init__(self, rows, offs, st):
        _Recs.__init__(self, rows, st)
        self.offs = offs

    def row(self, j):
        i, k = divmod(j, DENSE_STRIDE)
        assert int(self.offs[i]) + k < int(self.offs[i + 1])
        return self.rows[int(self.offs[i]) + k]


DENSE_STRIDE = 1 << 16


class _Out:
    def __init__(self, r):
        self.overflow, self.depth = int(r["overflow"]), int(r["depth"])


def _reads_backend(base, reads, qnames, refnames, quals=None, options=()):
    reads = [np.asarray(r, dtype=np.uint8) for r in reads]
    codes, offs = OC._flat(reads)
    ix = api.Index(base, device=0)
    st = api.Stream(ix, max_reads=len(reads), max_bases=codes.size)
    st.set_reads(codes, offs, quals)
    st.set_read_names(qnames)
    p = st.align_params()
    assert not p.apply_options(list(options))
    st.align_run(p)
    res, aln = st.align_fetch()
    got = SU.render_selected(res, _Recs(aln, st), refnames, reads, qnames)
    st.close(); ix.close()
    return [_Out(r) for r in res], got


def _pairs_backend(base, m1, m2, q1, q2, quals=None, options=()):
    (c1, o1), (c2, o2) = OC._flat(m1), OC._flat(m2)
    ix = api.Index(base, device=0)
    st = api.Stream(ix, max_reads=len(m1), max_bases=max(c1.size, c2.size))
    st.set_reads(c1, o1, None if quals is None else quals[0])
    st.set_read_names(q1)
    st.set_mates(c2, o2, q2, None if quals is None else quals[1])
    p = st.align_params()
    assert not p.apply_options(list(options))
    st.align_pairs_run(p)
    # the dense fetch returns every record of a pair; the fixed rows of h2g_align_pairs_fetch hold 16 per mate and flag a pair with more (bit 4), which a minimum
    # score of -303 produces
    res, a1, f1, a2, f2 = st.align_pairs_fetch_dense()
    a1, a2 = _DenseRecs(a1, f1, st), _DenseRecs(a2, f2, st)
    # (finish_pair reads the rows while the comparison runs: the long-edit area was copied out above, the stream can go)
    st.close(); ix.close()
    return res, a1, a2


@needs_ref
@pytest.mark.parametrize("kind", ["reads", "pairs"])
@pytest.mark.parametrize("name", REFERENCE_CASES)
def test_device_equals_the_reference(indexes, name, kind):
    import fuzz_align as FA
    import fuzz_pairs as FP
    c = OC.BY_NAME[name]
    _, base, src, records, _ = indexes("linear")
    s = OC.read_set(c, src, N, OC.DEVICE_GENOME["seed"])
    n = N_REFERENCE
    cut = lambda q, lst: None if q is None else q[:sum(len(r) for r in lst[:n])]        # noqa: E731
    info = {}
    try:
        bad = _reference_case(FA, FP, c, s, n, cut, kind, records, base, info)
    except api.H2GError as e:           # a device error in this process: end the session, the other cases would run on the same device
        pytest.exit("device error in %s %s: %s" % (name, kind, e), returncode=3)
    assert bad == 0 and info["overflow"] == 0, (name, kind, bad, info["overflow"])


def _reference_case(FA, FP, c, s, n, cut, kind, records, base, info):
    if kind == "reads":
        bad, _ = FA.run_case(7, genome=(records, None), reads=s["reads"][:n], quals=cut(s["qr"], s["reads"]), extra=c.opts, verbose=3, info=info, ref_timeout=300, base=base,
                             backend=_reads_backend)
    else:
        q = None if s["q1"] is None else (cut(s["q1"], s["m1"]), cut(s["q2"], s["m2"]))
        bad, _ = FP.run_case(7, genome=(records, None), pairs=(s["m1"][:n], s["m2"][:n]), quals=q, extra=c.opts, verbose=3, info=info, ref_timeout=300, base=base,
                             backend=_pairs_backend, stride=DENSE_STRIDE)
    return bad


# ---------------------------------------------------------------- the run's refusals
BAD_BLOCKS = [("sc_min", dict(sc_min=0, sc_max=0)), ("sc_min", dict(sc_min=-3)), ("mm_max", dict(mm_max=0, mm_min=0)), ("mm_min", dict(mm_max=1, mm_min=3)),
              ("rdg_linear", dict(rdg_linear=0)), ("rfg_linear", dict(rfg_linear=-1))]


def test_a_block_that_cannot_run_is_refused_before_anything_is_launched(g1_index, golden_dir):
    """h2g_align_run and h2g_align_pairs_run: H2G_ERR_ARG with the field's name in h2g_last_error, no change in any counter, and the good run that follows gives
    the bytes of the good run before.  Nothing here is run with such a block."""
    import h2o_py as H
    _, s1 = H.read_fasta_reads(os.path.join(golden_dir, "reads_pe_1.fa.gz"))
    _, s2 = H.read_fasta_reads(os.path.join(golden_dir, "reads_pe_2.fa.gz"))
    (c1, o1), (c2, o2) = OC._flat(s1), OC._flat(s2)
    q = [str(i) for i in range(len(s1))]
    ix = api.Index(g1_index, device=0)
    st = api.Stream(ix, max_reads=len(s1), max_bases=max(c1.size, c2.size))
    st.set_reads(c1, o1); st.set_read_names(q); st.set_mates(c2, o2, q)
    def counters():
        c = st.counters()
        return tuple(int(getattr(c, f)) for f in ("n_rank", "n_side", "n_sa_steps", "n_queries", "n_aligned", "n_overflow", "n_second_pass", "n_fast", "n_fast_bail", "n_adopted"))

    def good(paired):
        p = st.align_params()
        if paired:
            st.align_pairs_run(p)
            res, a1, f1, a2, f2 = st.align_pairs_fetch_dense()
            return hashlib.sha256(bytes(res) + f1.tobytes() + f2.tobytes()).hexdigest(), int(st.counters().n_aligned)
        st.align_run(p)
        res, aln, offs = st.align_fetch_dense()
        return hashlib.sha256(res.tobytes() + offs.tobytes()).hexdigest(), int(st.counters().n_aligned)

    for paired in (False, True):
        want = good(paired)
        assert want[1] > 100
        before = counters()
        for field, values in BAD_BLOCKS:
            p = st.align_params()
            for k, v in values.items():
                setattr(p, k, v)
            rc = (api.lib().h2g_align_pairs_run if paired else api.lib().h2g_align_run)(st.h, p)
            assert rc == H2G_ERR_ARG, (field, values, rc)
            msg = api.lib().h2g_last_error().decode()
            assert msg.startswith("align: ") and field in msg, (field, msg)
            assert counters() == before, (field, "a refused run changed the counters")
        assert good(paired) == want
    st.close(); ix.close()
