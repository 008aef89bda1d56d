"""The fast pass of SPLICED runs (hisat2_amd/csrc/h2g_fast.h with FG_SPLICED = 1: the configuration of h2g_k_go_fast_spl.hip) against the spliced general
machine, both instantiated on the host (tests/emul_spl/h2g_emul_spl.cpp over tests/emul): every read / pair of tests/spl_fast_cases.py through both.  What
the pass completes must equal the machine's result bit for bit (PairOut / ReadOut incl. the PRNG state and the work counters, every record); a read the
machine aligns with a splice edit is never completed; with the known-sites file loaded every read inside a decoy exon is handed on.  The share of class
(a) — reads wholly inside an exon — that completes is printed per case: tests/test_gpu_spl_fast.py takes its floor from the `gpu_layout` case."""
import os
import subprocess

import numpy as np
import pytest

import spl_fast_cases as SC
from fast_check import fast_check
from hisat2_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "oracle", "_ref", "hisat2-build-s")
pytestmark = pytest.mark.skipif(not os.path.exists(BUILD), reason="needs oracle/_ref/hisat2-build-s")

GENOME_SEED = 31
GPU_LAYOUT = dict(sub=0.005, seed=20261018)          # the reads of tests/test_gpu_spl_fast.py (there: 40 000 of each; here: the first 5 000 draws of the same generator)


@pytest.fixture(scope="module")
def emu_lib(tmp_path_factory):
    """tests/emul_spl/h2g_emul_spl.cpp with the spliced build's defines and the edit capacity of the other test libraries (tests/emul/Makefile: EDITS32)"""
    out = str(tmp_path_factory.mktemp("emuspl") / "libh2gemu_spl.so")
    subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wno-sign-compare", "-fPIC", "-shared", "-DH2G_GHIT_EDITS=32", "-DH2G_NEW_EDITS=24", "-DFG_ALIGN_MATE=0",
                    "-DFG_SPLICED=1", "-o", out, os.path.join(ROOT, "tests", "emul_spl", "h2g_emul_spl.cpp")], check=True)
    return out


@pytest.fixture(scope="module")
def index(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("splfast")
    g, _ = SC.genome(GENOME_SEED)
    fa = str(tmp / "g.fa")
    synth.write_fasta(fa, [g])
    base = str(tmp / "g")
    subprocess.run([BUILD, "-q", fa, base], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return base


def spl_check(lib, base, reads1, reads2=None, options=(), sites=None):
    """-> dict(n, completed, mismatching, bails, done flags, spl flags: the machine's result holds a splice edit)"""
    from h2gemu_py import Emu
    from h2gemu_align import set_options, set_splice_sites
    old = os.environ.get("H2GEMU_LIB")
    os.environ["H2GEMU_LIB"] = lib
    try:
        e = Emu(base)
    finally:
        if old is None:
            del os.environ["H2GEMU_LIB"]
        else:
            os.environ["H2GEMU_LIB"] = old
    set_options(e, 0, list(options))
    if sites:
        set_splice_sites(e, sites)
    r = fast_check(base, reads1, reads2, emu=e, spliced=True)
    r["done"], r["spl"] = r["done"].astype(bool), r["spl"].astype(bool)
    return r


def share_a(r, labels):
    a = labels == SC.A
    return float(r["done"][a].sum()) / max(1, int(a.sum()))


CASES = {
    "sub005": dict(sub=0.005),
    "sub03": dict(sub=0.03),
    "indel": dict(sub=0.005, indel=0.002),
    "dta": dict(sub=0.005, options=("--dta",)),
    "strand_fr": dict(sub=0.005, options=("--rna-strandness", "FR")),      # (an option of the SAM text: nothing of go() may change with it)
    "gpu_layout": dict(GPU_LAYOUT),
}


@pytest.mark.parametrize("db", (False, True), ids=("nodb", "known"))
@pytest.mark.parametrize("name", list(CASES))
def test_spliced_fast_pass_equals_the_machine(emu_lib, index, name, db):
    kw = dict(CASES[name])
    options = kw.pop("options", ())
    seed = kw.pop("seed", 1000 + sorted(CASES).index(name))
    c = SC.make(seed, 5000, 4000, genome_seed=GENOME_SEED, **kw)
    sites = c.sites if db else None
    for what, r1, r2, lab in (("reads", c.reads, None, c.rlabel), ("pairs", c.m1, c.m2, c.plabel)):
        r = spl_check(emu_lib, index, r1, r2, options=options, sites=sites)
        sa = share_a(r, lab)
        print("%s %s db=%d: completed %d of %d, class (a) share %.4f, bails %s; machine results with a splice edit: %d" % (name, what, db, r["completed"], r["n"], sa, r["bails"], int(r["spl"].sum())))
        assert r["mismatching"] == 0, (what, r["bad"], r["bails"])
        assert not (r["done"] & r["spl"]).any(), (what, np.flatnonzero(r["done"] & r["spl"])[:10])         # a read the machine aligns with a splice edit never completes
        assert r["spl"].sum() > 0.1 * r["n"]                                                                 # (... and the case has such reads)
        if db:
            cc = lab == SC.C
            assert cc.sum() > 300 and not r["done"][cc].any(), (what, np.flatnonzero(r["done"] & cc)[:10])   # every read inside a decoy exon is handed on
        # the bail rules are not too eager.  (At 3 % substitutions most reads extend through the local index, and a local hit anywhere within --max-intronlen of the
        # anchor is a would-be splice, which version 1 hands on without scoring it: the share is printed, profiles/r09_spliced_fast.md has the figures.)
        if kw["sub"] <= 0.005:
            assert sa > 0.5, (what, sa, r["bails"])
