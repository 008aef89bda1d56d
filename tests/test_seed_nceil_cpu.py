"""CPU tests of --n-ceil and --seed: the N ceiling of h2g_core.h (nceil_value / nceil_pass / nceil_dp, compiled for the host) against a Python
restatement of SimpleFunc::f (simple_func.h:86-108) at lengths where the (int) / (size_t) truncation and (double)0.15f against 0.15 decide;
the reference's --n-ceil token rules through api.parse_n_ceil; the host emulator's filter with the changed headers; genRandSeed's starting product."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from hisat2_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hisat2_amd", "csrc")
F015 = float(np.float32(0.15))
DMAX = 1.7976931348623157e308


def simple_f(t, c, l, x):
    """SimpleFunc::f<double> with I = 0, X = DMAX (aligner_seed_policy.cpp:294): std::max(I, std::min(X, C + L * X))"""
    X = {1: 0.0, 2: float(x), 3: math.sqrt(x), 4: math.log(x)}[t]
    v = c + l * X
    hi = v if v < DMAX else DMAX
    return hi if 0.0 < hi else 0.0


def ref_pass(t, c, l, n, ns):      # Scoring::nFilter: ns <= f<size_t>(len)
    f = simple_f(t, c, l, n)
    return f == DMAX or ns <= int(f)


def ref_dp(t, c, l, n):            # min(f<int>(len), len)
    f = simple_f(t, c, l, n)
    return n if f == DMAX else min(int(f), n)


FUNCS = [(2, 0.0, F015), (2, 0.0, 0.15), (2, 0.0, 0.05), (1, 5.0, F015), (1, 0.0, F015), (2, 3.0, F015), (3, 1.0, 2.0), (4, 0.0, 4.0),
         (2, -10.0, 0.1), (1, 2.5, 0.0), (2, 0.0, 1.0), (2, 0.0, 2.0), (3, -1.0, 0.5), (4, 0.5, 1.0)]
# 20, 40, 60, 80, 100 ...: 0.15 x len is an integer in exact arithmetic; (double)0.15f lies above 0.15, 0.15 below
LENS = [2, 3, 7, 19, 20, 21, 33, 40, 60, 80, 100, 101, 120, 140, 150, 151, 200, 250, 300, 1000, 20000]


@pytest.fixture(scope="module")
def nceil_exe(tmp_path_factory):
    t = tmp_path_factory.mktemp("nceil")
    src = t / "nceil.cpp"
    src.write_text('#include <stdio.h>\n#include "h2g_core.h"\nusing namespace h2g;\n'
                   'int main() { unsigned t, n, ns; double c, l;\n'
                   '  while(scanf("%u %lf %lf %u %u", &t, &c, &l, &n, &ns) == 5)\n'
                   '    printf("%d %d %.17g\\n", (int)nceil_pass(t, c, l, n, ns), nceil_dp(t, c, l, n), nceil_value(t, c, l, n));\n'
                   '  return 0; }\n')
    exe = t / "nceil"
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", CSRC, "-o", str(exe), str(src)], check=True)
    return str(exe)


def test_n_ceiling_matches_simple_func(nceil_exe):
    cases = []
    for (t, c, l) in FUNCS:
        for n in LENS:
            f = simple_f(t, c, l, n)
            for ns in sorted({0, 1, n, max(0, min(n, int(f))), max(0, min(n, int(f) + 1)), max(0, min(n, int(f) - 1))}):
                cases.append((t, c, l, n, ns))
    inp = "".join("%d %r %r %d %d\n" % x for x in cases)
    out = subprocess.run([nceil_exe], input=inp, capture_output=True, text=True, check=True).stdout.split("\n")
    for (t, c, l, n, ns), line in zip(cases, out):
        p, dp, v = line.split()
        assert float(v) == simple_f(t, c, l, n), (t, c, l, n)
        assert int(p) == int(ref_pass(t, c, l, n, ns)), (t, c, l, n, ns)
        assert int(dp) == ref_dp(t, c, l, n), (t, c, l, n)
    assert len(cases) > 500


def test_float_coefficient_matters():
    """the default coefficient is (double)0.15f: at lengths where 0.15 x len is an integer, 0.15 would give the same floor, but a
    coefficient of 0.15f x 1e4 would not; L,3 is 3 + 0.15f x len"""
    assert F015 > 0.15
    assert ref_dp(2, 3.0, F015, 100) == 18
    assert ref_dp(2, 0.0, F015, 20) == 3 and ref_dp(2, 0.0, 0.05, 20) == 1
    assert ref_dp(1, 0.0, F015, 100) == 0           # C,0: no N allowed
    assert ref_pass(1, 0.0, F015, 100, 0) and not ref_pass(1, 0.0, F015, 100, 1)


@pytest.mark.parametrize("arg,want", [
    ("L,0,0.05", (2, 0.0, 0.05)), ("5", (1, 5.0, F015)), ("C,0", (1, 0.0, F015)), ("L,3", (2, 3.0, F015)),
    ("S,1,2", (3, 1.0, 2.0)), ("G,0,4", (4, 0.0, 4.0)), ("Linear,1", (2, 1.0, F015)), ("C,2x", (1, 2.0, F015)), ("C,abc", (1, 0.0, F015)),
])
def test_parse_n_ceil(arg, want):
    assert api.parse_n_ceil(arg) == want


@pytest.mark.parametrize("arg,msg", [
    ("0,0.15", "Error: Bad function type '0'."),
    ("L,0,1,2", "Error: expected 3 or fewer comma-separated arguments to --n-ceil option, got 4"),
    (",,", "Error: expected at least one argument to --n-ceil option"),
])
def test_parse_n_ceil_refusals(arg, msg):
    with pytest.raises(ValueError) as e:
        api.parse_n_ceil(arg)
    assert str(e.value).startswith(msg)


def test_params_defaults_and_options():
    p = api.AlignParams()
    p.n_ceil_type, p.n_ceil_coeff = 2, F015
    rest = p.apply_options(["--seed", "12345", "--n-ceil", "L,3"], linear=True)
    assert not rest and p.seed == 12345 and (p.n_ceil_type, p.n_ceil_const, p.n_ceil_coeff) == (2, 3.0, F015)
    with pytest.raises(ValueError):
        api.AlignParams().apply_options(["--seed", "-1"], linear=True)


def test_header_defaults():
    """h2g_align_params_init's defaults (align_params_defaults) and AlnParams' in-class ones are the reference's"""
    src = open(os.path.join(CSRC, "h2g_align.h")).read()
    assert "p->seed = 0; p->n_ceil_type = 2; p->n_ceil_const = 0.0; p->n_ceil_coeff = (double)0.15f;" in src
    assert "static_assert(offsetof(AlnParams, seed0) == 60" in src


def test_rand_seed0():
    """genRandSeed's starting product (pat.h:59) in uint32 arithmetic, as AlnParams::seed0 carries it"""
    def seed0(s):
        v = s + 101
        for k in (59, 61, 67, 71, 73, 79, 83):
            v = (v * k) & 0xFFFFFFFF
        return v
    src = open(os.path.join(CSRC, "h2g_core.h")).read()
    assert "(seed + 101u) * 59u * 61u * 67u * 71u * 73u * 79u * 83u" in src
    assert seed0(0) != seed0(1) and seed0(2147483647) == ((2147483647 + 101) * 59 * 61 * 67 * 71 * 73 * 79 * 83) & 0xFFFFFFFF


def test_emulator_n_filter(g1_index):
    """the host emulator (tests/emul, built from the changed headers): a read with 30 Ns of 100 (its last 30 bases) is filtered by the default ceiling (go() is
    skipped: no rank call) and searched under --n-ceil C,40; a read without N is searched under C,0"""
    from h2gemu_align import emu_align
    import parity_cases as PC
    reads, offs = PC.load_reads(os.path.join(ROOT, "tests", "golden"))
    r0 = np.asarray(reads[0][:100], dtype=np.uint8).copy()
    rn = r0.copy()
    rn[70:] = 4
    assert int((rn == 4).sum()) == 30
    names = ["rn", "r0"]
    outs, _ = emu_align(g1_index, [rn, r0], names)
    assert outs[0].nrank == 0 and outs[1].nrank > 0
    outs, _ = emu_align(g1_index, [rn, r0], names, options=["--n-ceil", "C,40"])
    assert outs[0].nrank > 0
    outs, _ = emu_align(g1_index, [rn, r0], names, options=["--n-ceil", "C,0"])
    assert outs[0].nrank == 0 and outs[1].nrank > 0
