"""The graph primitives, the group walk above all, at EVERY capacity set that ships (tests/dense_cases.py CAPS): the *_big units', the default units' and the graph
fast pass's own (h2g_go_fast_graph_caps.h).  tests/emul builds one stand-alone program per set (h2g_caps_check_*: text in, text out); every result is either the
reference's vector or flagged as a capacity hit, and a flag must be owed: a case that, by the oracle's read-outs, fits inside the set is equal.  The fixtures are
gdense (tests/dense_cases.py: in-edge lists and node ranges of up to 64) and g1s.  The same programs built with AddressSanitizer + UBSan run the gdense inputs as
child processes (`make -C tests/emul sanitize`)."""
import gzip
import os
import subprocess

import pytest

import dense_cases as DC
import h2o_py as H
import parity_cases as PC

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL = os.path.join(HERE, "emul")
SETS = ("big", "gdef", "gfast")
MAXU = 0xFFFFFFFF


def prog(cs, san=False):
    return os.path.join(EMUL, f"h2g_caps_check_{cs}" + ("_san" if san else ""))


def run_prog(cs, args, san=False):
    r = subprocess.run([prog(cs, san)] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, (cs, args[0], r.returncode, err[-3000:])
    return r.stdout.decode().splitlines()


def flat_reads(golden_dir, fn, dst):
    """a committed FASTA of reads as the programs read them: one line of bases per read"""
    with gzip.open(os.path.join(golden_dir, fn), "rt") as f, open(dst, "w") as o:
        o.writelines(l for l in f if not l.startswith(">"))
    return str(dst)


@pytest.fixture(scope="module")
def work(tmp_path_factory, golden_dir, oracle_lib):
    """the indexes unpacked, the vector and read files of the programs written, the oracle's read-outs taken: once for the module"""
    d = tmp_path_factory.mktemp("caps")
    subprocess.run(["make", "-s", "-C", EMUL], check=True)
    w = {"dir": d, "gdense": PC.unpack_index(golden_dir, "gdense", d), "g1s": PC.unpack_index(golden_dir, "g1s", d)}
    w["caps"] = {}
    for cs in SETS:
        kv = run_prog(cs, ["caps"])[0].split()
        w["caps"][cs] = dict(zip(kv[0::2], map(int, kv[1::2])))
    for name, fns in (("gdense", ["probe_gdense_coords.txt.gz"]), ("g1s", ["probe_g1s_coords.txt.gz", "probe_g1s_coords_short.txt.gz"])):
        cases = [c for fn in fns for c in PC.parse_graph_coords(golden_dir, fn)]
        ix = H.load_index(oracle_lib, w[name])
        w[name + "_coords"] = cases
        w[name + "_needs"] = DC.coords_needs(oracle_lib, ix, cases)
        vf = d / f"{name}_coords.txt"
        with open(vf, "w") as o:
            for top, bot, nt, nb, ie, hlen, strad, want in cases:
                o.write(" ".join(map(str, [top, bot, nt, nb, hlen, len(ie)] + [x for p in ie for x in p])) + "\n")
        w[name + "_coords_file"] = str(vf)
    w["kmers"] = flat_reads(golden_dir, "reads_gdense_kmers.fa.gz", d / "kmers.txt")
    w["snp_reads"] = flat_reads(golden_dir, "reads_snp.fa.gz", d / "reads_snp.txt")
    for tag in ("se", "pe_1", "pe_2"):
        w[tag] = flat_reads(golden_dir, f"reads_gdense_{tag}.fa.gz", d / f"reads_{tag}.txt")
    # psearch / extend / adjust vectors: the query part of every line of the reference's files
    for name, reads, files in (("gdense", "kmers", {"psearch": "probe_gdense_psearch.txt.gz", "extend": "probe_gdense_extend.txt.gz", "adjust": "probe_gdense_adjust.txt.gz"}),
                               ("g1s", "snp_reads", {"psearch": "probe_g1s_psearch.txt.gz", "extend": "probe_g1s_extend.txt.gz", "adjust": "probe_g1s_adjust.txt.gz"})):
        for mode, fn in files.items():
            lines = H.glines(golden_dir, fn)
            nq = 2 if mode == "psearch" else 8 if mode == "extend" else 7
            vf = d / f"{name}_{mode}.txt"
            with open(vf, "w") as o:
                o.writelines(" ".join(l.split()[:nq]) + "\n" for l in lines)
            w[f"{name}_{mode}"] = (w[reads], str(vf), lines)
    return w


def test_capacity_sets_are_the_shipped_ones(work):
    """the programs are compiled with what ships: the *_big header, no header, the header h2g_k_go_fast_graph.hip includes"""
    for cs in SETS:
        c = work["caps"][cs]
        assert (c["H2G_IEDGE_CAP"], c["H2G_GW_MAXELT"], c["H2G_GW_MAXST"]) == DC.CAPS[cs] and c["H2G_GW_MAXROWS"] == 64 and c["FG_GRAPH"] == 1
    f = work["caps"]["gfast"]
    assert (f["H2G_GHIT_EDITS"], f["H2G_NEW_EDITS"], f["H2G_AWA_CAND"], f["H2G_AWA_DEPTH"]) == (12, 8, 4, 12)
    import ctypes
    for name, edits in (("libh2gemu_gdef.so", 32), ("libh2gemu_gfast.so", 12)):          # the emulator itself builds at both sets (working hits of 32 and of 12 edits)
        assert ctypes.CDLL(os.path.join(EMUL, name)).h2gemu_ghit_edits() == edits
    src = open(os.path.join(HERE, "..", "hisat2_amd", "csrc", "h2g_k_go_fast_graph.hip")).read()
    assert '#include "h2g_go_fast_graph_caps.h"' in src and "#define H2G_GW_MAXELT" not in src       # one source for the kernel's and the host's


def test_fixture_windows(work):
    """gdense reaches every window between the capacity sets (counted from the reference's vectors and the oracle's walk of them)"""
    w = DC.windows(work["gdense_coords"], work["gdense_needs"])
    print("gdense windows", w, "most states", max(n[1] for n in work["gdense_needs"]))
    assert w["ie3_4"] >= 50 and w["ie5_8"] >= 50 and w["ie9_24"] >= 20 and w["nodes5_8"] >= 50 and w["nodes9_24"] >= 50
    g = DC.windows(work["g1s_coords"], work["g1s_needs"])
    print("g1s windows", g)


@pytest.mark.parametrize("name", ["gdense", "g1s"])
@pytest.mark.parametrize("cs", SETS)
def test_coords_equal_or_flagged(work, cs, name):
    """genome_coords_graph_item: the reference's coordinates, or res.ok == 0 with nsteps == H2G_MAX; and only a case that does not fit the set may be flagged"""
    cases, needs = work[name + "_coords"], work[name + "_needs"]
    out = run_prog(cs, ["coords", work[name], work[name + "_coords_file"]])
    assert len(out) == len(cases)
    nflag = nfit = 0
    for (top, bot, nt, nb, ie, hlen, strad, want), need, l in zip(cases, needs, out):
        f = l.split()
        ok, nco, st, nsteps = map(int, f[:4])
        flagged = ok == 0 and nsteps == MAXU
        fit = DC.fits(need, DC.CAPS[cs])
        nflag += flagged; nfit += fit
        assert not (fit and flagged), ("flagged although it fits", cs, top, bot, need)
        if not flagged:
            got = [tuple(int(x) for x in c.split(":")) for c in f[4:]]
            assert ok == 1 and st == strad and got == want, (cs, top, bot, need, l)
    print(f"{name} at {cs}: {len(cases)} coordinate cases, {nfit} fit, {nflag} flagged ({100.0 * nflag / len(cases):.1f} %)")
    if cs == "big":
        # nothing but a list longer than the 24 entries an h2g_iedges stores is a capacity hit of the large units on these fixtures
        assert nflag == sum(1 for n in needs if n[0] > 24)
    if name == "gdense":
        assert nflag > 0 and nflag < len(cases)          # the capacity path ran, and so did the walk
    elif cs != "gfast":
        assert nflag == 0


@pytest.mark.parametrize("name", ["gdense", "g1s"])
@pytest.mark.parametrize("cs", SETS)
def test_partial_search_equal_or_counted(work, cs, name):
    """partial_search_graph_item: every field the reference's; the in-edge list's count is the true one and its stored entries (H2G_IEDGE_CAP of them) the first of
    the reference's list: a longer list is counted, never stored"""
    reads, vf, lines = work[name + "_psearch"]
    out = run_prog(cs, ["psearch", work[name], reads, vf])
    cap = DC.CAPS[cs][0]
    assert len(out) == len(lines)
    nlong = 0
    for l, g in zip(lines, out):
        f = l.split()
        want, wie = f[2:15], f[16:]
        got, gie = g.split(" | ")[0].split(), g.split(" | ")[1].split()
        assert got == want and int(gie[0]) == len(wie) == int(f[15]) and gie[1:] == wie[:cap], (cs, l, g)
        nlong += len(wie) > cap
    print(f"{name} at {cs}: {len(lines)} searches, {nlong} with a list longer than {cap}")
    if name == "gdense" and cs == "gfast":
        assert nlong > 0                                 # the counted-not-stored path ran


def _edits_fit(nedits, c):
    return nedits <= min(c["H2G_GHIT_EDITS"], c["H2G_NEW_EDITS"])


@pytest.mark.parametrize("name", ["gdense", "g1s"])
@pytest.mark.parametrize("cs", SETS)
def test_extend_equal_or_flagged(work, cs, name):
    """extend_item_alts: the reference's extension, or the hit's overflow bit; an extension whose edits fit the working hit and one extension's budget is equal"""
    reads, vf, lines = work[name + "_extend"]
    out = run_prog(cs, ["extend", work[name], reads, vf])
    assert len(out) == len(lines)
    nflag = 0
    for l, g in zip(lines, out):
        want = l.split(" -> ")[1].split()
        got = g.split()
        flagged = got[0] != "0"
        nflag += flagged
        assert not (flagged and _edits_fit(int(want[8]), work["caps"][cs])), ("flagged although it fits", cs, l, g)
        if not flagged:
            assert got[1:] == want, (cs, l, g)
    print(f"{name} at {cs}: {len(lines)} extensions, {nflag} flagged")


@pytest.mark.parametrize("name", ["gdense", "g1s"])
@pytest.mark.parametrize("cs", SETS)
def test_adjust_equal_or_flagged(work, cs, name):
    """adjust_with_alt: the reference's hits, or the overflow flag; a case whose hits all fit the working hit is equal"""
    reads, vf, lines = work[name + "_adjust"]
    out = run_prog(cs, ["adjust", work[name], reads, vf])
    assert len(out) == len(lines)
    nflag = 0
    for l, g in zip(lines, out):
        parts = l.split(" -> ")[1].split(" | ")
        found, nh = map(int, parts[0].split())
        gp = g.split(" | ")
        ovf, gnh = map(int, gp[0].split())
        nflag += ovf != 0
        fit = nh <= 8 and all(_edits_fit(int(p.split()[4]), work["caps"][cs]) for p in parts[1:])
        assert not (ovf and fit), ("flagged although it fits", cs, l, g)
        if not ovf:
            assert gnh == nh and (nh > 0) == bool(found) and [p.split() for p in gp[1:]] == [p.split() for p in parts[1:]], (cs, l, g)
    print(f"{name} at {cs}: {len(lines)} adjustments, {nflag} flagged")


@pytest.mark.parametrize("paired", [False, True])
def test_fast_lane_at_its_own_capacities(work, paired):
    """the fast lane compiled at the graph fast pass's capacities over the 2000 reads / 1000 pairs of gdense's alternate haplotype, against the MACHINE of the *_big
    build (which tests/test_go_parity_cpu.py holds to the reference binary): what the lane completes is the machine's result (the fields the emulator's own lane check compares), and reads leave it for
    the group walk's capacities (FB_GWALK)"""
    files = [work["pe_1"], work["pe_2"]] if paired else [work["se"]]
    mach = run_prog("big", ["machine", work["gdense"]] + files)
    fast = run_prog("gfast", ["fast", work["gdense"]] + files)
    assert len(mach) == len(fast) == (DC.N_PAIRS if paired else DC.N_READS)
    gwalk = work["caps"]["gfast"]["FB_GWALK"]
    ndone = ngw = 0
    bad = []
    for i, (m, f) in enumerate(zip(mach, fast)):
        done, bail, dig = f.split()
        if done == "1":
            ndone += 1
            if dig != m.split()[0]:
                bad.append(i)
        else:
            ngw += int(bail) == gwalk
    print(f"gdense {'pairs' if paired else 'reads'}: lane completed {ndone} of {len(fast)}, {ngw} handed on for the group walk's capacities")
    assert not bad, bad[:20]
    assert ndone > 0 and ngw > 0


@pytest.mark.parametrize("cs", SETS)
def test_sanitized_program_runs_clean(work, cs):
    """the program of each capacity set built with -fsanitize=address,undefined, as a child process over the gdense inputs: exit 0 and no report"""
    subprocess.run(["make", "-s", "-j3", "-C", EMUL, "sanitize"], check=True)          # (all three at the first call)
    run_prog(cs, ["coords", work["gdense"], work["gdense_coords_file"]], san=True)
    for mode in ("psearch", "extend", "adjust"):
        reads, vf, _ = work[f"gdense_{mode}"]
        run_prog(cs, [mode, work["gdense"], reads, vf], san=True)
    run_prog(cs, ["fast", work["gdense"], work["se"]], san=True)
    run_prog(cs, ["fast", work["gdense"], work["pe_1"], work["pe_2"]], san=True)
