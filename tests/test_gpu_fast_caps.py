"""The fast pass at the capacities of its compact state, on the device: the planted units of tests/fastcap_cases.py (tests/test_fast_caps_cpu.py shows on the host
which capacity windows they reach) through go() with the pass on and off, read by read.  What the device adds to the host lane is under test here: the cold words
of a slot live in HBM and are loaded and stored in parts by the queue kernel, and the batch runs three times, so a slot starts from the state its read left there.

Each arm is a process of its own (tests/fast_caps_worker.py: a stream reads its switches when it is made), with H2G_FAST_TAIL=0 and H2G_FAST_MATE_HANDOVER=0:
no tail policy and no pair parked for a drain launch, so which reads the pass completes does not follow timing (tests/test_gpu_ps0.py) and can be compared with
the host program's count exactly, reason by reason.  (The graph pass ships with group-walk capacities of its own, h2g_go_fast_graph_caps.h, while the host program
has the large units', tests/emul/Makefile; no unit of this case lies between the two, so the counts are equal on the graph index as well.)  All three groups of
units run, the relaxed one under its --score-min; the units are fed in a seeded shuffle.  The rendered SAM of every unit equals the reference aligner's, run live:
that pins the machine and the pass to the reference at these families."""
import json
import os
import subprocess
import sys

import pytest

import fast_caps_util as U
import fastcap_cases as FCC

ALIGN = os.path.join(U.ROOT, "oracle", "_ref", "hisat2-align-s")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not (os.path.exists(U.BUILD) and os.path.exists(ALIGN)), reason="needs oracle/_ref/hisat2-build-s and hisat2-align-s")]
GROUPS = FCC.GROUPS


@pytest.fixture(scope="module", params=U.KINDS)
def staged(request, tmp_path_factory):
    if not os.path.exists(U.prog(request.param)):
        subprocess.run(["make", "-s", "-j4", "-C", U.EMUL], check=True)
    w = U.stage(request.param, tmp_path_factory.mktemp("gfastcap_" + request.param))
    w["rows"] = U.read_out(w)
    return w


def _opts(group):
    return FCC.RELAXED if group.endswith("relaxed") else ()


def _arm(w, group, mode="run", pre=(), **env):
    ids, files, _ = w["groups"][group]
    e = dict(os.environ, H2G_FAST_TAIL="0", H2G_FAST_MATE_HANDOVER="0", PYTHONPATH=U.ROOT + os.pathsep + U.HERE)
    e.update(env)
    opts = ["opts=" + ";".join(_opts(group))] if _opts(group) and mode != "reuse" else []
    r = subprocess.run([sys.executable, os.path.join(U.HERE, "fast_caps_worker.py"), mode, *pre, w["base"]] + files + opts, env=e, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    return ids, json.loads(r.stdout.strip().splitlines()[-1])


def _label(w, ids, d):
    """the unit a worker's finding is about: its `id` is the unit's line in the group's file"""
    return w["units"][ids[d["id"]]]["label"]


@pytest.mark.parametrize("ps0", ["1", "0"])
@pytest.mark.parametrize("group", GROUPS)
def test_units_equal_the_machine_and_the_host_counts(staged, group, ps0):
    ids, got = _arm(staged, group, H2G_FAST_PS0=ps0)
    done, why = U.bails(staged["rows"], ids)
    print(staged["kind"], group, "ps0", ps0, {k: got[k] for k in ("n", "fast", "handed_on", "overflow", "why", "differing")}, "host", done, why)
    for d in got["first"]:
        print("differs:", _label(staged, ids, d), d)
    assert got["differing"] == 0 and got["n"] == len(ids)
    assert got["overflow"] == 0 and got["machine_overflow"] == 0
    assert got["fast"] + got["handed_on"] == len(ids)
    assert got["fast"] == done and got["why"] == why, (got["fast"], done, got["why"], why)


@pytest.mark.parametrize("group", GROUPS)
def test_rendered_sam_equals_the_reference_aligner(staged, group, tmp_path):
    """hisat2-align-s --no-spliced-alignment, run here over the same units, against go() with the pass on: (flag, rname, pos, cigar, AS) of every line of every unit"""
    import fuzz_pairs as F
    ids, files, _ = staged["groups"][group]
    units = staged["units"]
    fas = []
    for m, key in enumerate(("r1", "r2")[:len(files)]):
        fas.append(str(tmp_path / f"m{m + 1}.fa"))
        F.write_fasta_reads(fas[-1], [units[i][key] for i in ids])
    sam = str(tmp_path / "ref.sam")
    inputs = ["-1", fas[0], "-2", fas[1]] if len(fas) == 2 else ["-U", fas[0]]
    subprocess.run([ALIGN, "-f", "-p", "1", "--no-spliced-alignment", "-x", staged["base"]] + inputs + ["-S", sam] + list(_opts(group)), check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=120)
    _, got = _arm(staged, group, mode="sam", pre=(sam,))
    print(staged["kind"], group, {k: got[k] for k in ("n", "fast", "overflow", "differing")})
    for d in got["first"]:
        print("differs:", _label(staged, ids, d), d)
    assert got["n"] == len(ids) and got["fast"] > 0
    assert got["differing"] == 0 and got["overflow"] == 0


def test_pairs_with_align_mate_in_the_pass(staged):
    """H2G_FAST_AM=1: pairs that need alignMate are parked and finished by the alignMate build's drain launch instead of being handed on; the results stay the
    machine's (the split then differs from the host program's, whose build hands such pairs on: only its sum is compared)"""
    ids, got = _arm(staged, "pairs", H2G_FAST_AM="1", H2G_FAST_MATE_HANDOVER="1")
    print(staged["kind"], {k: got[k] for k in ("n", "fast", "handed_on", "overflow", "why", "differing")})
    for d in got["first"]:
        print("differs:", _label(staged, ids, d), d)
    assert got["differing"] == 0 and got["overflow"] == 0 and got["machine_overflow"] == 0
    assert got["fast"] + got["handed_on"] == len(ids)


def _slots_per_workgroup():
    """the largest H2G_FAST_SLOTS of the fast-pass kernels' sources"""
    import glob
    import re
    vals = [int(m) for fn in glob.glob(os.path.join(U.ROOT, "hisat2_amd", "csrc", "h2g_k_go_fast*.hip")) + [os.path.join(U.ROOT, "hisat2_amd", "csrc", "h2g_fast.h")]
            for m in re.findall(r"#define\s+H2G_FAST_SLOTS\s+(\d+)", open(fn).read())]
    assert vals
    return max(vals)


@pytest.mark.parametrize("group", ("reads", "pairs"))
def test_slot_reuse_within_one_launch(staged, group):
    """the units tiled by seeded permutations into two resident batches, the fast launch held to 64 workgroups (fast_reserve 192 of 256), both batches queued back
    to back.  A launch of 64 workgroups has 64 x H2G_FAST_SLOTS slots and a batch holds three times as many units, so a slot carries three units on average within
    one launch, each starting from what the one before left there.  No drain launch (H2G_FAST_ORPHAN=0).  The relaxed group is not tiled (a batch has one option block): its
    units run three times over the same slots in test_units_equal_the_machine_and_the_host_counts."""
    import fast_caps_worker as W
    assert W.REUSE_UNITS >= 3 * 64 * _slots_per_workgroup()
    ids, got = _arm(staged, group, mode="reuse", H2G_FAST_ORPHAN="0")
    print(staged["kind"], group, {k: got[k] for k in ("n", "units", "machine", "pass", "differing")})
    for d in got["first"]:
        print("differs:", _label(staged, ids, d), d)
    assert got["units"] >= W.REUSE_UNITS and got["n"] == len(ids)
    assert got["differing"] == [0, 0]
    for k in range(2):
        assert got["machine"][k]["overflow"] == 0 and got["pass"][k]["overflow"] == 0
        assert got["pass"][k]["fast"] + got["pass"][k]["handed_on"] == got["units"] and got["pass"][k]["fast"] > 0
