"""The fast pass (hisat2_amd/csrc/h2g_fast.h) at every capacity of its compact state, on the host: the planted reads and pairs of tests/fastcap_cases.py through
tests/emul/h2g_fastcap_check (linear index) and h2g_fastcap_check_g (SNP-graph index), which run every unit through the general machine and through the pass and
read out how far the unit filled the state.  What the pass completes is the machine's result; for every capacity there are units that completed with the array
exactly full ("at") and units that left for that capacity's reason ("over"), at least FLOOR of each; the windows no input reaches are listed in UNREACHABLE
with the highest value that was reached (DESIGN.md 3.1 has the table and the state that leaves first); and the families land where their labels say, so that a
changed capacity names the family that moved.  The same programs built with AddressSanitizer + UBSan run the same units as child processes."""
import collections
import os
import subprocess

import pytest

import fast_caps_util as U

pytestmark = pytest.mark.skipif(not os.path.exists(U.BUILD), reason="needs oracle/_ref/hisat2-build-s")
FLOOR = 20
# (capacity, window) no input reaches -> the largest mark of a completed unit, on either kind of index.  DESIGN.md 3.1 says which state leaves first.
UNREACHABLE = {("npairs", "over"): 4, ("localhits", "over"): 2, ("partial", "at"): 12, ("partial", "over"): 12}
# reasons no unit leaves for; every other reason of the issue's list must occur
NEVER = {"lin": {"localhits", "gsearch", "redundant", "npairs", "partial"},
         "graph": {"localhits", "gsearch", "redundant", "npairs", "partial", "indel", "gwalk"}}
REASONS_THAT_MATTER = {"input", "longpool", "subsample", "coords", "nghits", "edits", "depth", "localhits", "gsearch", "nres", "searched", "redundant", "mate", "npairs",
                       "partial", "straddle", "indel"}
# (family, parameter, variant without its strand sign or None = any) -> (outcome, least share of the family's units, kinds).  outcome: a bail reason, "done", or
# ("done", mark, value): completed with that mark of the read-out, or a dict {outcome: units}: the family's exact split
LABELS = [
    (("full", 1, "s0"), "done", 1.0, U.KINDS), (("full", 2, "s0"), "done", 1.0, ("lin",)), (("full", 3, "s0"), "nres", 1.0, ("lin",)), (("full", 4, "s0"), "nres", 1.0, ("lin",)),
    (("full", 5, "s0"), "nghits", 1.0, ("lin",)), (("full", 6, "s0"), "coords", 1.0, ("lin",)), (("full", 7, "s0"), "coords", 1.0, ("lin",)),
    (("full", 8, "s0"), "coords", 1.0, ("lin",)), (("full", 9, "s0"), "coords", 1.0, ("lin",)), (("full", 12, "s0"), "subsample", 1.0, ("lin",)),
    (("full", 40, "s0"), "subsample", 1.0, U.KINDS),
    (("tandem", 2, "s0"), "done", 1.0, U.KINDS), (("tandem", 3, "s0"), "nres", 0.85, U.KINDS), (("tandem", 4, "s0"), "nres", 0.85, U.KINDS),
    (("tandem", 5, "s0"), "nghits", 0.85, U.KINDS), (("tandem", 6, "s0"), "coords", 0.85, U.KINDS),
    (("tandempair", 2, "s0"), "done", 1.0, U.KINDS), (("tandempair", 3, "s0"), "nres", 0.85, U.KINDS), (("tandempair", 5, "s0"), "nghits", 0.85, U.KINDS),
    (("tandempair", 6, "s0"), "coords", 0.85, U.KINDS),
    (("chimera", 2, "s0"), "done", 1.0, U.KINDS), (("chimera", 6, "s0"), "nghits", 0.85, U.KINDS), (("chimera", 7, "s0"), "longpool", 0.9, U.KINDS),
    (("chimera", 8, "s0"), "longpool", 1.0, U.KINDS),
    (("length", 31, None), "input", 1.0, U.KINDS), (("length", 32, None), "done", 1.0, U.KINDS), (("length", 128, None), "done", 1.0, U.KINDS),
    (("length", 129, None), "input", 1.0, U.KINDS), (("n", 1, "s0"), "input", 1.0, U.KINDS),
    (("indel", 1, None), "indel", 1.0, ("lin",)), (("indel", 1, None), "done", 1.0, ("graph",)),
    (("pairs4", 4, "s0"), ("done", "npairs", 4), 1.0, U.KINDS), (("evensub", 5, "default"), ("done", "pool", 6), 0.75, ("lin",)),
    (("subst", 4, "default"), "done", 1.0, ("lin",)),
    (("straddle", 81, None), "straddle", 1.0, U.KINDS), (("pair", 6, "rescue"), "mate", 0.7, U.KINDS),
] + [(("overlap", k, v), ("done", "localhits", 2), 1.0, U.KINDS) for k in range(7, 16) for v in ("c2", "r2")]
# The full copies on the graph index: the shared variants of a family widen the node ranges, so a family splits over two or three outcomes by where a read's
# window lies against the variants.  The split itself is the label, as measured: 50 units per family
LABELS += [((("full", c, "s0"), split, 1.0, ("graph",))) for c, split in (
    (2, {"coords": 26, "done": 24}), (3, {"subsample": 10, "coords": 30, "nres": 10}), (4, {"subsample": 10, "coords": 30, "nres": 10}),
    (5, {"subsample": 10, "coords": 30, "nghits": 10}), (6, {"subsample": 26, "coords": 24}), (7, {"subsample": 26, "coords": 24}),
    (8, {"subsample": 26, "coords": 24}), (9, {"subsample": 26, "coords": 24}), (12, {"subsample": 40, "coords": 10}))]


@pytest.fixture(scope="module", params=U.KINDS)
def staged(request, tmp_path_factory):
    """the case of one index kind on disk and the plain program's read-out of it: once for the module"""
    subprocess.run(["make", "-s", "-j2", "-C", U.EMUL], check=True)
    w = U.stage(request.param, tmp_path_factory.mktemp("fastcap_" + request.param))
    w["rows"] = U.read_out(w)
    return w


def test_capacities_are_the_shipped_ones(staged):
    """the program is the pass as it ships (FG_ALIGN_MATE=0, the index kind's build) and the capacities this module counts windows for are the header's"""
    out = subprocess.run([U.prog(staged["kind"]), "caps"], stdout=subprocess.PIPE, check=True).stdout.decode().split()
    c = dict(zip(out[0::2], map(int, out[1::2])))
    assert c["FG_GRAPH"] == (staged["kind"] == "graph") and c["FG_ALIGN_MATE"] == 0 and c["FS_WORDS"] == 40 + 8 * c["FG_GRAPH"]
    have = {"edits": c["FG_FE"], "coords": c["FG_NCO"], "nghits": c["FG_NGH"], "nres": c["FG_NRES"], "searched": c["FG_NSRCH"], "npairs": c["FG_NPAIR"],
            "frames": c["FG_NFRAME"], "localhits": c["FG_NLOCAL"], "pool": c["FG_NLONG"] + c["FG_NLONGC"], "partial": 16}
    assert have == {k: v[1] for k, v in U.CAPS.items()}


def test_nothing_mismatches(staged):
    rows, units = staged["rows"], staged["units"]
    bad = [units[i]["label"] for i, r in enumerate(rows) if not r["equal"]]
    done, why = U.bails(rows)
    print(f"{staged['kind']}: {len(rows)} units, {done} completed, handed on: {why}")
    assert not bad, bad[:10]
    assert 3000 <= len(units) <= 9000 and done > len(rows) // 2


def test_sanitized_program_gives_the_same_read_out(staged):
    """the program built with -fsanitize=address,undefined over the same units, as a child process: exit 0, no report, and line for line the plain program's output"""
    subprocess.run(["make", "-s", "-j2", "-C", U.EMUL, "sanitize"], check=True)
    assert U.read_out(staged, san=True) == staged["rows"]


def test_windows(staged):
    """every capacity has its two windows: at least FLOOR units completed with the array exactly full, at least FLOOR left for its reason; a window of
    UNREACHABLE is empty and the highest value reached is the one the table says"""
    kind = staged["kind"]
    tab = U.windows(staged["units"], staged["rows"])
    print(f"\n{kind} index: capacity windows (units)\n{'capacity':<10} {'cap':>3} {'at':>5} {'over':>5} {'reached':>7}")
    for cap, t in tab.items():
        print(f"{cap:<10} {U.CAPS[cap][1]:>3} {len(t['at']):>5} {len(t['over']):>5} {t['reached']:>7}")
    for cap, t in tab.items():
        for win in ("at", "over"):
            n = len(t[win])
            if (cap, win) in UNREACHABLE:
                assert n == 0 and t["reached"] == UNREACHABLE[(cap, win)], (kind, cap, win, n, t["reached"])
            else:
                assert n >= FLOOR, (kind, cap, win, n, collections.Counter(l[:2] for l in t[win]).most_common(5))
        if (cap, "at") not in UNREACHABLE:
            assert t["reached"] == U.CAPS[cap][1], (kind, cap, t["reached"])       # nothing completes beyond a capacity


def test_reasons(staged):
    """every reason a read can leave for occurs, except the ones DESIGN.md 3.1 shows unreachable — and those do not occur"""
    kind = staged["kind"]
    _, why = U.bails(staged["rows"])
    want = REASONS_THAT_MATTER | ({"iedges", "gwalk"} if kind == "graph" else set())
    for r in sorted(want):
        if r in NEVER[kind]:
            assert why.get(r, 0) == 0, (kind, r, why)
        else:
            assert why.get(r, 0) >= 1, (kind, r, why)
    assert why.get("other", 0) == 0 and why.get("tail", 0) == 0, why


def test_labels_behave(staged):
    """a family's units land where its label says"""
    kind, units, rows = staged["kind"], staged["units"], staged["rows"]
    fam = collections.defaultdict(list)
    for u, r in zip(units, rows):
        f, p, v = u["label"]
        fam[(f, p, v[:-1])].append(r)
        fam[(f, p, None)].append(r)
    moved = []
    for key, outcome, share, kinds in LABELS:
        if kind not in kinds:
            continue
        rs = fam[key]
        assert rs, key
        split = dict(collections.Counter("done" if r["done"] else U.REASONS[r["bail"]] for r in rs))
        if isinstance(outcome, dict):
            if split != outcome:
                moved.append((key, outcome, split))
            continue
        if isinstance(outcome, tuple):
            hit = sum(1 for r in rs if r["done"] and U.mark(r, outcome[1]) == outcome[2])
        elif outcome == "done":
            hit = sum(1 for r in rs if r["done"])
        else:
            hit = sum(1 for r in rs if not r["done"] and U.REASONS[r["bail"]] == outcome)
        if hit < share * len(rs):
            moved.append((key, outcome, hit, len(rs), split))
    assert not moved, (kind, moved)
