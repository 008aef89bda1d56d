"""What tests/test_fast_caps_cpu.py and tests/test_gpu_fast_caps.py share: the case of tests/fastcap_cases.py staged on disk (index by the reference's builder, read
files of tests/emul/h2g_fastcap_check), that program's read-out parsed, and the capacity windows counted from it."""
import os
import subprocess

import fastcap_cases as FCC
from fast_check import BAIL_REASONS as REASONS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMUL = os.path.join(HERE, "emul")
BUILD = os.path.join(ROOT, "oracle", "_ref", "hisat2-build-s")
KINDS = ("lin", "graph")
FIELDS = ("done", "bail", "equal", "nghits", "nco", "nres0", "nres1", "nsearched0", "nsearched1", "npairs", "nframes", "nlocal", "pool", "np0", "np1", "np2", "np3", "edits")
# capacity -> (the marks of the read-out it bounds, the largest value a read may hold, the reason a read leaves for).  h2g_fast.h: FG_FE, FG_NCO, FG_NGH, FG_NRES,
# FG_NSRCH, FG_NPAIR, FG_NFRAME, FG_NLOCAL, FG_NLONG + FG_NLONGC, the 16 partial hits of a strand (test_capacities_are_the_shipped_ones holds the numbers to the build)
CAPS = {
    "edits": (("edits",), 4, "edits"),
    "coords": (("nco",), 5, "coords"),
    "nghits": (("nghits",), 4, "nghits"),
    "nres": (("nres0", "nres1"), 2, "nres"),
    "searched": (("nsearched0", "nsearched1"), 7, "searched"),
    "npairs": (("npairs",), 4, "npairs"),
    "frames": (("nframes",), 5, "depth"),
    "localhits": (("nlocal",), 2, "localhits"),
    "pool": (("pool",), 6, "longpool"),
    "partial": (("np0", "np1", "np2", "np3"), 16, "partial"),
}


def prog(kind, san=False):
    return os.path.join(EMUL, "h2g_fastcap_check" + ("_g" if kind == "graph" else "") + ("_san" if san else ""))


def stage(kind, d):
    """the case of `kind` in directory d: index g, the groups' read files, the relaxed group's option block -> dict(base, units, G, groups {name: (unit ids, files, params)})"""
    d = str(d)
    G, units = FCC.case(kind == "graph")
    subprocess.run([BUILD] + FCC.write_genome(G, d), check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    base = os.path.join(d, "g")
    from h2gemu_py import Emu
    from h2gemu_align import set_options
    e = Emu(base, "g" if kind == "graph" else "")
    pf = os.path.join(d, "relaxed.params")
    with open(pf, "wb") as f:
        f.write(bytes(set_options(e, 0, FCC.RELAXED)))
    groups = {}
    for g in FCC.GROUPS:
        ids = [i for i, u in enumerate(units) if u["group"] == g]
        files = [os.path.join(d, f"{g}_1.txt")]
        with open(files[0], "w") as f:
            f.writelines(FCC.text_of(units[i]["r1"]) + "\n" for i in ids)
        if g == "pairs":
            files.append(os.path.join(d, f"{g}_2.txt"))
            with open(files[1], "w") as f:
                f.writelines(FCC.text_of(units[i]["r2"]) + "\n" for i in ids)
        groups[g] = (ids, files, pf if g.endswith("relaxed") else None)
    return dict(kind=kind, dir=d, base=base, units=units, G=G, groups=groups)


def read_out(w, san=False, emul=None):
    """h2g_fastcap_check over every group -> one dict of FIELDS per unit, in the units' order.  The program runs as a child process; a sanitizer report fails"""
    rows = [None] * len(w["units"])
    p = prog(w["kind"], san)
    if emul:
        p = os.path.join(emul, os.path.basename(p))
    for g, (ids, files, params) in w["groups"].items():
        r = subprocess.run([p, "run", w["base"]] + files + (["params=" + params] if params else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        err = r.stderr.decode(errors="replace")
        assert r.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, (w["kind"], g, r.returncode, err[-3000:])
        lines = r.stdout.decode().splitlines()
        assert len(lines) == len(ids), (g, len(lines), len(ids))
        for i, l in zip(ids, lines):
            rows[i] = dict(zip(FIELDS, map(int, l.split())))
    return rows


def mark(row, cap):
    return max(row[f] for f in CAPS[cap][0])


def windows(units, rows):
    """capacity -> dict(at: labels of the units that completed with the mark at the capacity, over: labels of those that left for its reason, reached: the largest
    mark of a completed unit)"""
    out = {}
    for cap, (fs, c, reason) in CAPS.items():
        at = [u["label"] for u, r in zip(units, rows) if r["done"] and mark(r, cap) == c]
        over = [u["label"] for u, r in zip(units, rows) if not r["done"] and REASONS[r["bail"]] == reason]
        reached = max((mark(r, cap) for r in rows if r["done"]), default=0)
        out[cap] = dict(at=at, over=over, reached=reached)
    return out


def bails(rows, ids=None):
    """{reason: count} and the number completed, over rows (of the unit ids given)"""
    c = {}
    done = 0
    for i in (range(len(rows)) if ids is None else ids):
        r = rows[i]
        if r["done"]:
            done += 1
        else:
            c[REASONS[r["bail"]]] = c.get(REASONS[r["bail"]], 0) + 1
    return done, c
