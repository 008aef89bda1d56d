"""GPU: every read set the reference takes, through the `hisat2-align-amd` command line, against `oracle/_ref/hisat2-align-s` run live on the same files:
tabbed files that mix pairs and unpaired reads, -1/-2 together with -U, QSEQ with --qc-filter (also through the C ABI: h2g_set_read_filter), --seed on tabbed
pairs, and --un / --al / --un-conc / --al-conc / --al-conc-disc (by the wrapper script's rule applied to the reference's SAM, and against files the wrapper wrote)."""
import gzip
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import readsets_util as R
import sam_lines as SL
from test_sam_lines import diff_lines

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "hisat2_amd", "hisat2-align-amd")
FRONT = os.path.join(ROOT, "hisat2_amd", "hisat2-amd")          # the front end: the read-file options (--un, --al-conc ...) are its own, as in the reference
REF = os.path.join(ROOT, "oracle", "_ref", "hisat2-align-s")
needs_ref = pytest.mark.skipif(not os.path.exists(REF), reason="needs oracle/_ref")
KINDS = ("un", "al", "un-conc", "al-conc", "al-conc-disc")


@pytest.fixture(scope="module")
def genome(golden_dir):
    return R.load_genome(golden_dir)


def run_ref(args, sam, err, p=1):
    subprocess.run([REF, "-p", str(p)] + (["--reorder"] if p > 1 else []) + [str(a) for a in args] + ["-S", str(sam)], check=True, stderr=open(err, "w"))


def run_amd(args, sam, err, p=3, exe=CLI, **kw):
    return subprocess.run([exe, "-p", str(p)] + [str(a) for a in args] + ["-S", str(sam)], stderr=open(err, "w"), **kw)


def same_output(tmp, tag, ref_args, amd_args=None, ref_p=1, amd_p=3):
    ref_sam, ref_err, amd_sam, amd_err = (tmp / f"{tag}.{x}" for x in ("ref.sam", "ref.err", "amd.sam", "amd.err"))
    run_ref(ref_args, ref_sam, ref_err, p=ref_p)
    run_amd(ref_args if amd_args is None else amd_args, amd_sam, amd_err, p=amd_p, check=True)
    want = SL.body_lines(str(ref_sam))
    assert len(want) > 0
    assert diff_lines(SL.body_lines(str(amd_sam)), want) == 0, tag
    assert open(amd_err).read() == open(ref_err).read(), tag          # the alignment summary
    return want


@needs_ref
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("fmt", ["tab5", "tab6"])
def test_tabbed_pairs_and_unpaired_reads(tmp_path, genome, g1_index, g1s_index, fmt, graph):
    """about half pairs and half unpaired reads in random order; without spliced alignment, and in the default mode (temporary splice sites: -p 3 here is
    -p 3 --reorder there)"""
    base = g1s_index if graph else g1_index
    # (two waves of 1000 x 3 reads in the default mode; a third of the records cross one of 40 introns, so that what a read sees of the earlier reads' junctions matters)
    recs = R.make_records(genome, 601 + graph, 3000) + R.spliced_records(genome, 701 + graph, 1500)
    order = np.random.default_rng(801 + graph).permutation(len(recs))
    recs = [recs[i] for i in order]
    path = tmp_path / f"mixed.{fmt}"
    R.write_tabbed(path, recs, six=fmt == "tab6")
    npairs = sum(len(r) == 5 for r in recs)
    assert 0.4 * len(recs) < npairs < 0.6 * len(recs)
    common = ["-x", base, f"--{fmt}", path]
    want = same_output(tmp_path, "nospliced", common + ["--no-spliced-alignment"], common + ["--no-spliced-alignment", "--batch", "700"])
    assert len(want) >= len(recs) + npairs
    same_output(tmp_path, "default", common, ref_p=3, amd_p=3)


@needs_ref
def test_alternating_file_does_not_fall_apart_into_runs(tmp_path, genome, g1_index):
    """pair, unpaired read, pair, ...: N records in windows of B are at most 2 ceil(N / B) device runs"""
    a = R.make_records(genome, 611, 1500, pair_frac=1.0, name="p")
    b = R.make_records(genome, 612, 1500, pair_frac=0.0, name="u")
    recs = [x for pair in zip(a, b) for x in pair]
    path = tmp_path / "alt.tab5"
    R.write_tabbed(path, recs)
    stats = tmp_path / "stats.json"
    common = ["-x", g1_index, "--tab5", path, "--no-spliced-alignment"]
    same_output(tmp_path, "alt", common, common + ["--batch", "512", "--h2g-stats", stats])
    st = json.load(open(stats))
    n = len(recs)
    assert st["reads"] == n and st["overflow"] == 0
    assert st["runs"] <= 2 * ((n + 511) // 512), st


@needs_ref
def test_alternating_file_with_temporary_splice_sites(tmp_path, genome, g1_index):
    """the same in the default mode, where a window is a wave of 1000 x <-p> records (--batch does not apply) and every read keeps its record's id
    (h2g_set_read_ids): two runs per wave, output == hisat2 -p 3 --reorder; half of the records cross introns that other records cross too"""
    recs = R.make_records(genome, 613, 4000) + R.spliced_records(genome, 614, 4000)
    order = np.random.default_rng(615).permutation(len(recs))
    recs = [recs[i] for i in order]
    pairs, singles = [r for r in recs if len(r) == 5], [r for r in recs if len(r) == 3]
    recs = [x for pair in zip(pairs, singles) for x in pair][:7000]
    assert all((len(r) == 5) == (i % 2 == 0) for i, r in enumerate(recs)) and len(recs) == 7000
    path = tmp_path / "alt.tab6"
    R.write_tabbed(path, recs, six=True)
    stats = tmp_path / "stats.json"
    common = ["-x", g1_index, "--tab6", path]
    want = same_output(tmp_path, "alt", common, common + ["--h2g-stats", stats], ref_p=3, amd_p=3)
    assert sum("N" in l.split("\t")[5] for l in want) > 1000          # spliced alignments
    st = json.load(open(stats))
    n, wave = len(recs), 3000
    assert st["reads"] == n and st["overflow"] == 0
    assert st["runs"] <= 2 * ((n + wave - 1) // wave), st


@needs_ref
@pytest.mark.parametrize("mode", ["--no-spliced-alignment", "--no-temp-splicesite"])
def test_mates_together_with_unpaired_reads(tmp_path, genome, g1_index, mode):
    """-1/-2 with -U (two files each, the second of them gzipped here; the reference binary of oracle/_ref reads the plain files): the pairs first, then the
    unpaired reads, one summary with both blocks"""
    files = {}
    for k, (seed, n) in enumerate(((621, 900), (622, 500))):
        pairs = R.make_records(genome, seed, n, pair_frac=1.0, name=f"p{k}_")
        singles = R.make_records(genome, seed + 10, n // 2, pair_frac=0.0, name=f"u{k}_")
        for tag, reads in (("1", [(r[0], r[1], r[2]) for r in pairs]), ("2", [(r[0], r[3], r[4]) for r in pairs]), ("u", singles)):
            files[(k, tag)] = tmp_path / f"f{k}_{tag}.fq"
            R.write_fastx(files[(k, tag)], reads)
            if k:
                R.write_fastx(str(files[(k, tag)]) + ".gz", reads)
    sources = lambda gz: [x for tag, opt in (("1", "-1"), ("2", "-2"), ("u", "-U")) for x in (opt, f"{files[(0, tag)]},{files[(1, tag)]}{gz}")]
    common = ["-x", g1_index, "-q", mode]
    args = common + sources(".gz")
    want = same_output(tmp_path, "mixed", common + sources(""), args + ["--batch", "400"])
    assert len(want) >= 2 * 1400 + 700
    same_output(tmp_path, "newsumm", common + sources("") + ["--new-summary"], args + ["--new-summary"])
    if mode == "--no-temp-splicesite":
        # the default mode (temporary splice sites) is refused for this one combination, by name
        p = subprocess.run([CLI] + [str(a) for a in args if a != mode], capture_output=True, text=True)
        assert p.returncode != 0 and "-U" in p.stderr and "--no-temp-splicesite" in p.stderr and "--no-spliced-alignment" in p.stderr, p.stderr


def qseq_inputs(tmp_path, genome, seed, n, paired):
    rng = np.random.default_rng(seed)
    recs = R.make_records(genome, seed, n, pair_frac=1.0 if paired else 0.0)
    filt = ["0" if rng.random() < 0.1 else "1" for _ in range(n)], ["0" if rng.random() < 0.1 else "1" for _ in range(n)]
    out = {}
    for m in (1, 2) if paired else (1,):
        reads = [(r[1], r[2]) if m == 1 else (r[3], r[4]) for r in recs]
        out[f"q{m}"] = tmp_path / f"r_{m}_qseq.txt"
        R.write_qseq(out[f"q{m}"], reads, m, filt[m - 1])
        out[f"f{m}"] = tmp_path / f"r_{m}.fq"
        R.write_fastx(out[f"f{m}"], [(R.qseq_name(i, m), s, q) for i, (s, q) in enumerate(reads)])
    assert 0.05 * n < filt[0].count("0") < 0.2 * n
    return out


@needs_ref
@pytest.mark.parametrize("paired", [False, True])
def test_qseq_and_qc_filter(tmp_path, genome, g1_index, paired):
    """QSEQ input, a tenth of the reads with filter 0: with --qc-filter they are not aligned (YF:Z:QC; the mate of a filtered read is aligned alone), as in the
    reference; without it the output is that of the same reads, under the same names, as FASTQ"""
    f = qseq_inputs(tmp_path, genome, 631 + paired, 1500, paired)
    src = (lambda a, b: ["-1", a, "-2", b]) if paired else (lambda a, b: ["-U", a])
    common = ["-x", g1_index, "--no-spliced-alignment"]
    want = same_output(tmp_path, "qc", common + ["--qseq", "--qc-filter"] + src(f["q1"], f.get("q2")), amd_p=4)
    nqc = sum("YF:Z:QC" in l for l in want)
    assert nqc > 100
    if paired:
        # a filtered read whose mate passed and aligned on its own
        assert sum("YF:Z:QC" in l and not int(l.split("\t")[1]) & 8 for l in want) > 20
    plain = same_output(tmp_path, "noqc", common + ["--qseq"] + src(f["q1"], f.get("q2")))
    assert not any("YF:Z:QC" in l for l in plain)
    fq = tmp_path / "fq.sam"
    run_amd(common + ["-q"] + src(f["f1"], f.get("f2")), fq, tmp_path / "fq.err", check=True)
    assert diff_lines(SL.body_lines(str(fq)), plain) == 0
    assert open(tmp_path / "fq.err").read() == open(tmp_path / "noqc.amd.err").read()


def test_read_filter_through_the_c_abi(tmp_path, genome, g1_index):
    """h2g_set_read_filter + h2g_align_pairs_run with the fast pass on and off (fresh processes: the switch is read once): identical digests, reads with a zero
    byte have no alignment, their passing mates still align, and h2g_set_reads clears the bytes"""
    rng = np.random.default_rng(641)
    n = 6000
    recs = R.make_records(genome, 641, n, pair_frac=1.0, random_frac=0.05, far_frac=0.1)
    code = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
    m1 = np.array([[code[c] for c in r[1]] for r in recs], dtype=np.uint8)
    m2 = np.array([[code[c] for c in r[3]] for r in recs], dtype=np.uint8)
    p1 = (rng.random(n) >= 0.1).astype(np.uint8)
    p2 = (rng.random(n) >= 0.1).astype(np.uint8)
    npz = tmp_path / "reads.npz"
    np.savez(npz, m1=m1, m2=m2, pass1=p1, pass2=p2)
    got = {}
    for fast in ("0", "1"):
        env = dict(os.environ, H2G_GO_FAST=fast, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "qc_digest.py"), g1_index, str(npz)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got[fast] = json.loads(r.stdout.strip().splitlines()[-1])
    print(got)
    nfilt = int(((p1 == 0) | (p2 == 0)).sum())
    for tag in ("filtered", "cleared"):
        assert got["0"][tag]["fast"] == 0 and got["1"][tag]["fast"] > n // 4, got
        assert got["1"][tag]["fast"] + got["1"][tag]["handed_on"] == n
        assert got["0"][tag]["sha"] == got["1"][tag]["sha"], tag
        assert got["0"][tag]["overflow"] == 0 and got["1"][tag]["overflow"] == 0
    for fast in ("0", "1"):
        assert got[fast]["filtered"]["filtered_with_alignment"] == 0
        assert got[fast]["filtered"]["passing_mate_aligned"] > nfilt // 4
        assert got[fast]["cleared"]["filtered_with_alignment"] > nfilt // 2        # the same reads align once the bytes are gone
        assert got[fast]["filtered"]["sha"] != got[fast]["cleared"]["sha"]
    # a pair with a filtered mate is the general machine's: the fast pass hands it on
    assert got["1"]["filtered"]["fast"] <= n - nfilt and got["1"]["filtered"]["handed_on"] > got["1"]["cleared"]["handed_on"]


@needs_ref
@pytest.mark.parametrize("fmt", ["tab5", "tab6"])
def test_seed_on_tabbed_pairs(tmp_path, genome, g1_index, fmt):
    """--seed 7: a read's PRNG seed is drawn from its name as parsed — both mates of a tab5 pair hash the pair's name, tab6 mates their own; repeats make the
    choice among equal alignments depend on it"""
    recs = R.make_records(genome, 651, 1500, pair_frac=1.0, random_frac=0.05)
    rep = R.repeated_pairs(genome, 60)
    assert len(rep) >= 20
    recs += rep
    path = tmp_path / f"pairs.{fmt}"
    R.write_tabbed(path, recs, six=fmt == "tab6")
    same_output(tmp_path, "seed", ["-x", g1_index, f"--{fmt}", path, "--no-spliced-alignment", "--seed", "7", "-k", "2"])


def originals_of(fmt, recs=None, files=None):
    """the original text of every record, per mate"""
    if fmt == "tab5":
        return [("\t".join(r) + "\n",) if len(r) == 3 else ("\t".join(r) + "\n", "") for r in recs]
    texts = []
    for path in files:
        opener = gzip.open if str(path).endswith(".gz") else open
        lines = opener(path, "rt").read().split("\n")
        per = 2 if fmt == "fasta" else 4
        texts.append(["".join(l + "\n" for l in lines[i:i + per]) for i in range(0, len(lines) - 1, per)])
    return list(zip(*texts))


def check_read_files(tmp, tag, want, nreads, gz):
    """the files the command line wrote hold exactly the records the rule puts there, in order; no file is (vacuously) empty"""
    for kind in KINDS:
        for m in (0, 1):
            conc = kind not in ("un", "al")
            if not conc and m:
                continue
            fn = tmp / (f"{tag}_{kind}.{m + 1}.out" if conc else f"{tag}_{kind}.out")
            got = (gzip.open(fn, "rt") if gz else open(fn)).read()
            assert got == want[kind][m], (tag, kind, m)


def read_file_args(tmp, tag, gz):
    return [x for kind in KINDS for x in (f"--{kind}{'-gz' if gz else ''}", tmp / f"{tag}_{kind}.out")]


@needs_ref
@pytest.mark.parametrize("case", ["unpaired_fastq", "paired_fasta", "mixed_tab5"])
def test_read_files_follow_the_flag_rule(tmp_path, genome, g1_index, case):
    """--un / --al / --un-conc / --al-conc / --al-conc-disc, plain and -gz: the rule of the reference's wrapper script, applied here to the reference binary's
    SAM for the same input, names the records of every file"""
    common = ["-x", g1_index, "--no-spliced-alignment", "-k", "3"]
    if case == "unpaired_fastq":
        recs = R.make_records(genome, 661, 1200, pair_frac=0.0)
        path = tmp_path / "u.fq"
        R.write_fastx(path, recs)
        args, orig = common + ["-q", "-U", path], originals_of("fastq", files=[path])
        orig = [(t[0],) for t in orig]
        live = ("un", "al")
    elif case == "paired_fasta":
        recs = R.make_records(genome, 662, 1200, pair_frac=1.0)
        p1, p2 = tmp_path / "p_1.fa", tmp_path / "p_2.fa"
        R.write_fastx(p1, [(r[0], r[1], r[2]) for r in recs], fasta=True)
        R.write_fastx(p2, [(r[0], r[3], r[4]) for r in recs], fasta=True)
        args, orig = common + ["-f", "-1", p1, "-2", p2], originals_of("fasta", files=[p1, p2])
        live = ("un-conc", "al-conc", "al-conc-disc")
    else:
        recs = R.make_records(genome, 663, 1600)
        path = tmp_path / "m.tab5"
        R.write_tabbed(path, recs)
        args, orig = common + ["--tab5", path], originals_of("tab5", recs=recs)
        live = KINDS
    ref_sam = tmp_path / "ref.sam"
    run_ref(args, ref_sam, tmp_path / "ref.err")
    want = R.sort_by_flags(SL.body_lines(str(ref_sam)), orig)
    # not vacuous: the reference alone routes at least 5 % of the reads to every file that this kind of input can reach
    lines = [l for l in SL.body_lines(str(ref_sam)) if not int(l.split("\t")[1]) & 256]
    fl = [int(l.split("\t")[1]) for l in lines]
    count = {"un": sum(not f & 192 and f & 4 for f in fl), "al": sum(not f & 192 and not f & 4 for f in fl), "un-conc": sum(bool(f & 64) and not f & 2 for f in fl),
             "al-conc": sum(bool(f & 64) and bool(f & 2) for f in fl), "al-conc-disc": sum(bool(f & 64) and (not f & 4 or not f & 8) for f in fl)}
    for kind in live:
        assert count[kind] >= 0.05 * len(recs), (kind, count)
    for gz in (False, True):
        tag = "gz" if gz else "plain"
        amd_sam = tmp_path / f"{tag}.sam"
        run_amd(args + ["--batch", "500"] + read_file_args(tmp_path, tag, gz), amd_sam, tmp_path / f"{tag}.err", exe=FRONT, check=True)
        assert diff_lines(SL.body_lines(str(amd_sam)), SL.body_lines(str(ref_sam))) == 0
        check_read_files(tmp_path, tag, want, len(recs), gz)


@needs_ref
def test_read_files_with_no_unal(tmp_path, genome, g1_index):
    """--no-unal keeps its meaning next to the read files: the SAM is the reference's --no-unal SAM, and the files hold what the rule makes of the reference's
    full SAM (the unaligned reads are sorted although their lines are not printed), as with the reference's script, which drops the 0x4 lines itself"""
    recs = R.make_records(genome, 671, 1600)
    path = tmp_path / "m.tab5"
    R.write_tabbed(path, recs)
    args = ["-x", g1_index, "--no-spliced-alignment", "-k", "3", "--tab5", path]
    full, nounal = tmp_path / "ref_full.sam", tmp_path / "ref_nounal.sam"
    run_ref(args, full, tmp_path / "ref_full.err")
    run_ref(args + ["--no-unal"], nounal, tmp_path / "ref_nounal.err")
    want = R.sort_by_flags(SL.body_lines(str(full)), originals_of("tab5", recs=recs))
    assert want["un"][0].count("\n") >= 0.05 * len(recs) and want["un-conc"][0].count("\n") >= 0.05 * len(recs)
    assert len(SL.body_lines(str(nounal))) < len(SL.body_lines(str(full))) - 0.1 * len(recs)
    for gz in (False, True):
        tag = "gz" if gz else "plain"
        amd_sam = tmp_path / f"{tag}.sam"
        run_amd(args + ["--no-unal", "--batch", "500"] + read_file_args(tmp_path, tag, gz), amd_sam, tmp_path / f"{tag}.err", exe=FRONT, check=True)
        assert diff_lines(SL.body_lines(str(amd_sam)), SL.body_lines(str(nounal))) == 0
        assert not any(int(l.split("\t")[1]) & 4 for l in SL.body_lines(str(amd_sam)))
        assert open(tmp_path / f"{tag}.err").read() == open(tmp_path / "ref_nounal.err").read()
        check_read_files(tmp_path, tag, want, len(recs), gz)


GOLDEN_FILES = {
    "pe": (["-q", "-1", "in_1.fq", "-2", "in_2.fq"],
           {"--un": ("un.fq", ["un.fq"]), "--al": ("al.fq", ["al.fq"]), "--un-conc": ("unc.fq", ["unc.1.fq", "unc.2.fq"]), "--al-conc": ("alc_%.fq", ["alc_1.fq", "alc_2.fq"]),
            "--al-conc-disc": ("", ["al-conc-disc-mate.1", "al-conc-disc-mate.2"])}),
    "tab": (["--tab5", "in.tab5"],
            {"--un": ("un.tab5", ["un.tab5"]), "--al": ("al.tab5", ["al.tab5"]), "--un-conc": ("unc.tab5", ["unc.1.tab5", "unc.2.tab5"]),
             "--al-conc": ("alc.tab5", ["alc.1.tab5", "alc.2.tab5"]), "--al-conc-disc": ("acd", ["acd.1", "acd.2"])}),
}


@pytest.mark.parametrize("which", ["pe", "tab"])
def test_read_files_equal_the_wrapper_scripts(tmp_path, golden_dir, g1_index, which):
    """the record text and the file names: tests/golden/readsets_<which>_* hold an input and the files `hisat2 --un ... --al-conc-disc <dir>` (the reference's wrapper
    script over its hisat2-align-s, -p 1 --no-spliced-alignment) wrote for it; the command line writes the same bytes under the same names"""
    inputs, opts = GOLDEN_FILES[which]
    pre = f"readsets_{which}_"
    for fn in os.listdir(golden_dir):
        if fn.startswith(pre + "in"):
            with gzip.open(os.path.join(golden_dir, fn), "rb") as f, open(tmp_path / fn[len(pre):-3], "wb") as o:
                shutil.copyfileobj(f, o)
    args = [a if a.startswith("-") else str(tmp_path / a) for a in inputs]
    for opt, (arg, _) in opts.items():
        args += [opt, str(tmp_path / arg) if arg else str(tmp_path)]
    run_amd(["-x", g1_index, "--no-spliced-alignment"] + args, tmp_path / "out.sam", tmp_path / "err.txt", exe=FRONT, check=True)
    nrec = sum(1 for _ in open(tmp_path / inputs[-1])) // (4 if which == "pe" else 1)
    for opt, (_, names) in opts.items():
        for k, name in enumerate(names):
            want = gzip.open(os.path.join(golden_dir, pre + name + ".gz"), "rb").read()
            assert open(tmp_path / name, "rb").read() == want, (opt, name)
            # (the goldens are not vacuous: at least 5 % of the records in every file this input can reach; the second mates of a tab5 pair have no text of their own)
            reachable = not (which == "pe" and opt in ("--un", "--al")) and not (which == "tab" and k == 1)
            if reachable:
                assert want.count(b"\n") // (4 if which == "pe" else 1) >= 0.05 * nrec, (opt, name)
            else:
                assert want == b""
