"""GPU: --seed, --non-deterministic and --n-ceil through the command line and the C ABI.  The command line against the reference binary
(oracle/_ref/hisat2-align-s) with the same options: every SAM body line and the alignment summary byte-identical.  The genome carries families of
near-identical copies on both strands (test_gpu_large_k's builder), so most reads have several equally good placements and the seed decides the
primary; a share of the reads carries 0-40 Ns, and of the pairs one mate, the other or both.  Every --seed case also checks that the reference's own
output differs from its --seed 0 output by a stated number of lines; every --n-ceil case that the reference's YF:Z:NS count moves from the default's
by a stated number.  --non-deterministic seeds from the clock: explicit seeds equal to genRandSeed (h2g_set_read_seeds) must reproduce a hashed run
bit for bit, and the command line with a fixed H2G_ARB_SEED must repeat itself."""
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import sam_lines as SL
from hisat2_amd import api, synth
from test_gpu_large_k import CLI, REF, build, make_genome, make_pairs, make_reads, ref_run, amd_run
from test_sam_lines import diff_lines

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(not os.path.exists(os.path.join(REF, "hisat2-align-s")), reason="needs oracle/_ref")
# lines by which the reference's --seed <s> output differs from its --seed 0 output (at least)
SEED_MIN = 100   # measured 153 (graph) to 3008 (unpaired)


def _add_ns(rng, reads, frac=0.4, most=40):
    reads = reads.copy()
    for i in range(len(reads)):
        if rng.random() < frac:
            k = int(rng.integers(0, most + 1))
            reads[i, rng.choice(reads.shape[1], size=k, replace=False)] = 4
    return reads


@pytest.fixture(scope="module")
def gen(tmp_path_factory):
    t = str(tmp_path_factory.mktemp("seednceil"))
    # the spliced and graph cases read the small family: spliced pairing joins every two copies of a family, and 8 copies keep those lists within
    # what the default units hold (overflow 0)
    contigs, copies = make_genome(931, length=1_500_000, elements=(700, 1300), copies=(40, 80), small=(900, 8))
    base = build(t, contigs)
    rng = np.random.default_rng(932)
    big = [c for c in copies if c[3] < 2]
    synth.write_reads_fasta(os.path.join(t, "u.fa"), _add_ns(rng, make_reads(contigs, big, 1500, 933)))
    m1, m2 = make_pairs(contigs, big, 1000, 934)
    synth.write_reads_fasta(os.path.join(t, "p1.fa"), _add_ns(rng, m1, 0.3))
    synth.write_reads_fasta(os.path.join(t, "p2.fa"), _add_ns(rng, m2, 0.3))
    small = [c for c in copies if c[3] == 2]
    s1, s2 = make_pairs(contigs, small, 600, 935)
    synth.write_reads_fasta(os.path.join(t, "s1.fa"), _add_ns(rng, s1, 0.2))
    synth.write_reads_fasta(os.path.join(t, "s2.fa"), _add_ns(rng, s2, 0.2))
    return t, base, contigs


def _inputs(t, kind):
    if kind == "u":
        return ["-U", os.path.join(t, "u.fa")]
    if kind == "p":
        return ["-1", os.path.join(t, "p1.fa"), "-2", os.path.join(t, "p2.fa")]
    return ["-1", os.path.join(t, "s1.fa"), "-2", os.path.join(t, "s2.fa")]


def _both(t, tag, base, inputs, opts, env=None):
    rs, re_ = ref_run(t, tag, base, inputs, opts)
    want = SL.body_lines(rs)
    as_, ae, st = amd_run(t, tag, base, inputs, opts) if env is None else _amd_env(t, tag, base, inputs, opts, env)
    assert diff_lines(SL.body_lines(as_), want) == 0
    assert open(ae).read() == open(re_).read()
    assert st["overflow"] == 0, st
    return want, SL.body_lines(as_)


def _amd_env(t, tag, base, inputs, opts, env):
    import json
    sam, err, st = (os.path.join(t, tag + x) for x in (".amde.sam", ".amde.err", ".amde.json"))
    subprocess.run([CLI, "-f", "-p", "4", "-x", base, "-S", sam, "--h2g-stats", st] + inputs + list(opts), check=True, stderr=open(err, "w"),
                   timeout=1200, env=dict(os.environ, **env))
    return sam, err, json.load(open(st))


def _moved(a, b):
    return sum((Counter(a) - Counter(b)).values())


SEED_CASES = [
    ("u", ("--no-spliced-alignment",)),
    ("p", ("--no-spliced-alignment",)),
    ("s", ("--no-temp-splicesite",)),
    ("s", ()),                                   # temporary splice sites, -p 4
    ("u", ("--no-spliced-alignment", "-k", "100")),
    ("p", ("--no-spliced-alignment", "--bowtie2-dp", "2")),
]


@needs_ref
@pytest.mark.parametrize("seed", ["1", "12345", "2147483647"])
@pytest.mark.parametrize("kind", ["u", "p"])
def test_seed_fast_pass(gen, kind, seed):
    """--no-spliced-alignment: the fast pass; H2G_GO_FAST=0 (the general machine alone) prints the same"""
    t, base = gen[:2]
    opts = ["--no-spliced-alignment", "--seed", seed]
    want, got = _both(t, "sf%s%s" % (kind, seed), base, _inputs(t, kind), opts)
    _, got0 = _both(t, "sf%s%s0" % (kind, seed), base, _inputs(t, kind), opts, env={"H2G_GO_FAST": "0"})
    assert got0 == got
    w0, _ = ref_run(t, "sf%s%s.s0" % (kind, seed), base, _inputs(t, kind), ["--no-spliced-alignment", "--seed", "0"])
    n = _moved(want, SL.body_lines(w0))
    print("seed", kind, seed, "moved", n)
    assert n >= SEED_MIN, n


@needs_ref
@pytest.mark.parametrize("kind,opts", SEED_CASES[2:])
def test_seed_modes(gen, kind, opts):
    t, base = gen[:2]
    tag = "sm%s%s" % (kind, "".join(o.strip("-")[:3] for o in opts))
    want, _ = _both(t, tag, base, _inputs(t, kind), list(opts) + ["--seed", "12345"])
    w0, _ = ref_run(t, tag + ".s0", base, _inputs(t, kind), list(opts))
    n = _moved(want, SL.body_lines(w0))
    print("seed modes", tag, "moved", n)
    assert n >= SEED_MIN, n


@needs_ref
def test_seed_graph_index(gen, tmp_path):
    t0, contigs = gen[0], gen[2]
    t = str(tmp_path)
    base = build(t, contigs, snp_seed=936)
    inputs = _inputs(t0, "s")
    want, _ = _both(t, "sg", base, inputs, ["--no-spliced-alignment", "--seed", "12345"])
    w0, _ = ref_run(t, "sg.s0", base, inputs, ["--no-spliced-alignment"])
    n = _moved(want, SL.body_lines(w0))
    print("seed graph moved", n)
    assert n >= SEED_MIN, n


@needs_ref
def test_seed_zero_is_the_default(gen):
    t, base = gen[:2]
    a, ae, _ = amd_run(t, "z0", base, _inputs(t, "p"), ["--no-spliced-alignment", "--seed", "0"])
    b, be, _ = amd_run(t, "zn", base, _inputs(t, "p"), ["--no-spliced-alignment"])
    assert SL.body_lines(a) == SL.body_lines(b) and open(ae).read() == open(be).read()


def _ns_count(lines):
    return sum(1 for l in lines if "\tYF:Z:NS" in l)


# (--n-ceil, direction of the YF:Z:NS count against the default L,0,0.15: +1 more, -1 fewer)
NCEIL_CASES = [("L,0,0.05", 1), ("5", 1), ("C,0", 1), ("L,3", -1), ("S,1,2", -1), ("G,0,4", -1)]
NCEIL_MIN = 30   # measured 44 to 213 (|delta|)


@needs_ref
@pytest.mark.parametrize("kind", ["u", "p"])
@pytest.mark.parametrize("arg,sign", NCEIL_CASES)
def test_n_ceil(gen, kind, arg, sign):
    t, base = gen[:2]
    tag = "nc%s%s" % (kind, arg.replace(",", "_"))
    want, _ = _both(t, tag, base, _inputs(t, kind), ["--no-spliced-alignment", "--n-ceil", arg])
    d0, _ = ref_run(t, tag + ".d", base, _inputs(t, kind), ["--no-spliced-alignment"])
    delta = _ns_count(want) - _ns_count(SL.body_lines(d0))
    print("n-ceil", kind, arg, "NS delta", delta)
    assert delta * sign >= NCEIL_MIN, delta


@needs_ref
@pytest.mark.parametrize("arg", ["L,0,0.05", "L,3"])
def test_n_ceil_bowtie2_dp(gen, arg):
    t, base = gen[:2]
    tag = "ncdp%s" % arg.replace(",", "_")
    want, _ = _both(t, tag, base, _inputs(t, "p"), ["--no-spliced-alignment", "--bowtie2-dp", "2", "--n-ceil", arg])
    d0, _ = ref_run(t, tag + ".d", base, _inputs(t, "p"), ["--no-spliced-alignment", "--bowtie2-dp", "2"])
    assert _ns_count(want) != _ns_count(SL.body_lines(d0))


@needs_ref
@pytest.mark.parametrize("opts", [("--n-ceil", "0,0.15"), ("--n-ceil", "L,0,1,2"), ("--seed", "-1")])
def test_refusals_match_the_reference(gen, opts):
    """exit status and the first line of the message (the reference goes on with its usage text)"""
    t, base = gen[:2]
    inputs = _inputs(t, "u")
    r = subprocess.run([os.path.join(REF, "hisat2-align-s"), "-f", "-x", base, "-S", os.path.join(t, "rf.sam")] + inputs + list(opts),
                       capture_output=True, text=True, timeout=300)
    a = subprocess.run([CLI, "-f", "-x", base, "-S", os.path.join(t, "af.sam")] + inputs + list(opts), capture_output=True, text=True, timeout=300)
    assert a.returncode == r.returncode != 0
    assert a.stderr.splitlines()[0] == r.stderr.splitlines()[0], (a.stderr, r.stderr[:300])


# ---- --non-deterministic
def gen_rand_seed(codes, name, seed):
    """genRandSeed pat.h:55-91 of a FASTA read (qualities 'I')"""
    v = seed + 101
    for k in (59, 61, 67, 71, 73, 79, 83):
        v = (v * k) & 0xFFFFFFFF
    for i, c in enumerate(codes):
        v ^= (int(c) << ((i & 15) << 1)) & 0xFFFFFFFF
    for i in range(len(codes)):
        v ^= (ord("I") << ((i & 3) << 3)) & 0xFFFFFFFF
    for i, ch in enumerate(name.encode()):
        if ch == ord("/"):
            break
        v ^= (ch << ((i & 3) << 3)) & 0xFFFFFFFF
    return v


def _read_fa(path):
    names, seqs = [], []
    for l in open(path):
        l = l.rstrip("\n")
        if l.startswith(">"):
            names.append(l[1:])
        else:
            seqs.append(np.frombuffer(l.encode(), dtype=np.uint8))
    lut = np.full(256, 0, dtype=np.uint8)
    for ch, c in zip(b"ACGTN", range(5)):
        lut[ch] = c
    codes = [lut[s] for s in seqs]
    return names, codes


def _records(aln, offs):
    """the defined content of the dense records aln[0 .. offs[-1]): every field, and the edits up to nedits (the rest of the edit array is
    unspecified, and so is each edit's pad byte)"""
    out = []
    for k in range(int(offs[-1])):
        r = aln[k]
        ne = r.nedits if r.nedits <= api.MAX_EDITS else 1                   # a long record: its marker entry (h2g_align_fetch_long_edits)
        eds = tuple((e.pos, e.chr, e.qchr, e.type, e.snp) for e in r.edits[:ne])
        out.append((r.fw, r.tidx, r.toff, r.len, r.trim5, r.trim3, r.nedits, r.pad, r.score, eds))   # (pad: h2g_alnres.splicescore)
    return out


def _api_run(base, graph, names1, codes1, names2, codes2, opts, seeds):
    """one batch through the C ABI; -> the fetched rows: read / pair results (rnd_state for pairs), record offsets and the records' defined content"""
    ix = api.Index(base, device=0)
    c1 = np.concatenate(codes1).astype(np.uint8)
    o1 = np.concatenate([[0], np.cumsum([len(c) for c in codes1])]).astype(np.uint32)
    st = api.Stream(ix, max_reads=len(codes1), max_bases=int(c1.size) + 1024)
    try:
        st.set_reads(c1, o1)
        st.set_read_names(names1)
        p = st.align_params()
        rest = p.apply_options(list(opts))
        assert not rest, rest
        if names2 is not None:
            c2 = np.concatenate(codes2).astype(np.uint8)
            o2 = np.concatenate([[0], np.cumsum([len(c) for c in codes2])]).astype(np.uint32)
            st.set_mates(c2, o2, names2)
        if seeds is not None:
            st.set_read_seeds(*seeds)
        if names2 is not None:
            st.align_pairs_run(p)
            res, a1, o1_, a2, o2_ = st.align_pairs_fetch_dense()
            pr = [(tuple(r.nres), r.npairs, r.overflow, r.nrank, r.nsteps, r.depth, r.nside, r.rnd_state, r.pad,
                   bytes(r.pair_i)[:min(r.npairs, api.PAIR_CAP)], bytes(r.pair_j)[:min(r.npairs, api.PAIR_CAP)]) for r in res]
            return pr, o1_.tobytes(), o2_.tobytes(), _records(a1, o1_), _records(a2, o2_)
        st.align_run(p)
        res, aln, offs = st.align_fetch_dense()
        return res.tobytes(), offs.tobytes(), _records(aln, offs)
    finally:
        st.close()
        ix.close()


@pytest.mark.parametrize("case", ["u", "p", "graph", "spliced", "xl", "u_nofast", "p_nofast"])
def test_explicit_seeds_equal_hashed_seeds(gen, case, tmp_path, monkeypatch):
    """h2g_set_read_seeds with genRandSeed(read, s) == a hashed run with params.seed = s: every defined field of the fetched rows (rnd_state for
    pairs) and of their records.  (Edit entries past nedits are unspecified: a stream whose memory held an earlier run's rows
    may show its bytes there.)"""
    t, base, contigs = gen
    if case.endswith("nofast"):
        monkeypatch.setenv("H2G_GO_FAST", "0")
    graph = case == "graph"
    if graph:
        base = build(str(tmp_path), contigs, snp_seed=937)
    paired = case in ("p", "graph", "spliced", "p_nofast")
    f1, f2 = ("s1.fa", "s2.fa") if case in ("spliced", "graph") else ("p1.fa", "p2.fa")
    n1, c1 = _read_fa(os.path.join(t, f1 if paired else "u.fa"))
    n2, c2 = _read_fa(os.path.join(t, f2)) if paired else (None, None)
    opts = ["--spliced", "--no-temp-splicesite"] if case == "spliced" else ["--no-spliced-alignment"]
    if case == "xl":
        opts += ["-k", "100"]
    s = 12345
    hashed = _api_run(base, graph, n1, c1, n2, c2, opts + ["--seed", str(s)], None)
    seeds1 = np.array([gen_rand_seed(c, n, s) for c, n in zip(c1, n1)], dtype=np.uint32)
    seeds2 = np.array([gen_rand_seed(c, n, s) for c, n in zip(c2, n2)], dtype=np.uint32) if paired else None
    explicit = _api_run(base, graph, n1, c1, n2, c2, opts, (seeds1, seeds2))
    assert explicit == hashed
    other = _api_run(base, graph, n1, c1, n2, c2, opts, (seeds1 ^ np.uint32(0x9e3779b9), None if seeds2 is None else seeds2 ^ np.uint32(0x7f4a7c15)))
    assert other != hashed


@pytest.mark.parametrize("kind", ["u", "p"])
def test_non_deterministic_cli(gen, kind):
    t, base = gen[:2]
    opts = ["--no-spliced-alignment", "--non-deterministic"]
    a, _, _ = _amd_env(t, "nd1" + kind, base, _inputs(t, kind), opts, {"H2G_ARB_SEED": "77"})
    b, _, _ = _amd_env(t, "nd2" + kind, base, _inputs(t, kind), ["--no-spliced-alignment", "--nondeterministic", "--gpus", "1", "--batch", "300"],
                       {"H2G_ARB_SEED": "77"})
    c, _, _ = amd_run(t, "nd0" + kind, base, _inputs(t, kind), ["--no-spliced-alignment"])
    la, lb, lc = SL.body_lines(a), SL.body_lines(b), SL.body_lines(c)
    assert la == lb                                  # the same draws whatever the batching
    names = Counter((l.split("\t")[0], int(l.split("\t")[1]) & 0xC0) for l in la if not int(l.split("\t")[1]) & 0x100)
    assert set(names.values()) == {1}                # every read (mate) once as a primary line
    assert la != lc
    d, _, _ = _amd_env(t, "nd3" + kind, base, _inputs(t, kind), opts + ["-s", "100"], {"H2G_ARB_SEED": "77"})
    ld = SL.body_lines(d)
    assert set(ld) <= set(la) and len(ld) < len(la)   # -s: the skipped reads consume their draws, the others keep theirs
