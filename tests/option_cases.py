"""One table of scoring-option cases at the edges of the fast pass's packed fields (tests only): tests/test_option_grid_cpu.py runs it on the host, tests/test_gpu_option_grid.py on
the device.

The fast pass (hisat2_amd/csrc/h2g_fast.h) keeps go()'s state in narrow fields: scores and the minimum score in 16 bits (F_SMIN16, `(score + 32768) << 16`, the
`m0 < -30000` hand-on of FPC_GO_INIT), read offsets in 8, edits in 16 each, nres / nsearched / npairs in 2 or 3.  go_plan() sends a run through it for every value of the
options below, so whether those fields hold is decided by the options.  Every case is a Case row: the reference's option list, FASTA or FASTQ, the read set, and what is
expected of the fast pass — `takes` (it completes at least `floor` of the batch itself) or `bails_whole` (it hands every unit on, for the named reason).

Read sets are pure functions of the seeds here: 101-base pairs and reads at a substitution rate of 0.03 (per case: an N rate, an indel rate, the fragment length, long
deletions), and one ragged set cut to the lengths of ragged_cases' class W (32 .. 128).  Qualities are drawn over the whole range 2 .. 40, base by base.

Floors.  `floor` (a fraction of the batch, a multiple of 0.05) is half of what the host instantiation (tests/emul, variant "") completed on the host batch of that case,
rounded down; the measured counts stand next to it as (pairs of N_HOST, reads of N_HOST).  They were measured once with measure() below and are not to be loosened: a
fast pass that takes less than half of what it took when the case was written has lost the case.

Every penalty in the table is 1 or more: what is below that is refused (tests/test_align_options_cpu.py, tests/test_gpu_option_grid.py), never run.
"""
import os
from collections import namedtuple

import numpy as np

from hisat2_amd import synth

N_HOST, N_DEVICE = 3000, 20000
HOST_GENOME = dict(lens=[400000, 150000, 60000], seed=9101, n_gaps=3, gap_len=300, repeats=40, repeat_len=500)        # 610 kbp
HOST_GRAPH = dict(lens=[400000, 150000, 60000], seed=9102, n_gaps=3, gap_len=300, repeats=20, repeat_len=500)         # + a variant about every 200 bp
DEVICE_GENOME = dict(lens=[1500000, 400000, 100000], seed=81, n_gaps=3, gap_len=300, repeats=80, repeat_len=600)      # == test_gpu_dense_lsa.py::small2
SNP_EVERY = 200
SUB = 0.03

# floors: (fraction of pairs, fraction of reads); measured: (pairs, reads) the host instantiation completed of N_HOST each
Case = namedtuple("Case", "name group opts fastq expect reason nrate indel frag ragged longdel flags device_pairs floors measured reference")


def case(name, group, opts, fastq=False, expect="takes", reason=None, nrate=0.0, indel=0.0, frag=300, ragged=False, longdel=False, flags=0, device_pairs=None, floors=(0.0, 0.0), measured=(0, 0), reference="equal"):
    """reference: what oracle/_ref/hisat2-align-s does with the case — "equal" (it runs, and the host machine must give its SAM lines), or the word for what it did instead
    (then only the fast-against-machine half of the case is kept).  flags: the overflow bits a unit may keep after the second pass (0: none).  Bit 1 says a working hit
    outgrew the 192 edits of the large-workspace units: at a minimum score near -30 000 a deletion of hundreds of bases is a candidate the reference's unbounded lists
    hold; such a read is flagged by name (n_overflow), and its lines are still compared.  device_pairs: the pairs of the device batch where N_DEVICE cannot be used: at
    these minimum scores the records beyond 32 edits of 20 000 pairs hold 1.5 million edits (measured on the host), more than one part of the stream's long-edit area
    (2^20); which record then finds no room, and is flagged for it, follows the timing of the passes, so two runs of the same batch differ.  5000 pairs fit."""
    return Case(name, group, tuple(opts.split()), fastq, expect, reason, nrate, indel, frag, ragged, longdel, flags, device_pairs or N_DEVICE, floors, measured, reference)


CASES = [
    # ---- the 16-bit score range: scores down to -29 000 are held, the guard hands on below -30 000 exactly
    case("mp300-c29000", "score16", "--mp 300,300 --score-min C,-29000", flags=1, device_pairs=5000, floors=(0.15, 0.25), measured=(1029, 1730)),
    case("c30000", "score16", "--score-min C,-30000", flags=1, device_pairs=5000, floors=(0.15, 0.25), measured=(988, 1629)),
    case("c30001", "score16", "--score-min C,-30001", flags=1, device_pairs=5000, expect="bails_whole", reason="input"),
    case("c31000", "score16", "--score-min C,-31000", flags=1, device_pairs=5000, expect="bails_whole", reason="input"),
    case("c40000-clamped", "score16", "--score-min C,40000", floors=(0.45, 0.45), measured=(2717, 2998)),       # min_score_for clamps a positive minimum to 0: exact matches only
    case("c0", "score16", "--score-min C,0", floors=(0.45, 0.45), measured=(2717, 2998)),
    # ---- the function types of --score-min
    # (every 8th read and first mate carries a deletion of 26-70 bases, which this minimum admits: records beyond 32 edits, kept in the long-edit area)
    case("l-3", "scoremin", "--score-min L,0,-3", longdel=True, floors=(0.15, 0.25), measured=(1077, 1613)),
    case("s-5-4", "scoremin", "--score-min S,-5,-4", floors=(0.20, 0.30), measured=(1344, 1960)),
    case("g-20-8", "scoremin", "--score-min G,-20,-8", floors=(0.20, 0.30), measured=(1326, 1930)),
    case("mp1-l-0.6", "scoremin", "--mp 1,1 --score-min L,0,-0.6", floors=(0.20, 0.30), measured=(1264, 1893)),  # up to 60 edits per read
    # ---- mismatch, N and gap penalties
    case("mp40-0-fastq", "penalties", "--mp 40,0", fastq=True, floors=(0.30, 0.45), measured=(1991, 2984)),     # the penalty is the quality
    case("mp1-0-fastq", "penalties", "--mp 1,0", fastq=True, floors=(0.25, 0.35), measured=(1526, 2106)),
    case("ignore-quals", "penalties", "--ignore-quals", fastq=True, floors=(0.20, 0.40), measured=(1459, 2671)),
    case("ignore-quals-mp5-3", "penalties", "--ignore-quals --mp 5,3", fastq=True, floors=(0.25, 0.35), measured=(1606, 2227)),
    case("np40", "penalties", "--np 40", nrate=0.002, floors=(0.15, 0.35), measured=(989, 2228)),
    case("np1-nceil0", "penalties", "--np 1 --n-ceil 0", nrate=0.002, floors=(0.15, 0.35), measured=(989, 2228)),
    case("nceil-half", "penalties", "--n-ceil L,0,0.5", nrate=0.02, floors=(0.00, 0.05), measured=(27, 362)),
    case("gaps1", "penalties", "--rdg 1,1 --rfg 1,1", indel=0.005, floors=(0.05, 0.25), measured=(508, 1582)),
    case("gaps40-20", "penalties", "--rdg 40,20 --rfg 40,20", indel=0.005, floors=(0.20, 0.45), measured=(1373, 2716)),
    case("ragged-mp7-1-fastq", "penalties", "--mp 7,1 --score-min L,0,-0.3", fastq=True, ragged=True, floors=(0.25, 0.40), measured=(1755, 2417)),
    # ---- soft clipping
    case("sp1", "softclip", "--sp 1", floors=(0.20, 0.40), measured=(1457, 2667)),
    case("sp40", "softclip", "--sp 40", floors=(0.25, 0.45), measured=(1515, 2775)),
    case("no-softclip", "softclip", "--no-softclip", floors=(0.25, 0.45), measured=(1515, 2775)),
    # ---- pairing and hit counts
    case("x120", "pairing", "-X 120", floors=(0.05, 0.45), measured=(300, 2710)),                            # 300-base fragments: nearly every pair fails the fragment test
    case("x100000", "pairing", "-X 100000", floors=(0.20, 0.45), measured=(1466, 2710)),
    case("k1", "pairing", "-k 1", floors=(0.20, 0.45), measured=(1466, 2709)),
    case("k5-seeds5", "pairing", "-k 5 --max-seeds 5", floors=(0.20, 0.45), measured=(1466, 2709)),
    case("k3-seeds64", "pairing", "-k 3 --max-seeds 64", floors=(0.20, 0.45), measured=(1466, 2710)),
]
BY_NAME = {c.name: c for c in CASES}
GROUPS = ("score16", "scoremin", "penalties", "softclip", "pairing")
# one case of each group also runs on the SNP graph
GRAPH_CASES = ("mp300-c29000", "l-3", "mp40-0-fastq", "sp1", "x120")
# cases whose lists outgrow the default units (--max-seeds 64 > their capacity: go_plan's big_main): the device runs them on the general machine whole, with no fast pass
# to compare (fast == 0 and handed_on == 0 with the switch on as well); the host instantiation, built with the large capacities, still checks the pass against the machine
DEVICE_MACHINE_ONLY = ("k3-seeds64",)
# the three cases the device also runs through the drain launch and with alignMate in the pass: one with qualities, one 16-bit edge, one with records beyond 32 edits
DEVICE_EXTRA_CASES = ("mp40-0-fastq", "c30000", "l-3")


def make_genome(spec):
    return synth.make_genome(list(spec["lens"]), spec["seed"], n_gaps=spec["n_gaps"], gap_len=spec["gap_len"], repeats=spec["repeats"], repeat_len=spec["repeat_len"])


def make_graph(spec):
    """-> (contigs, variants, the alternate haplotype that carries all of them)"""
    contigs = make_genome(spec)
    var = synth.make_snps(contigs, spec["seed"] + 9, every=SNP_EVERY)
    return contigs, var, synth.apply_snps(contigs, var)


def _indels(m, rate, rng):
    """one 1-3 base deletion or insertion in about rate * length of the rows of an (n, L) mate array (synth.make_pairs draws none); the row keeps its length"""
    m = m.copy()
    n, L = m.shape
    for k in np.nonzero(rng.random(n) < rate * L)[0]:
        p, ln = int(rng.integers(10, L - 10)), int(rng.integers(1, 4))
        if rng.random() < 0.5:      # bases missing from the read; the tail is filled with seeded bases
            m[k, p:L - ln] = m[k, p + ln:].copy()
            m[k, L - ln:] = rng.integers(0, 4, size=ln, dtype=np.uint8)
        else:                       # bases added to the read
            m[k, p + ln:] = m[k, p:L - ln].copy()
            m[k, p:p + ln] = rng.integers(0, 4, size=ln, dtype=np.uint8)
    return m


_SETS = {}


def read_set(c, contigs, n, seed):
    """the case's batch over `contigs` -> dict(m1, m2, reads: lists of uint8 arrays; q1, q2, qr: flat phred+33 bytes or None).  Cached by what the case asks of it."""
    key = (id(contigs), n, seed, c.nrate, c.indel, c.frag, c.ragged, c.fastq, c.longdel)
    if key in _SETS:
        return _SETS[key]
    rng = np.random.default_rng(seed + 17)
    rdlen = 128 if c.ragged else 101
    m1, m2 = synth.make_pairs(contigs, n, rdlen, seed + 1, frag_mean=c.frag, frag_sd=30, sub_rate=SUB)
    reads, _ = synth.make_reads(contigs, n, rdlen, seed + 2, sub_rate=SUB, indel_rate=c.indel, n_rate=c.nrate)
    if c.indel:
        m1, m2 = _indels(m1, c.indel, rng), _indels(m2, c.indel, rng)
    if c.longdel:
        from test_long_edits_cpu import deletion_reads
        m1, reads = m1.copy(), reads.copy()
        m1[::8] = deletion_reads(contigs, n, rdlen, seed + 3)[::8]
        reads[::8] = deletion_reads(contigs, n, rdlen, seed + 4)[::8]
    if c.nrate:
        m1 = np.where(rng.random(m1.shape) < c.nrate, np.uint8(4), m1)
        m2 = np.where(rng.random(m2.shape) < c.nrate, np.uint8(4), m2)
    m1, m2, reads = list(m1), list(m2), list(reads)
    if c.ragged:
        import ragged_cases as RC
        lengths = [x for x in RC.length_classes(16, 10, "W")["W"] if RC.FAST_MIN <= x <= RC.FAST_MAX]
        m1, m2, reads = (RC.trim_reads(x, seed + 20 + k, lengths)[0] for k, x in enumerate((m1, m2, reads)))
    out = dict(m1=m1, m2=m2, reads=reads, q1=None, q2=None, qr=None)
    if c.fastq:
        for k, s in (("q1", m1), ("q2", m2), ("qr", reads)):
            out[k] = (33 + rng.integers(2, 41, size=sum(len(r) for r in s))).astype(np.uint8)
    _SETS[key] = out
    return out


# ---- the host machine as the device runs it: the default configuration, then whatever it flagged once more through the large-workspace configuration
# (tests/emul/libh2gemu_long.so = the *_big units: 192 edits per working hit), whose results replace the flagged ones — go_run's second pass
LONG_EDITS = 192


def _long_rec_type():
    import ctypes as C
    from hisat2_amd import api

    class AlnRecLong(C.Structure):      # AlnRec (h2g_align.h) as libh2gemu_long.so lays it out
        _fields_ = [("fw", C.c_uint32), ("tidx", C.c_uint32), ("toff", C.c_uint32), ("len", C.c_uint32), ("trim5", C.c_uint32), ("trim3", C.c_uint32),
                    ("nedits", C.c_uint32), ("pad", C.c_uint32), ("score", C.c_int64), ("edits", api.Edit * LONG_EDITS)]
    return AlnRecLong


def _long_emu(base, options):
    from h2gemu_align import set_options
    from h2gemu_py import Emu
    e = Emu(base, "long")
    assert e.ghit_edits() == LONG_EDITS
    if options:
        set_options(e, 0, options)
    return e


def _flat(lst):
    from h2gemu_py import flat_reads
    return flat_reads(lst)


def _sub_quals(quals, offs, ids):
    return None if quals is None else np.concatenate([quals[offs[i]:offs[i + 1]] for i in ids])


class _Rows:
    """record rows of the first pass with the flagged units' rows replaced: rows[i * stride + k]"""
    def __init__(self, first, stride):
        self.first, self.stride, self.over = first, stride, {}

    def __getitem__(self, j):
        i, k = divmod(j, self.stride)
        o = self.over.get(i)
        return self.first[j] if o is None else o[0][o[1] * self.stride + k]


def host_reads_backend(base, reads, qnames, refnames, quals=None, options=()):
    """a fuzz_align backend -> (outs, rendered records); outs[i].overflow is what is left after the second pass"""
    import sam_util as SU
    from h2gemu_align import emu_align
    reads = [np.asarray(r, dtype=np.uint8) for r in reads]
    outs, recs = emu_align(base, reads, qnames, quals=quals, options=list(options))
    outs, rows = list(outs), _Rows(recs, SU.AL_MAX_RESULTS)
    ids = [i for i in range(len(reads)) if outs[i].overflow]
    host_reads_backend.second_pass = len(ids)
    host_reads_backend.left = lambda: sorted({o.overflow for o in outs})
    if ids:
        e = _long_emu(base, options)
        e.load_reads([reads[i] for i in ids], _sub_quals(quals, _flat(reads)[1], ids))
        o2, r2 = e.align([qnames[i] for i in ids], rec_type=_long_rec_type())
        for k, i in enumerate(ids):
            outs[i] = o2[k]
            rows.over[i] = (r2, k)
    return outs, SU.render(outs, rows, refnames, reads, qnames)


def host_pairs_backend(base, m1, m2, q1, q2, quals=None, options=()):
    """a fuzz_pairs backend -> (outs, rows of the first mates, of the second mates), stride sam_util.AL_MAX_RESULTS"""
    import fuzz_pairs as FP
    import sam_util as SU
    outs, r1, r2 = FP.emu_pairs(base, m1, m2, q1, q2, quals=quals, options=tuple(options))
    outs, r1, r2 = list(outs), _Rows(r1, SU.AL_MAX_RESULTS), _Rows(r2, SU.AL_MAX_RESULTS)
    ids = [i for i in range(len(outs)) if outs[i].overflow]
    host_pairs_backend.second_pass = len(ids)
    host_pairs_backend.left = lambda: sorted({o.overflow for o in outs})
    if ids:
        e = _long_emu(base, options)
        e.load_reads([m1[i] for i in ids], None if quals is None else _sub_quals(quals[0], _flat(m1)[1], ids))
        if quals is not None:
            e.set_mate_quals(_sub_quals(quals[1], _flat(m2)[1], ids))
        po, l1, l2 = e.align_pairs([m2[i] for i in ids], [q1[i] for i in ids], [q2[i] for i in ids], rec_type=_long_rec_type())
        for k, i in enumerate(ids):
            outs[i] = po[k]
            r1.over[i], r2.over[i] = (l1, k), (l2, k)
    return outs, r1, r2


def floor_of(completed, n):
    """half of `completed`, rounded down to 0.05 of the batch, as a fraction"""
    return int((completed / 2.0) / (0.05 * n)) * 0.05


def measure(base, contigs, names=None):
    """run the host instantiation once over every `takes` case and print the floors= / measured= to write into CASES (tests/option_cases.py as a script, see below)"""
    import fast_check as FC
    for c in CASES:
        if names and c.name not in names:
            continue
        s = read_set(c, contigs, N_HOST, HOST_GENOME["seed"])
        rp = FC.fast_check(base, s["m1"], s["m2"], quals=s["q1"], quals2=s["q2"], options=c.opts)
        rr = FC.fast_check(base, s["reads"], quals=s["qr"], options=c.opts)
        print(f'{c.name}: floors=({floor_of(rp["completed"], N_HOST):.2f}, {floor_of(rr["completed"], N_HOST):.2f}), measured=({rp["completed"]}, {rr["completed"]})  '
              f'mismatching {rp["mismatching"]} {rr["mismatching"]}  bails {rp["bails"]} {rr["bails"]}', flush=True)


if __name__ == "__main__":      # python tests/option_cases.py [case names]: needs oracle/_ref/hisat2-build-s and tests/emul built
    import subprocess
    import sys
    import tempfile
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tempfile.mkdtemp(prefix="h2optm")
    g = make_genome(HOST_GENOME)
    synth.write_fasta(os.path.join(tmp, "g.fa"), g)
    subprocess.run([os.path.join(ROOT, "oracle", "_ref", "hisat2-build-s"), "-q", os.path.join(tmp, "g.fa"), os.path.join(tmp, "g")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    measure(os.path.join(tmp, "g"), g, set(sys.argv[1:]))
