"""The library's parser of the reference's alignment options (hisat2_amd/csrc/h2g_options.cpp: h2g_align_option_arity,
h2g_align_params_apply_options, h2g_align_params_presets) — the one copy of the rules, used by hisat2-align-amd and by
api.AlignParams.apply_options.  The expected fields are written out by hand from the reference's rules (hisat2.cpp:1500-1910,
:3903, :4078; aligner_seed_policy.cpp:30-70, :279-441).  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hisat2_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "hisat2_amd", "hisat2-align-amd")
F = lambda x: float(np.float32(x))
IMAX = 2 ** 31 - 1

# what a command line without alignment options runs with on a linear index (hisat2.cpp:336-345, :440, :490-521; aligner_seed_policy.cpp:294)
DEFAULTS = dict(
    khits=5, kseeds=10, no_spliced_alignment=0, secondary=0, bowtie2_dp=0, mm_max=6, mm_min=2, n_pen=1, rdg_const=5, rdg_linear=3, rfg_const=5,
    rfg_linear=3, sc_max=2, sc_min=1, score_min_type=2, score_min_const=0.0, score_min_coeff=F(-0.2), no_temp_splicesite=0, min_intronlen=20,
    max_intronlen=500000, pen_cansplice=0, pen_noncansplice=12, pen_canintronlen_type=4, pen_noncanintronlen_type=4, first_read_id=0,
    pen_canintronlen_const=-8.0, pen_canintronlen_coeff=1.0, pen_noncanintronlen_const=-8.0, pen_noncanintronlen_coeff=1.0, min_anchor_len=7,
    min_anchor_len_noncan=14, xs_only=0, use_haplotype=0, max_alts_tried=16, max_frag_len=1000, min_frag_len=0, pe_orientation=0, nofw=0, norc=0,
    avoid_pseudogene=0, transcriptome_mapping_only=0, no_anchorstop=0, pen_conflictsplice=1000000, seed=0, n_ceil_type=2, n_ceil_const=0.0,
    n_ceil_coeff=F(0.15))
GRAPH = dict(khits=10, kseeds=20)
SENS = dict(bowtie2_dp=1, score_min_type=2, score_min_const=0.0, score_min_coeff=F(-0.5))
VERY = dict(bowtie2_dp=2, score_min_type=2, score_min_const=0.0, score_min_coeff=F(-1.0), khits=30, kseeds=60)
DTA = dict(min_anchor_len=15, min_anchor_len_noncan=20, pen_noncanintronlen_type=4, pen_noncanintronlen_const=-8.0, pen_noncanintronlen_coeff=2.0)

# (options, linear index?, the fields that differ from DEFAULTS)
CASES = [
    ("", True, {}),
    ("", False, GRAPH),
    # -k, --max-seeds and the presets (resolved after every option was read; the index type decides the default -k)
    ("-k 3", True, dict(khits=3, kseeds=6)),
    ("-k 1", False, dict(khits=1, kseeds=5)),
    ("-k 3 --max-seeds 40", True, dict(khits=3, kseeds=40)),
    ("--max-seeds 7", False, dict(khits=10, kseeds=7)),
    ("-k 128 --max-seeds 256", True, dict(khits=128, kseeds=256)),
    ("-k 7x", True, dict(khits=7, kseeds=14)),
    ("--sensitive", True, SENS),
    ("--sensitive", False, dict(SENS, **GRAPH)),
    ("-k 3 --sensitive", True, dict(SENS, khits=10, kseeds=20)),
    ("--sensitive -k 12", True, dict(SENS, khits=12, kseeds=24)),
    ("-k 3 --very-sensitive", True, VERY),
    ("--very-sensitive", True, VERY),
    ("--very-sensitive --max-seeds 33", False, dict(VERY, kseeds=33)),
    ("--very-sensitive --sensitive", True, SENS),
    ("--bowtie2-dp 2 --sensitive", True, dict(SENS, bowtie2_dp=2)),
    ("--bowtie2-dp 1", True, dict(bowtie2_dp=1)),
    # --score-min: the type from the first letter, the terms not given are zero; a preset's wins whatever the order
    ("--score-min C,-18", True, dict(score_min_type=1, score_min_const=-18.0, score_min_coeff=0.0)),
    ("--score-min Linear,0,-0.2", True, dict(score_min_coeff=-0.2)),
    ("--score-min S", True, dict(score_min_type=3, score_min_coeff=0.0)),
    ("--score-min G,1,2.5", True, dict(score_min_type=4, score_min_const=1.0, score_min_coeff=2.5)),
    ("--score-min L,1,-0.3 --sensitive", True, SENS),
    ("--sensitive --score-min C,-18", True, SENS),
    # scoring scheme: atoi of each number, a second number only when given
    ("--mp 4,1", True, dict(mm_max=4, mm_min=1)),
    ("--mp 3", True, dict(mm_max=3)),
    ("--mp 5x,1", True, dict(mm_max=5, mm_min=1)),
    ("--ignore-quals", True, dict(mm_min=6)),
    ("--ignore-quals --mp 4,1", True, dict(mm_max=4, mm_min=1)),
    ("--mp 4,1 --ignore-quals", True, dict(mm_max=4, mm_min=1)),
    ("--sp 3,0", True, dict(sc_max=3, sc_min=3)),
    ("--no-softclip", True, dict(sc_max=IMAX, sc_min=IMAX)),
    ("--np 2x", True, dict(n_pen=2)),
    ("--rdg 4,2 --rfg 6,1", True, dict(rdg_const=4, rdg_linear=2, rfg_const=6, rfg_linear=1)),
    ("--rdg 8 --rfg 9", True, dict(rdg_const=8, rfg_const=9)),
    ("--secondary", True, dict(secondary=1)),
    # --n-ceil: one token x is C,x; the type by name; the terms not given keep their value
    ("--n-ceil 5", True, dict(n_ceil_type=1, n_ceil_const=5.0)),
    ("--n-ceil L,3", True, dict(n_ceil_const=3.0)),
    ("--n-ceil S,1,2", True, dict(n_ceil_type=3, n_ceil_const=1.0, n_ceil_coeff=2.0)),
    ("--n-ceil Log,0,4", True, dict(n_ceil_type=4, n_ceil_coeff=4.0)),
    ("--n-ceil Constant,2x", True, dict(n_ceil_type=1, n_ceil_const=2.0)),
    ("--n-ceil Sqrt,,7", True, dict(n_ceil_type=3, n_ceil_const=7.0)),
    # splice scoring
    ("--min-intronlen 50 --max-intronlen 1000", True, dict(min_intronlen=50, max_intronlen=1000)),
    ("--pen-cansplice 3 --pen-noncansplice 20 --pen-conflictsplice 0", True, dict(pen_cansplice=3, pen_noncansplice=20, pen_conflictsplice=0)),
    ("--pen-canintronlen S", True, dict(pen_canintronlen_type=3)),
    ("--pen-intronlen L,-1", True, dict(pen_canintronlen_type=2, pen_canintronlen_const=-1.0)),
    ("--pen-noncanintronlen C,5,0.5", True, dict(pen_noncanintronlen_type=1, pen_noncanintronlen_const=5.0, pen_noncanintronlen_coeff=0.5)),
    # --dta is applied after every option was read
    ("--dta", True, DTA),
    ("--downstream-transcriptome-assembly", False, dict(DTA, **GRAPH)),
    ("--dta --pen-noncanintronlen C,1,1", True, DTA),
    ("--dta-cufflinks", True, dict(DTA, xs_only=1)),
    # modes and the transcriptome policy
    ("--no-spliced-alignment", True, dict(no_spliced_alignment=1)),
    ("--no-temp-splicesite", True, dict(no_temp_splicesite=1)),
    ("--avoid-pseudogene --tmo --no-anchorstop", True, dict(avoid_pseudogene=1, transcriptome_mapping_only=1, no_anchorstop=1)),
    ("--transcriptome-mapping-only", True, dict(transcriptome_mapping_only=1)),
    ("--splicesite-db-only", True, {}),
    ("--haplotype --max-altstried 8", False, dict(GRAPH, use_haplotype=1, max_alts_tried=8)),
    # pairs and strands
    ("-X 500 -I 10", True, dict(max_frag_len=500, min_frag_len=10)),
    ("--maxins 300 --minins 5", True, dict(max_frag_len=300, min_frag_len=5)),
    ("--rf", True, dict(pe_orientation=1)),
    ("--ff", True, dict(pe_orientation=2)),
    ("--ff --fr", True, {}),
    ("--nofw", True, dict(nofw=1)),
    ("--norc", True, dict(norc=1)),
    ("--seed 12345", True, dict(seed=12345)),
    ("--seed 2147483647", True, dict(seed=2147483647)),
    ("-k 2 --mp 4,2 --no-softclip --score-min L,0,-0.6 --n-ceil L,0,0.5 --no-temp-splicesite --pen-canintronlen G,-9 --dta --rf --seed 7", False,
     dict(DTA, khits=2, kseeds=5, mm_max=4, sc_max=IMAX, sc_min=IMAX, score_min_coeff=-0.6, n_ceil_coeff=0.5, no_temp_splicesite=1,
          pen_canintronlen_const=-9.0, pe_orientation=1, seed=7)),
]

# every refusal of the command line, with its text
REFUSALS = [
    ("-k 0", "-k arg must be at least 1"),
    ("--min-intronlen 19", "--min-intronlen arg must be at least 20"),
    ("--max-intronlen 19", "--max-intronlen arg must be at least 20"),
    ("--pen-cansplice -1", "--pen-cansplice arg must be at least 0"),
    ("--pen-noncansplice -1", "--pen-noncansplice arg must be at least 0"),
    ("--pen-conflictsplice -1", "--pen-conflictsplice arg must be at least 0"),
    ("--max-altstried 7", "--max-altstried arg must be at least 8"),
    ("-X 0", "-X arg must be at least 1"),
    ("--maxins 0", "-X arg must be at least 1"),
    ("-I -1", "-I arg must be positive"),
    ("--seed -1", "--seed arg must be at least 0"),
    ("--seed 2147483648", "--seed arg must be at least 0"),
    ("--seed 3000000000", "--seed arg must be at least 0"),
    ("--n-ceil 0,0.15", "Error: Bad function type '0'.  Should be C (constant), L (linear), S (square root) or G (natural log)."),
    ("--n-ceil L,0,1,2", "Error: expected 3 or fewer comma-separated arguments to --n-ceil option, got 4"),
    ("--n-ceil ,,", "Error: expected at least one argument to --n-ceil option"),
    ("--score-min X,1", "Error: bad function type in --score-min X,1"),
    ("--pen-canintronlen x,1", "Error: bad function type in --pen-canintronlen x,1"),
    ("--pen-noncanintronlen 3", "Error: bad function type in --pen-noncanintronlen 3"),
]
SCORING_REFUSALS = [
    # penalties go() divides by: the soft-clipping minimum (aligner_seed_policy.cpp:446) and the mismatch maximum (:411, checked where --mp is read: the
    # reference's line ends without its bracket)
    ("--sp 0", "min (0) should be greater than 0"),
    ("--sp 0,0", "min (0) should be greater than 0"),
    ("--sp -2,5", "min (-2) should be greater than 0"),
    ("--mp 0", "Error: Maximum mismatch penalty (0) is less than minimum penalty (2"),
    ("--mp 1", "Error: Maximum mismatch penalty (1) is less than minimum penalty (2"),
    ("--mp 1,3", "Error: Maximum mismatch penalty (1) is less than minimum penalty (3"),
    ("--ignore-quals --mp 1,3", "Error: Maximum mismatch penalty (1) is less than minimum penalty (3"),
    ("--mp 1,3 --ignore-quals", "Error: Maximum mismatch penalty (1) is less than minimum penalty (3"),
    # values the reference itself dies of (--mp 0,0: SIGFPE) or hangs on (a gap extension of 0 never ends Scoring::maxReadGaps): refusals of our own
    ("--mp 0,0", "--mp: the maximum mismatch penalty must be at least 1 (got 0)"),
    ("--mp -1,-3", "--mp: the maximum mismatch penalty must be at least 1 (got -1)"),
    ("--rdg 0,0", "--rdg: the gap extension penalty must be at least 1 (got 0)"),
    ("--rdg 5,0", "--rdg: the gap extension penalty must be at least 1 (got 0)"),
    ("--rfg 5,0", "--rfg: the gap extension penalty must be at least 1 (got 0)"),
    ("--rfg 2,-1", "--rfg: the gap extension penalty must be at least 1 (got -1)"),
]
REFUSALS += SCORING_REFUSALS
# the rows above whose text is our own: the reference gives no first line to equal (it crashes or hangs)
OWN_REFUSALS = {"--mp 0,0", "--mp -1,-3", "--rdg 0,0", "--rdg 5,0", "--rfg 5,0", "--rfg 2,-1"}
REF_ALIGN = os.path.join(ROOT, "oracle", "_ref", "hisat2-align-s")

ARITY = {"-k": 1, "--max-seeds": 1, "--secondary": 0, "--mp": 1, "--sp": 1, "--no-softclip": 0, "--np": 1, "--rdg": 1, "--rfg": 1, "--score-min": 1,
         "--n-ceil": 1, "--min-intronlen": 1, "--max-intronlen": 1, "--pen-cansplice": 1, "--pen-noncansplice": 1, "--pen-conflictsplice": 1,
         "--pen-canintronlen": 1, "--pen-intronlen": 1, "--pen-noncanintronlen": 1, "--sensitive": 0, "--very-sensitive": 0,
         "--no-spliced-alignment": 0, "--no-temp-splicesite": 0, "--bowtie2-dp": 1, "--dta": 0, "--downstream-transcriptome-assembly": 0,
         "--dta-cufflinks": 0, "--avoid-pseudogene": 0, "--tmo": 0, "--transcriptome-mapping-only": 0, "--no-anchorstop": 0,
         "--splicesite-db-only": 0, "--haplotype": 0, "--max-altstried": 1, "-X": 1, "--maxins": 1, "-I": 1, "--minins": 1, "--fr": 0, "--rf": 0,
         "--ff": 0, "--nofw": 0, "--norc": 0, "--ignore-quals": 0, "--seed": 1,
         "-x": -1, "-U": -1, "--rg-id": -1, "--non-deterministic": -1, "--nondeterministic": -1, "--bogus": -1, "": -1, "--spliced": -1, "--MP": -1}


def command_line_block():
    """the block hisat2-align-amd starts from: the library's defaults, spliced alignment on"""
    p = api.AlignParams()
    api.lib().h2g_align_params_init(C.byref(p), None)
    p.no_spliced_alignment = 0
    return p


def fields(p):
    return {n: getattr(p, n) for n, _ in api.AlignParams._fields_}


def test_the_table_covers_every_option():
    assert len(CASES) >= 40
    used = {o for line, _, _ in CASES for o in line.split() if o in ARITY}
    assert used == {o for o, a in ARITY.items() if a >= 0}


def test_defaults():
    assert fields(command_line_block()) == DEFAULTS


@pytest.mark.parametrize("line,linear,diff", CASES, ids=[f"{c[0] or 'none'}-{'linear' if c[1] else 'graph'}" for c in CASES])
def test_options(line, linear, diff):
    p = command_line_block()
    assert p.apply_options(line.split(), linear=linear) == []
    assert fields(p) == dict(DEFAULTS, **diff)


def test_the_block_says_which_index_when_linear_is_not_given():
    """apply_options' default: a block whose -k is 5 came from a linear index"""
    p = command_line_block()
    p.apply_options(["--sensitive"])
    assert (p.khits, p.kseeds) == (5, 10)
    p = command_line_block()
    p.khits, p.kseeds = 10, 20
    p.apply_options([])
    assert (p.khits, p.kseeds) == (10, 20)


def test_leftovers_and_output_options():
    """options of the SAM text are skipped with their arguments, --spliced is the tests' shorthand, the rest comes back"""
    p = command_line_block()
    p.no_spliced_alignment = 1
    rest = p.apply_options(["--rg-id", "g1", "--rg", "SM:x", "-k", "2", "--spliced", "--rna-strandness", "FR", "--no-sq", "--novel-splicesite-outfile", "f",
                            "--summary-file", "s", "--omit-sec-seq", "--new-summary", "--add-chrname", "--remove-chrname", "--no-mixed", "--no-discordant",
                            "--no-templatelen-adjustment", "--known-splicesite-infile", "ss.txt", "--bogus"], linear=True)
    assert rest == ["--known-splicesite-infile", "ss.txt", "--bogus"]
    assert fields(p) == dict(DEFAULTS, khits=2, kseeds=5)


@pytest.mark.parametrize("line,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(line, msg):
    with pytest.raises(ValueError) as e:
        command_line_block().apply_options(line.split(), linear=True)
    assert str(e.value) == msg


def test_an_option_without_its_argument_is_refused():
    with pytest.raises(ValueError) as e:
        command_line_block().apply_options(["--secondary", "--mp"], linear=True)
    assert str(e.value) == "option --mp needs an argument"


def test_arity():
    L = api.lib()
    for name, want in ARITY.items():
        assert L.h2g_align_option_arity(name.encode()) == want, name
    assert L.h2g_align_option_arity(None) == -1


@pytest.mark.skipif(not os.path.exists(CLI), reason="hisat2-align-amd not built")
@pytest.mark.parametrize("line,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_command_line_refuses_before_it_needs_a_device(tmp_path, line, msg):
    """the same refusals through hisat2-align-amd: found before the index (here: none) or a device is touched"""
    r = tmp_path / "r.fa"
    r.write_text(">0\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    p = subprocess.run([CLI, "-f", "-x", str(tmp_path / "no_such_index"), "-U", str(r)] + line.split() + ["-S", str(tmp_path / "o.sam")],
                       capture_output=True, text=True)
    assert p.returncode == 1
    assert p.stderr.splitlines()[0] == msg


@pytest.mark.skipif(not os.path.exists(REF_ALIGN), reason="needs oracle/_ref")
@pytest.mark.parametrize("line,msg", [r for r in SCORING_REFUSALS if r[0] not in OWN_REFUSALS], ids=[r[0] for r in SCORING_REFUSALS if r[0] not in OWN_REFUSALS])
def test_scoring_refusals_are_the_reference_binarys(tmp_path, line, msg):
    """the text of the scoring refusals is the live reference's first stderr line, and it exits with 1 as well (it reads its options before it looks for the index)"""
    r = tmp_path / "r.fa"
    r.write_text(">0\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    p = subprocess.run([REF_ALIGN, "-f", "-x", str(tmp_path / "no_such_index"), "-U", str(r)] + line.split() + ["-S", str(tmp_path / "o.sam")],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 1
    assert p.stderr.splitlines()[0] == msg


def test_a_block_that_cannot_run_is_not_mended_by_the_parser():
    """the refusals look at what an option leaves behind: --ignore-quals alone sets mm_min = mm_max and passes; a --mp that leaves the block's minimum above its maximum does not"""
    p = command_line_block()
    p.mm_min = 5
    with pytest.raises(ValueError) as e:
        p.apply_options(["--mp", "4"], linear=True)
    assert str(e.value) == "Error: Maximum mismatch penalty (4) is less than minimum penalty (5"
    p = command_line_block()
    assert p.apply_options(["--ignore-quals", "--mp", "1,1", "--sp", "1", "--rdg", "0,1", "--rfg", "0,1"], linear=True) == []
    assert (p.mm_max, p.mm_min, p.sc_min, p.sc_max, p.rdg_linear, p.rfg_linear) == (1, 1, 1, 1, 1, 1)
