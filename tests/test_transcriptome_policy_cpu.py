"""CPU: --avoid-pseudogene and --tmo through the host instantiation of the go() machine (tests/emul: the code of the spliced units) against
the reference binary, on the genes-and-processed-pseudogenes genome of tests/test_gpu_transcriptome_policy.py with a
--known-splicesite-infile: every read's SAM fields equal.  Records carry their transcript class above the strand under these options
(H2G_FW_TCLASS, include/h2g.h); the Python renderer reads fw as the strand, so the class bits are masked before rendering."""
import os
import subprocess

import pytest

import sam_util as SU
from h2gemu_align import emu_align
from hisat2_amd import synth
import test_gpu_transcriptome_policy as T

needs_ref = pytest.mark.skipif(not os.path.exists(os.path.join(T.REF, "hisat2-align-s")), reason="needs oracle/_ref")


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    t = str(tmp_path_factory.mktemp("tpcpu"))
    contigs, genes, introns = T.make_genome(501)
    base = T.build(t, contigs)
    ss, _ = T.write_annotation(t, genes, introns)
    reads = T.make_reads(contigs, genes, 800, 502)
    rfa = os.path.join(t, "r.fa")
    synth.write_reads_fasta(rfa, reads)
    return t, base, ss, [(0, a - 1, b, "+") for a, b in introns], rfa, reads


@needs_ref
@pytest.mark.parametrize("opts", [["--avoid-pseudogene"], ["--avoid-pseudogene", "-k", "1"], ["--tmo"]])
def test_policy_equals_the_reference_on_the_host(case, opts):
    t, base, ss, sites, rfa, reads = case
    sam = os.path.join(t, "ref.sam")
    subprocess.run([os.path.join(T.REF, "hisat2-align-s"), "-f", "-p", "1", "--no-temp-splicesite", "-x", base, "-U", rfa, "-S", sam,
                    "--known-splicesite-infile", ss] + opts, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    refnames, want = SU.parse_sam(sam)
    qn = [str(i) for i in range(len(reads))]
    rl = [reads[i] for i in range(len(reads))]
    outs, recs = emu_align(base, rl, qn, no_spliced=0, options=opts, splice_sites=sites)
    assert any(r.fw & 2 for r in recs)                  # the class rides in fw under the policy
    for r in recs:
        r.fw &= 1
    got = SU.render(outs, recs, refnames, rl, qn)
    assert [q for q in qn if got[q] != want[q]] == []
