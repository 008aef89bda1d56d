"""CPU: FASTQ records parsed on the device, the parts that need none.  The record arithmetic of csrc/h2g_fastq.h driven lane by lane against the host parser under the
host sanitizers (tests/fastq/fq_check.cpp); the command-line fixtures of tests/test_gpu_fastq.py are all plain; what --h2g-device-parse is refused with; the new
structs and exports against the header."""
import ctypes as C
import os
import re
import subprocess

import pytest

import fastq_cases as F
import readsets_util as R
from hisat2_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "hisat2_amd", "hisat2-align-amd")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fq") / "fq_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "fastq", "fq_check.cpp"), "-lz"], check=True)
    return exe


def test_record_arithmetic_under_sanitizers(checker):
    """plain texts equal Reader::parse_record byte for byte (ragged lengths, CRLF, no last newline, trims, phred64, max_records); one record of each not-plain kind
    is flagged at its index: clean under ASan + UBSan"""
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]


def test_the_command_line_fixtures_are_all_plain(checker, golden_dir, tmp_path):
    """so that tests/test_gpu_fastq.py may ask for host_parsed == 0"""
    files = F.cli_fixtures(R.load_genome(golden_dir), tmp_path)
    paths = [p for k, p in sorted(files.items()) if not k.endswith("_64")]     # (Phred+64 or not is the same to the predicate without --phred64; counted below with it ...)
    r = subprocess.run([checker] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    counts = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^plain (\S+) (\d+) (\d+)$", r.stdout, re.M)}
    assert len(counts) == len(paths)
    for p in paths:
        plain, n = counts[p]
        assert plain == n and n in (777, 1223, 2000), (p, plain, n)
    # ... and every quality character of the Phred+64 files is at least 64
    for k in ("m1_64", "m2_64", "u_64"):
        lines = open(files[k]).read().split("\n")
        assert min(min(map(ord, q)) for q in lines[3::4] if q) >= 64


REFUSED = [("-f", ["-f"]), ("-F", ["-F", "30,10"]), ("-r", ["-r"]), ("-c", ["-c"]), ("--tab5", ["--tab5", "x.tab5"]), ("--tab6", ["--tab6", "x.tab6"]), ("--12", ["--12", "x.tab5"]),
           ("--qseq", ["--qseq"]), ("--int-quals", ["--int-quals"]), ("--solexa-quals", ["--solexa-quals"]), ("--un", ["--un", "u.fq"]), ("--al-gz", ["--al-gz", "a.fq.gz"]),
           ("--un-conc", ["--un-conc", "u.fq"]), ("--al-conc", ["--al-conc", "a.fq"]), ("--al-conc-disc", ["--al-conc-disc", "a.fq"]), ("--parse-only", ["--parse-only"])]


@pytest.mark.parametrize("name,extra", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_together_with(name, extra):
    """by name, before any device or index is touched (-x unused)"""
    for files in (["-U", "r.fq"], ["-1", "a.fq", "-2", "b.fq"]):
        for args in (["--h2g-device-parse"] + extra, extra + ["--h2g-device-parse"], ["--wrapper", "basic-0", "--h2g-device-parse"] + extra):
            p = subprocess.run([CLI, "-x", "unused"] + files + args, capture_output=True, text=True)
            assert p.returncode == 1 and "--h2g-device-parse is not built together with" in p.stderr and name in p.stderr, (args, p.stderr)
            assert p.stdout == ""


def test_structs_and_exports_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "h2g.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(h2g_fastq_opts), sizeof(h2g_fastq_result), sizeof(h2g_fastq_stats)); return 0; }\n')
    exe = str(tmp_path / "sz")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    sizes = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(api.FastqOpts), C.sizeof(api.FastqResult), C.sizeof(api.FastqStats)] == [24, 80, 24]
    header = open(os.path.join(ROOT, "include", "h2g.h")).read()
    declared = set(re.findall(r"\b(h2g_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(api.EXPORTS)
    for name in ("h2g_set_reads_fastq", "h2g_fetch_read_set", "h2g_get_fastq_stats"):
        assert name in api.EXPORTS
