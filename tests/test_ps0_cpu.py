"""The fast pass's first partial searches from a table (hisat2_amd/csrc/h2g_fast.h fg_ps0_*, FPC_NB_PICK; the device writes the table in h2g_k_ps0.hip) on the
host: tests/ps0/ps0_check.cpp, a stand-alone program built with AddressSanitizer and UBSan, over the golden linear index.  (a) For every golden read and the
edge reads (lengths 0, 1, ftabChars, ftabChars + 1, ftabChars + 2, 30, 101, H2G_PK_MAXLEN, H2G_PK_MAXLEN + 1; an N inside and beyond the first ftabChars bases),
both strands, the packed record unpacks to the words FPC_NB_AFTER_PS consumes.  (b) Host lanes (fast_run_single) with a host-built table and with a null
pointer end in byte-identical state, word store, outputs and work counters — reads and pairs, unequal and empty mates included."""
import os
import subprocess

import numpy as np

import parity_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ps0", "ps0_check.cpp")


def test_table_path_equals_request_path(g1_index, golden_dir, tmp_path):
    exe = str(tmp_path / "ps0_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DH2G_GHIT_EDITS=32",
                    "-DH2G_NEW_EDITS=24", "-DFG_ALIGN_MATE=0", "-o", exe, SRC], check=True)
    reads, offs = PC.load_reads(golden_dir)
    rb = str(tmp_path / "reads.bin")
    with open(rb, "wb") as f:
        f.write(np.uint32(len(offs) - 1).tobytes()); f.write(offs.astype("<u4").tobytes()); f.write(np.ascontiguousarray(reads, dtype=np.uint8).tobytes())
    r = subprocess.run([exe, g1_index, rb], capture_output=True, text=True, timeout=600)
    print(r.stdout); print(r.stderr[-4000:])
    assert r.returncode == 0
    assert "ps0_check ok" in r.stdout
