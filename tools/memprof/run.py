#!/usr/bin/env python3
"""Memory-access profile of the go() machine on the bench workload (host instantiation, default device workspace layout).
usage: run.py [nreads] [pairs]"""
import ctypes as C
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
from h2gemu_py import Emu  # noqa: E402
from hisat2_amd import synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
paired = len(sys.argv) > 2 and sys.argv[2] == "pairs"
subprocess.run(["make", "-s", "-C", HERE], check=True)
os.environ["H2GEMU_LIB"] = os.path.join(HERE, "libh2gemu_memprof.so")      # (the default units' edit capacity: sam_util.AlnRec is its record)
base, contigs = bench.build_index(os.path.join(ROOT, ".bench_cache"), 4_900_000)
e = Emu(base)
if not paired:
    reads, _ = synth.make_reads(contigs, n, 101, bench.SEED + 1000, sub_rate=0.005)
    e.load_reads(reads)
    e.align()
else:
    m1, m2 = synth.make_pairs(contigs, n, 101, bench.SEED + 2000, frag_mean=300, frag_sd=30, sub_rate=0.005)
    e.load_reads(m1)
    e.align_pairs(m2)
e.L.h2gemu_memprof_report.argtypes = [C.c_uint32]
sys.stdout.flush()
e.L.h2gemu_memprof_report(n)
e.L.mach_pctrace_close()
