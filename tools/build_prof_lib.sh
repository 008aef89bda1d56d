#!/bin/bash
# the library with the wave-level time split compiled in (-DH2G_GO_PROF): hisat2_amd/csrc/obj_prof/libh2g_prof.so, loaded through H2G_LIB (never the shipped library).
# The Makefile's units and flags (the fast units' -O2 included), in an object directory of its own.
set -e
cd "$(dirname "$0")/../hisat2_amd/csrc"
make GOPROF=-DH2G_GO_PROF OBJDIR="$PWD/obj_prof" OUT="$PWD/obj_prof/libh2g_prof.so" "$PWD/obj_prof/libh2g_prof.so"
ls -la obj_prof/libh2g_prof.so
