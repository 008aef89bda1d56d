// h2g_emul_spl.cpp — TEST-ONLY host instantiation of the fast pass under the SPLICED rules (h2g_fast.h with FG_SPLICED = 1: the configuration of
// hisat2_amd/csrc/h2g_k_go_fast_spl.hip) next to the spliced general machine: the emulator as it is, plus the loop of h2gemu_fast_check with spliced
// alignment on and the emulator's splice-site database handed to the pass.  Compiled by tests/test_spl_fast_cpu.py with -DFG_SPLICED=1 -DFG_ALIGN_MATE=0
// and the EDITS32 defines of tests/emul/Makefile.
#if !defined(FG_SPLICED) || !FG_SPLICED
#error "compile with -DFG_SPLICED=1"
#endif
#include "../emul/h2g_emul.cpp"

// h2gemu_fast_check (fast_check_lanes) with the spliced machine, whose splice-site database the pass shares; the spliced build of the pass is for linear
// indexes.  spl_flags[i] (may be null) = 1: the MACHINE's result of read / pair i holds a record with a splice edit — computed for EVERY read, completed or not.
extern "C" void h2gemu_fast_check_spl(Emu* e, const uint8_t* codes2, const uint32_t* offs2, const char* names1, const uint32_t* noffs1, const char* names2,
                                      const uint32_t* noffs2, uint64_t* stats, uint32_t* bad_ids, uint32_t cap, uint8_t* done_flags, uint8_t* spl_flags) {
	fast_check_lanes(e, 0, !e->dg.linear, true, codes2, offs2, names1, noffs1, names2, noffs2, stats, bad_ids, cap, done_flags, spl_flags);
}
