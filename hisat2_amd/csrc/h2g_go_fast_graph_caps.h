// Capacities of the graph primitives' scratch in the graph fast pass's unit (h2g_k_go_fast_graph.hip; h2g_graph.h, include/h2g.h; the general machine's units keep
// theirs).  A header of its own so that a host instantiation of this unit (tests/emul: libh2gemu_gfast.so, h2g_caps_check) cannot drift from the kernel's.  A hit of
// the fast path holds four edits and a resolution five coordinates, every capacity hit is flagged by the primitive and the read handed on: smaller lists change which
// reads the pass completes, never what it writes.
#define H2G_GHIT_EDITS 12
#define H2G_IEDGE_CAP  4       // a read of this pass keeps in-edge lists of at most two entries (fg_ie_pack); a longer one is counted, not stored
#define H2G_NEW_EDITS  8
#define H2G_GW_MAXELT  8
#define H2G_GW_MAXST   12
#define H2G_GW_MAXROWS 64      // fixed: the row masks of the group walk are 64-bit words
#define H2G_AWA_CAND   4
#define H2G_AWA_DEPTH  12
