// go() fast pass over a GRAPH index: h2g_k_go_fast.hip compiled with the graph form of the compact state (h2g_fast.h, FG_GRAPH = 1).
#define FG_GRAPH 1
// Capacities of the graph primitives' scratch in THIS unit: h2g_go_fast_graph_caps.h (shared with the host instantiations of tests/emul)
#include "h2g_go_fast_graph_caps.h"
#define H2G_HAPLOTYPE  0       // --haplotype runs on the graph_spl units (go_run: `spl`), never through this pass
#define H2G_INLINE_GLF         // the graph LF leaf functions inline in this unit's search loops (lease C: 75.8 -> 74.2 ms per million pairs)
#define FG_KERNEL   k_go_fast_graph
#define FG_UNIT     h2g_go_fast_graph_unit
#include "h2g_k_go_fast.hip"
