// go() kernel for GRAPH (SNP) indexes with the extra-large workspace (see h2g_go_xl.h).
#include "h2g_go_xl.h"
#define H2G_SPLICE_DB 0   // unspliced kernels: no splice-site database joins (h2g_machine.h)
#include "h2g_go_kernels.h"
H2G_GO_UNIT(graph_xl, true, 2, 10)
