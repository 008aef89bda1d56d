// go() kernel for GRAPH (SNP) indexes with the extra-large workspace (see h2g_go_xl.h).
#include "h2g_go_xl.h"
#define H2G_SPLICE_DB 1   // spliced alignment: the machine with the splice-site database joins
#include "h2g_go_kernels.h"
H2G_GO_UNIT(graph_spl_xl, true, 2, 11)
