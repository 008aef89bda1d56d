// go() kernel for LINEAR indexes with the extra-large workspace (see h2g_go_xl.h).
#include "h2g_go_xl.h"
#define H2G_SPLICE_DB 1   // spliced alignment: the machine with the splice-site database joins
#define H2G_HAPLOTYPE 0    // haplotypes belong to graph indexes
#include "h2g_go_kernels.h"
H2G_GO_UNIT(linear_spl_xl, false, 2, 9)
