// go() fast pass for SPLICED runs on a linear index: h2g_k_go_fast.hip compiled with FG_SPLICED = 1 (h2g_fast.h).  Reads whose whole trace stays unspliced
// under the spliced rules complete here; a read a splice would enter is handed on to the spliced machine units (go_run; h2g_stream_tune "fast_spliced").
#define FG_SPLICED  1
#define FG_KERNEL   k_go_fast_spl
#define FG_UNIT     h2g_go_fast_spl_unit
#include "h2g_k_go_fast.hip"
