// capacities of the *_xl go() units: option sets beyond the large workspace (h2g_go_big.h), -k 33..128 and --max-seeds 65..256.  A run that asks
// for more than the large units hold runs here whole: no fast pass, no second pass (go_run).  Selection past H2G_SELECT_CAP and the concordant
// lists past AL_MAX_PAIRS live in the workspace with 16-bit indexes (H2G_XL, h2g_align.h); a list PairOut cannot carry leaves through the
// stream's side area (XlPairs) and reaches the compact paired fetch as a trailer (include/h2g.h).
#pragma once
#define H2G_XL 1
#ifndef H2G_GHIT_EDITS
#define H2G_GHIT_EDITS 192
#endif
#ifndef H2G_NEW_EDITS
#define H2G_NEW_EDITS 160
#endif
// A slot of these units is 18.7 MB (linear; the graph units add a 52 KB GraphSlot), most of it the searched and reported lists of the two mates.
// 128 reads in flight per workgroup of 256 threads, at most 12 workgroups (go_run): 1536 slots, 29 GB of workspace.
#ifndef H2G_GO_THREADS
#define H2G_GO_THREADS 256
#endif
#ifndef H2G_GO_SLOTS
#define H2G_GO_SLOTS 128
#endif
#define AL_MAX_GHITS     256     // max(khits, kseeds) <= 256
#define AL_MAX_SEARCHED  2048    // a read of a 200-copy family at -k 100 searches more than 1024 hits
#define AL_MAX_RESULTS   1024    // a mate's report list: 2 k + 4 rows that grow on demand (aln_sink.h:2565); more than 512 on a 200-copy family
#define AL_MAX_DEPTH     128
#define AL_MAX_LOCALHITS 8
#define AL_MAX_COORDS    24
#define AL_MAX_PARTIAL   64
#define AL_WS_PAIRS      4096    // concordant pairs kept per pair (the reference keeps every one: aln_sink.cpp:74-112; spliced pairing
                                 // joins the copies of a family within --max-intronlen: hundreds to thousands)
// graph walk / ALT extension scratch (h2g_graph.h), as the large units
#define H2G_GW_MAXELT    96
#define H2G_GW_MAXST     160
#define H2G_GW_MAXROWS   64      // fixed: the row masks of the group walk are 64-bit words
#define H2G_AWA_DEPTH    24
#define H2G_AWA_CAND     8
#define H2G_OFFDIFF_CAP  64
