// The reference's alignment options -> h2g_align_params (include/h2g.h): the one place where an option's text becomes a field.
// Host only, no device and no index: the command line (h2g_cli.cpp) and the Python binding (api.py) both parse through it.
// Parse rules of hisat2.cpp:1500-1620 / aligner_seed_policy.cpp.
#include "../../include/h2g.h"
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

namespace {

enum Op {
	O_K, O_MAX_SEEDS, O_SECONDARY, O_MP, O_SP, O_NO_SOFTCLIP, O_NP, O_RDG, O_RFG, O_SCORE_MIN, O_N_CEIL, O_MIN_INTRONLEN, O_MAX_INTRONLEN,
	O_PEN_CANSPLICE, O_PEN_NONCANSPLICE, O_PEN_CONFLICTSPLICE, O_PEN_CANINTRONLEN, O_PEN_NONCANINTRONLEN, O_SENSITIVE, O_VERY_SENSITIVE,
	O_NO_SPLICED, O_NO_TEMP_SS, O_BOWTIE2_DP, O_DTA, O_DTA_CUFFLINKS, O_AVOID_PSEUDOGENE, O_TMO, O_NO_ANCHORSTOP, O_SS_DB_ONLY, O_HAPLOTYPE,
	O_MAX_ALTSTRIED, O_MAXINS, O_MININS, O_FR, O_RF, O_FF, O_NOFW, O_NORC, O_IGNORE_QUALS, O_SEED
};
struct Opt { const char* name; int arity; Op op; };
const Opt OPTS[] = {
	{"-k", 1, O_K}, {"--max-seeds", 1, O_MAX_SEEDS}, {"--secondary", 0, O_SECONDARY}, {"--mp", 1, O_MP}, {"--sp", 1, O_SP}, {"--no-softclip", 0, O_NO_SOFTCLIP},
	{"--np", 1, O_NP}, {"--rdg", 1, O_RDG}, {"--rfg", 1, O_RFG}, {"--score-min", 1, O_SCORE_MIN}, {"--n-ceil", 1, O_N_CEIL},
	{"--min-intronlen", 1, O_MIN_INTRONLEN}, {"--max-intronlen", 1, O_MAX_INTRONLEN}, {"--pen-cansplice", 1, O_PEN_CANSPLICE},
	{"--pen-noncansplice", 1, O_PEN_NONCANSPLICE}, {"--pen-conflictsplice", 1, O_PEN_CONFLICTSPLICE}, {"--pen-canintronlen", 1, O_PEN_CANINTRONLEN},
	{"--pen-intronlen", 1, O_PEN_CANINTRONLEN}, {"--pen-noncanintronlen", 1, O_PEN_NONCANINTRONLEN}, {"--sensitive", 0, O_SENSITIVE},
	{"--very-sensitive", 0, O_VERY_SENSITIVE}, {"--no-spliced-alignment", 0, O_NO_SPLICED}, {"--no-temp-splicesite", 0, O_NO_TEMP_SS},
	{"--bowtie2-dp", 1, O_BOWTIE2_DP}, {"--dta", 0, O_DTA}, {"--downstream-transcriptome-assembly", 0, O_DTA}, {"--dta-cufflinks", 0, O_DTA_CUFFLINKS},
	{"--avoid-pseudogene", 0, O_AVOID_PSEUDOGENE}, {"--tmo", 0, O_TMO}, {"--transcriptome-mapping-only", 0, O_TMO}, {"--no-anchorstop", 0, O_NO_ANCHORSTOP},
	{"--splicesite-db-only", 0, O_SS_DB_ONLY}, {"--haplotype", 0, O_HAPLOTYPE}, {"--max-altstried", 1, O_MAX_ALTSTRIED}, {"-X", 1, O_MAXINS},
	{"--maxins", 1, O_MAXINS}, {"-I", 1, O_MININS}, {"--minins", 1, O_MININS}, {"--fr", 0, O_FR}, {"--rf", 0, O_RF}, {"--ff", 0, O_FF},
	{"--nofw", 0, O_NOFW}, {"--norc", 0, O_NORC}, {"--ignore-quals", 0, O_IGNORE_QUALS}, {"--seed", 1, O_SEED},
};
const Opt* find_opt(const char* name) {
	if(name) for(const Opt& o : OPTS) if(!strcmp(o.name, name)) return &o;
	return nullptr;
}

std::vector<std::string> split_commas(const char* s) {     // empty tokens are dropped (tokenize)
	std::vector<std::string> v;
	std::string cur;
	for(; *s; s++) { if(*s == ',') { if(!cur.empty()) v.push_back(cur); cur.clear(); } else cur.push_back(*s); }
	if(!cur.empty()) v.push_back(cur);
	return v;
}
h2g_status fail(char* err, size_t cap, const char* fmt, ...) {
	if(err && cap) { va_list ap; va_start(ap, fmt); vsnprintf(err, cap, fmt, ap); va_end(ap); }
	return H2G_ERR_ARG;
}
void two(const char* v, int32_t* x, int32_t* y) { *x = atoi(v); const char* c = strchr(v, ','); if(c) *y = atoi(c + 1); }
uint32_t func_letter(const char* v) { return v[0] == 'C' ? 1 : v[0] == 'L' ? 2 : v[0] == 'S' ? 3 : v[0] == 'G' ? 4 : 0; }

}  // namespace

extern "C" int h2g_align_option_arity(const char* name) { const Opt* o = find_opt(name); return o ? o->arity : -1; }

extern "C" h2g_status h2g_align_params_apply_options(h2g_align_params* p, h2g_align_presets* pre, const char* const* opts, size_t n, char* err, size_t err_cap) {
	if(!p || !pre || (!opts && n)) return fail(err, err_cap, "h2g_align_params_apply_options: null argument");
	h2g_align_params& P = *p;
	*pre = h2g_align_presets{0, 0, 0, 0, 0};
	bool dta = false, ignore_quals = false, saw_mp = false;
	for(size_t i = 0; i < n; i++) {
		const char* o = opts[i];
		const Opt* opt = find_opt(o);
		if(!opt) return fail(err, err_cap, "%s is not an alignment option", o ? o : "(null)");
		if(opt->arity && (i + 1 >= n || !opts[i + 1])) return fail(err, err_cap, "option %s needs an argument", o);
		const char* v = opt->arity ? opts[++i] : "";
		switch(opt->op) {
		case O_K: {
			const int k = atoi(v);
			if(k < 1) return fail(err, err_cap, "-k arg must be at least 1");
			pre->k_arg = (uint32_t)k; pre->saw_k = 1;
			break;
		}
		case O_MAX_SEEDS: pre->max_seeds_arg = (uint32_t)atoi(v); break;
		case O_N_CEIL: {
			// hisat2.cpp:1525-1549: 1-3 tokens, one token x is C,x; then PARSE_FUNC (aligner_seed_policy.cpp:47-70): type, constant and coefficient
			// when given (istringstream >> double), the others keep their value
			std::vector<std::string> t = split_commas(v);
			if(t.size() > 3) return fail(err, err_cap, "Error: expected 3 or fewer comma-separated arguments to --n-ceil option, got %zu", t.size());
			if(t.empty()) return fail(err, err_cap, "Error: expected at least one argument to --n-ceil option");
			if(t.size() == 1) t.insert(t.begin(), "C");
			const std::string& ty = t[0];
			const uint32_t type = ty == "C" || ty == "Constant" ? 1 : ty == "L" || ty == "Linear" ? 2 : ty == "S" || ty == "Sqrt" ? 3 : ty == "G" || ty == "Log" ? 4 : 0;
			if(!type) return fail(err, err_cap, "Error: Bad function type '%s'.  Should be C (constant), L (linear), S (square root) or G (natural log).", ty.c_str());
			auto num = [](const std::string& s) { double d = 0.0; std::istringstream ss(s); ss >> d; return d; };
			P.n_ceil_type = type;
			if(t.size() > 1) P.n_ceil_const = num(t[1]);
			if(t.size() > 2) P.n_ceil_coeff = num(t[2]);
			break;
		}
		case O_SECONDARY: P.secondary = 1; break;
		case O_MP:
			// refused where the option is read, whatever --ignore-quals does later (aligner_seed_policy.cpp:411-416; the message ends without its bracket).
			// The maximum is a divisor of go() (maxmm, the pair bound): below 1 the reference itself dies of SIGFPE (--mp 0,0), so that refusal is ours
			two(v, &P.mm_max, &P.mm_min); saw_mp = true;
			if(P.mm_min > P.mm_max) return fail(err, err_cap, "Error: Maximum mismatch penalty (%d) is less than minimum penalty (%d", P.mm_max, P.mm_min);
			if(P.mm_max < 1) return fail(err, err_cap, "--mp: the maximum mismatch penalty must be at least 1 (got %d)", P.mm_max);
			break;
		case O_SP: {   // both read from the first number (aligner_seed_policy.cpp:438); the minimum is a divisor of the trimming bound (:446-449)
			int32_t unused = 0; two(v, &P.sc_max, &unused); P.sc_min = P.sc_max;
			if(P.sc_min < 1) return fail(err, err_cap, "min (%d) should be greater than 0", P.sc_min);
			break;
		}
		case O_NO_SOFTCLIP: P.sc_max = P.sc_min = INT32_MAX; break;
		case O_NP: P.n_pen = atoi(v); break;
		// a gap extension below 1 never ends Scoring::maxReadGaps / maxRefGaps (scoring.cpp:53, :84: the reference hangs; max_gaps here would): refused by name
		case O_RDG: case O_RFG: {
			const bool rd = opt->op == O_RDG;
			two(v, rd ? &P.rdg_const : &P.rfg_const, rd ? &P.rdg_linear : &P.rfg_linear);
			if((rd ? P.rdg_linear : P.rfg_linear) < 1) return fail(err, err_cap, "%s: the gap extension penalty must be at least 1 (got %d)", o, rd ? P.rdg_linear : P.rfg_linear);
			break;
		}
		case O_SCORE_MIN: {
			P.score_min_type = func_letter(v);
			if(!P.score_min_type) return fail(err, err_cap, "Error: bad function type in --score-min %s", v);
			P.score_min_const = P.score_min_coeff = 0.0;
			const char* c1 = strchr(v, ',');
			if(c1) { P.score_min_const = atof(c1 + 1); const char* c2 = strchr(c1 + 1, ','); if(c2) P.score_min_coeff = atof(c2 + 1); }
			break;
		}
		// splice scoring hisat2.cpp:1631-1688
		case O_MIN_INTRONLEN: case O_MAX_INTRONLEN: {
			const int x = atoi(v);
			if(x < 20) return fail(err, err_cap, "%s arg must be at least 20", o);
			(opt->op == O_MIN_INTRONLEN ? P.min_intronlen : P.max_intronlen) = (uint32_t)x;
			break;
		}
		case O_PEN_CANSPLICE: case O_PEN_NONCANSPLICE: case O_PEN_CONFLICTSPLICE: {
			const int x = atoi(v);
			if(x < 0) return fail(err, err_cap, "%s arg must be at least 0", o);
			(opt->op == O_PEN_CANSPLICE ? P.pen_cansplice : opt->op == O_PEN_NONCANSPLICE ? P.pen_noncansplice : P.pen_conflictsplice) = x;
			break;
		}
		case O_PEN_CANINTRONLEN: case O_PEN_NONCANINTRONLEN: {   // PARSE_FUNC: only the given fields change
			const bool nc = opt->op == O_PEN_NONCANINTRONLEN;
			const uint32_t t = func_letter(v);
			if(!t) return fail(err, err_cap, "Error: bad function type in %s %s", o, v);
			(nc ? P.pen_noncanintronlen_type : P.pen_canintronlen_type) = t;
			const char* c1 = strchr(v, ',');
			if(c1) {
				(nc ? P.pen_noncanintronlen_const : P.pen_canintronlen_const) = atof(c1 + 1);
				const char* c2 = strchr(c1 + 1, ',');
				if(c2) (nc ? P.pen_noncanintronlen_coeff : P.pen_canintronlen_coeff) = atof(c2 + 1);
			}
			break;
		}
		case O_SENSITIVE: pre->sensitive = 1; break;
		case O_VERY_SENSITIVE: pre->very_sensitive = 1; break;
		case O_NO_SPLICED: P.no_spliced_alignment = 1; break;
		case O_NO_TEMP_SS: P.no_temp_splicesite = 1; break;
		case O_BOWTIE2_DP: P.bowtie2_dp = (uint32_t)atoi(v); break;
		case O_DTA: dta = true; break;
		case O_DTA_CUFFLINKS: dta = true; P.xs_only = 1; break;
		case O_AVOID_PSEUDOGENE: P.avoid_pseudogene = 1; break;               // TranscriptomePolicy (tp.h), reportHit hi_aligner.h:6105-6127
		case O_TMO: P.transcriptome_mapping_only = 1; break;
		case O_NO_ANCHORSTOP: P.no_anchorstop = 1; break;                     // hisat2.cpp:1710-1712
		case O_SS_DB_ONLY: break;                                             // accepted and read nowhere by the reference (hisat2.cpp:1706-1708)
		case O_HAPLOTYPE: P.use_haplotype = 1; break;                         // hisat2.cpp:1749 (ARG_HAPLOTYPE)
		case O_MAX_ALTSTRIED: { const int x = atoi(v); if(x < 8) return fail(err, err_cap, "--max-altstried arg must be at least 8"); P.max_alts_tried = (uint32_t)x; break; }
		case O_MAXINS: { const int x = atoi(v); if(x < 1) return fail(err, err_cap, "-X arg must be at least 1"); P.max_frag_len = (uint32_t)x; break; }
		case O_MININS: { const int x = atoi(v); if(x < 0) return fail(err, err_cap, "-I arg must be positive"); P.min_frag_len = (uint32_t)x; break; }
		case O_FR: P.pe_orientation = 0; break;                               // hisat2.cpp:1166-1168
		case O_RF: P.pe_orientation = 1; break;
		case O_FF: P.pe_orientation = 2; break;
		case O_NOFW: P.nofw = 1; break;                                       // hisat2.cpp:1337-1338
		case O_NORC: P.norc = 1; break;
		case O_IGNORE_QUALS: ignore_quals = true; break;                      // hisat2.cpp:1434
		case O_SEED: {                                                        // parseInt(0, ...) hisat2.cpp:1204, 1016-1032
			const long s = strtol(v, nullptr, 10);
			if(s < 0 || s > INT32_MAX) return fail(err, err_cap, "--seed arg must be at least 0");
			P.seed = (uint32_t)s;
			break;
		}
		}
	}
	if(dta) {   // hisat2.cpp:3920, 4078-4079: after every option was read
		P.min_anchor_len = 15; P.min_anchor_len_noncan = 20;
		P.pen_noncanintronlen_type = 4; P.pen_noncanintronlen_const = -8.0; P.pen_noncanintronlen_coeff = 2.0;
	}
	// COST_MODEL_CONSTANT: every mismatch costs the maximum (aligner_seed_policy.cpp:279, scoring.h:129); a --mp sets the quality model again (:418)
	if(ignore_quals && !saw_mp) P.mm_min = P.mm_max;
	return H2G_OK;
}

// hisat2.cpp applies its presets AFTER every option was read, and the index type decides the default -k:
//   khits starts at 10 (:336); -k sets it and saw_k (:1316-1322); --sensitive: bowtie2_dp 0 -> 1, khits < 10 -> 10 (+ saw_k),
//   --score-min L,0,-0.5 (:1892-1901); --very-sensitive: bowtie2_dp 2, khits < 30 -> 30 (+ saw_k), L,0,-1 (:1902-1909);
//   without saw_k khits = 5 on a linear index, 10 on a graph (:3903-3906); --max-seeds 0 -> max(5, 2 khits) (:3174-3176).
// So `--sensitive` alone keeps -k 5 on a linear index, and a preset's --score-min wins over an explicit one.
extern "C" void h2g_align_params_presets(h2g_align_params* p, int linear, const h2g_align_presets* pre) {
	if(!p || !pre) return;
	uint32_t khits = pre->saw_k ? pre->k_arg : 10u;
	bool sawk = pre->saw_k != 0;
	if(pre->sensitive) {
		if(p->bowtie2_dp == 0) p->bowtie2_dp = 1;
		if(khits < 10) { khits = 10; sawk = true; }
		p->score_min_type = 2; p->score_min_const = 0.0; p->score_min_coeff = (double)(-0.5f);
	} else if(pre->very_sensitive) {
		p->bowtie2_dp = 2;
		if(khits < 30) { khits = 30; sawk = true; }
		p->score_min_type = 2; p->score_min_const = 0.0; p->score_min_coeff = (double)(-1.0f);
	}
	if(!sawk) khits = linear ? 5u : 10u;
	p->khits = khits;
	p->kseeds = pre->max_seeds_arg ? pre->max_seeds_arg : (khits * 2 > 5 ? khits * 2 : 5);
}
