// h2g_cli_sort.h — the read files of the command line (h2g_cli.cpp): --un / --al / --un-conc / --al-conc / --al-conc-disc and their -gz forms, their file names,
// and the sorting of every read's original record by the flags of its SAM lines (`ReadSorter`).  Header-only, host code.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <sys/stat.h>
#include <zlib.h>

namespace h2g_cli {

// the flag field of the SAM line [t, le); a line without one counts as secondary (0x100: no read file takes it, --no-unal keeps it)
inline unsigned sam_flag_of_line(const char* t, const char* le) {
	const char* tab = (const char*)memchr(t, '\t', (size_t)(le - t));
	return tab ? (unsigned)strtoul(tab + 1, nullptr, 10) : 0x100u;
}

// --un / --al / --un-conc / --al-conc / --al-conc-disc (and -gz): the reference's wrapper script sorts every read's original record by the flags of its
// non-secondary SAM line(s); here the command line's formatter stage does, from the lines it has just formatted.
struct ReadFile {
	FILE* f = nullptr; gzFile g = nullptr;
	void open(const std::string& fn, bool gz) {
		if(gz) g = gzopen(fn.c_str(), "wb"); else f = fopen(fn.c_str(), "wb");
		if(!g && !f) { fprintf(stderr, "Error: could not open %s for writing\n", fn.c_str()); exit(1); }
	}
	bool bad = false;                 // a write or the close failed
	void put(const char* p, size_t n) { if(!n) return; if(g) { if(gzwrite(g, p, (unsigned)n) != (int)n) bad = true; } else if(f && fwrite(p, 1, n, f) != n) bad = true; }
	void close() { if(g && gzclose(g) != Z_OK) bad = true; if(f && fclose(f) != 0) bad = true; g = nullptr; f = nullptr; }
};
enum { RS_UN, RS_AL, RS_UN_CONC, RS_AL_CONC, RS_AL_CONC_DISC, RS_KINDS };
const char* const rs_names[RS_KINDS] = {"un", "al", "un-conc", "al-conc", "al-conc-disc"};
inline bool is_directory(const std::string& p) { struct stat sb; return stat(p.c_str(), &sb) == 0 && S_ISDIR(sb.st_mode); }
// the file name(s) of one of these options: an unpaired kind writes to its argument (<dir>/un-seqs, <dir>/al-seqs for a directory); a -conc kind to two files,
// named after the argument's base name: every '%' becomes 1 / 2, else .1 / .2 goes before the last extension, else it is appended (<dir>/un-conc-mate.1 ...)
inline void read_sink_names(int kind, const std::string& arg, std::string* fn1, std::string* fn2) {
	std::string dir, base;
	if(is_directory(arg) || (!arg.empty() && arg.back() == '/')) { dir = arg; if(dir.back() != '/') dir.push_back('/'); }
	else { const size_t sl = arg.rfind('/'); if(sl == std::string::npos) base = arg; else { dir = arg.substr(0, sl + 1); base = arg.substr(sl + 1); } }
	if(kind == RS_UN || kind == RS_AL) { *fn1 = base.empty() ? dir + rs_names[kind] + "-seqs" : arg; fn2->clear(); return; }
	if(base.empty()) base = std::string(rs_names[kind]) + "-mate";
	std::string b1 = base, b2 = base;
	const size_t dot = base.rfind('.');
	if(base.find('%') != std::string::npos) { for(char& c : b1) if(c == '%') c = '1'; for(char& c : b2) if(c == '%') c = '2'; }
	else if(dot != std::string::npos) { b1.insert(dot, ".1"); b2.insert(dot, ".2"); }
	else { b1 += ".1"; b2 += ".2"; }
	*fn1 = dir + b1; *fn2 = dir + b2;
}
// which read-file option `a` is: 0 none of them, 1 + 2 kind + (1 if -gz), -1 a -bz2 / -lz4 form (refused by name)
inline int read_sink_option(const std::string& a) {
	for(int k = 0; k < RS_KINDS; k++) {
		const std::string o = std::string("--") + rs_names[k];
		if(a == o) return 1 + 2 * k;
		if(a == o + "-gz") return 2 + 2 * k;
		if(a == o + "-bz2" || a == o + "-lz4") return -1;
	}
	return 0;
}
struct ReadSorter {
	bool on = false;
	ReadFile out[RS_KINDS][2];
	bool have[RS_KINDS] = {false, false, false, false, false};
	void open(int kind, const std::string& arg, bool gz) {
		std::string f1, f2;
		read_sink_names(kind, arg, &f1, &f2);
		out[kind][0].open(f1, gz);
		if(!f2.empty()) out[kind][1].open(f2, gz);
		have[kind] = true; on = true;
	}
	bool close() { bool ok = true; for(auto& k : out) for(ReadFile& f : k) { f.close(); ok = ok && !f.bad; } return ok; }   // false: writing one of the files failed
	// one record: its SAM lines [t, te) and the original text of its read (unpaired) or of its two mates
	void record(const char* t, const char* te, const char* o1, size_t n1, const char* o2, size_t n2) {
		while(t < te) {
			const char* le = (const char*)memchr(t, '\n', (size_t)(te - t));
			if(!le) le = te;
			const unsigned fl = sam_flag_of_line(t, le);
			t = le + 1;
			if(fl & 0x100u) continue;                                 // one write per read, however many -k lines it has
			const bool m1 = (fl & 0x40u) != 0, m2 = (fl & 0x80u) != 0;
			if(!m1 && !m2) { ReadFile& f = out[(fl & 4u) ? RS_UN : RS_AL][0]; f.put(o1, n1); continue; }
			const int m = m1 ? 0 : 1;
			const char* o = m1 ? o1 : o2;
			const size_t n = m1 ? n1 : n2;
			out[(fl & 2u) ? RS_AL_CONC : RS_UN_CONC][m].put(o, n);
			if(!(fl & 4u) || !(fl & 8u)) out[RS_AL_CONC_DISC][m].put(o, n);
		}
	}
};

}  // namespace h2g_cli
