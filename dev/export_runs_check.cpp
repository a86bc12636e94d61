// export_runs_check.cpp -- the arithmetic of the aligned run builder (aligned_segments, pangraph_amd/csrc/pga_runs.h) without a device:
// random edits are prepared (prepare_edit), turned into runs, the runs listed forward and -- as row_piece_runs (pga_rows.h) lists a piece on the
// reverse strand -- backwards, and a scalar walk of each table (letter by letter, as k_rows steps from run to run) is compared with a direct
// Edit::apply_aligned (edits.rs:331-347) and its reverse complement.  Shapes: substitutions under deletions, duplicate positions,
// overlapping and adjacent deletions, deletions of the whole consensus, consensus lengths around 16.
// Build and run (host only):  g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ipangraph_amd/csrc -Iinclude
//                             dev/export_runs_check.cpp -o export_runs_check && ./export_runs_check
#define __constant__
#include "pga_runs.h"
#include <cstdio>
#include <random>
#include <string>

using namespace pga;

struct Run { uint32_t out, kind; uint64_t src; };                      // as RowRun of pga_rows.h: kind | 4 = read backwards and complement

static std::string walk(const std::vector<Run> &R, uint32_t len, const std::string &cons, bool &bad)
{
	std::string s(len, '?');
	size_t a = 0;
	for (uint32_t b = 0; b < len; ++b) {
		while (a + 1 < R.size() && R[a + 1].out <= b) ++a;
		const uint32_t s_beg = R[a].out, s_end = a + 1 < R.size() ? R[a + 1].out : len;
		if (b < s_beg || b >= s_end || s_end <= s_beg) { fprintf(stderr, "run table not ordered or with an empty run at letter %u\n", b); exit(2); }
		const bool rev = (R[a].kind & 4u) != 0u;
		const uint32_t kd = R[a].kind & 3u, off = rev ? s_end - 1u - b : b - s_beg;
		if (kd == 1u) { fprintf(stderr, "an insertion run in an aligned table\n"); exit(2); }
		if (kd == 0u && R[a].src + off >= cons.size()) { fprintf(stderr, "consensus read out of bounds\n"); exit(2); }
		uint32_t c = kd == 0u ? (uint8_t)cons[R[a].src + off] : kd == 2u ? (uint32_t)(R[a].src & 255u) : (uint32_t)'-';
		if (rev) { const uint32_t cc = h_comp.t[c]; if (cc) c = cc; else bad = true; }
		s[b] = (char)c;
	}
	return s;
}

int main()
{
	std::mt19937_64 rng(20261018);
	auto below = [&](uint64_t n) { return (uint32_t)(rng() % n); };
	const char letters[] = "ACGTYRWSKMDVHBN-";
	const uint32_t lens[] = {1, 2, 15, 16, 17, 31, 32, 33, 64, 100, 257};
	long cases = 0, gaps = 0, lost = 0, dup = 0, whole = 0;
	for (int it = 0; it < 20000; ++it) {
		const uint32_t L = lens[below(sizeof(lens) / sizeof(lens[0]))];
		const uint64_t base = below(40);                                    // the consensus somewhere inside a longer buffer
		std::string buf(base + L + below(5), 'x'), cons(L, 'A');
		for (uint32_t i = 0; i < L; ++i) cons[i] = buf[base + i] = letters[below(it % 4 ? 4 : 16)];
		std::vector<pga_sub_t> subs; std::vector<pga_del_t> dels; std::vector<pga_ins_t> inss;
		const int shape = it % 8;
		for (uint32_t k = below(6); k-- > 0;) {
			const uint32_t pos = below(L), len = below(L - pos + 1);
			dels.push_back(pga_del_t{pos, shape == 1 ? std::min(len, 20u) : len});
			if (shape == 2 && pos + len < L) dels.push_back(pga_del_t{pos + len, below(L - pos - len + 1)});     // adjacent
			if (shape == 3 && len) dels.push_back(pga_del_t{pos + below(len), 1u});                              // inside another
		}
		if (shape == 4) { dels.push_back(pga_del_t{0u, L}); ++whole; }
		if (shape == 5) { dels.push_back(pga_del_t{0u, L / 2}); dels.push_back(pga_del_t{L / 2, L - L / 2}); ++whole; }
		for (uint32_t k = below(8); k-- > 0;) {
			const uint32_t pos = below(L);
			subs.push_back(pga_sub_t{pos, (uint32_t)(uint8_t)letters[below(16)]});
			if (below(3) == 0) { subs.push_back(pga_sub_t{pos, (uint32_t)(uint8_t)letters[below(16)]}); ++dup; }
		}
		for (const pga_del_t &d : dels) if (d.len && below(2)) subs.push_back(pga_sub_t{d.pos + below(d.len), (uint32_t)'G'});   // under a deletion
		for (size_t i = subs.size(); i > 1; --i) std::swap(subs[i - 1], subs[below(i)]);
		for (uint32_t k = below(3); k-- > 0;) inss.push_back(pga_ins_t{below(L + 1), 0u, 0u});                   // ignored in aligned mode
		// ---- Edit::apply_aligned, directly ----
		std::string want = cons;
		for (const pga_sub_t &s : subs) want[s.pos] = (char)s.alt;
		for (const pga_del_t &d : dels) for (uint32_t p = d.pos; p < d.pos + d.len; ++p) { if (want[p] != cons[p] && want[p] != '-') ++lost; want[p] = '-'; }
		std::string want_rc(L, '?');
		for (uint32_t i = 0; i < L; ++i) want_rc[i] = (char)h_comp.t[(uint8_t)want[L - 1 - i]];
		// ---- the runs ----
		PreparedEdit P;
		prepare_edit(subs.data(), (uint32_t)subs.size(), dels.data(), (uint32_t)dels.size(), inss.data(), 0u, nullptr, L, P);
		std::vector<PrSeg> segs;
		const uint32_t built = aligned_segments(P, L, base, segs);
		if (built != L) { fprintf(stderr, "case %d: the runs add up to %u, not %u\n", it, built, L); return 1; }
		std::vector<Run> fwd, rev;
		const uint32_t ns = (uint32_t)segs.size();
		for (uint32_t s = 0; s < ns; ++s) { fwd.push_back(Run{segs[s].out, segs[s].kind, segs[s].src}); if (segs[s].kind == PR_GAP) ++gaps; }
		for (uint32_t s = ns; s-- > 0;) rev.push_back(Run{built - (s + 1 < ns ? segs[s + 1].out : built), segs[s].kind | 4u, segs[s].src});
		for (uint32_t s = 0; s + 1 < ns; ++s) if (segs[s].kind == PR_GAP && segs[s + 1].kind == PR_GAP) { fprintf(stderr, "case %d: two gap runs in a row (intervals not merged)\n", it); return 1; }
		bool bad = false;
		const std::string got = walk(fwd, L, buf, bad), got_rc = walk(rev, L, buf, bad);
		if (bad) { fprintf(stderr, "case %d: the complement rejected one of its own letters\n", it); return 1; }
		if (got != want || got_rc != want_rc) {
			fprintf(stderr, "case %d (L %u) differs\n  cons %s\n  want %s\n  got  %s\n  want_rc %s\n  got_rc  %s\n", it, L, cons.c_str(), want.c_str(), got.c_str(), want_rc.c_str(), got_rc.c_str());
			return 1;
		}
		++cases;
	}
	if (!gaps || !lost || !dup || !whole) { fprintf(stderr, "the generator missed a shape: gaps %ld lost %ld dup %ld whole %ld\n", gaps, lost, dup, whole); return 1; }
	printf("export_runs_check OK: %ld cases, %ld gap runs, %ld substitutions lost under deletions, %ld duplicate positions, %ld whole-consensus deletions\n", cases, gaps, lost, dup, whole);
	return 0;
}
