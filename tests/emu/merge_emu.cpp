// pga_merge_idx.h without a device: the tables of mg_build_tables and the list kernels k_merge_lists / k_merge_count / k_merge_write run under
// dev/emu/hip_emu.h, then k_rows<false> (pga_rows.h) over the runs they built, every buffer allocated at exactly the size the kernels may
// touch -- under the address sanitizer an access one entry out is an error -- against a direct scalar construction of every edge:
// PangraphBlock::reverse_complement (pangraph_block.rs:63-75), Edit::reverse_complement with a stable sort (edits.rs:257-276), Edit::shift and
// Edit::concat (edits.rs:278-304).  The emulator has no wave intrinsics: k_merge_scan of pga_merge.hip, the one-wave exclusive sum of the
// output insertion counts, is NOT run here; a plain loop stands in for it.
// Build and run (host only):  g++ -std=c++17 -g -O1 -DPGA_EMU -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined
//                             tests/emu/merge_emu.cpp -o merge_emu && ./merge_emu
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include "../../dev/emu/hip_emu.h"
#include "../../pangraph_amd/csrc/pga_merge_idx.h"

using namespace pga;

typedef std::pair<uint32_t, std::string> Ins;
struct Member { std::vector<pga_sub_t> subs; std::vector<pga_del_t> dels; std::vector<Ins> inss; };
struct Block { std::string cons; std::vector<Member> mem; };

static bool g_bad;                                                      // the direct construction met a letter without a complement
static char comp(char c) { const uint8_t t = h_comp.t[(uint8_t)c]; if (!t) { g_bad = true; return c; } return (char)t; }
static std::string revcomp(const std::string &s) { std::string r; for (size_t i = s.size(); i-- > 0;) r.push_back(comp(s[i])); return r; }
static Member edit_revcomp(const Member &e, uint32_t len)
{
	Member r;
	for (auto &s : e.subs) r.subs.push_back(pga_sub_t{len - s.pos - 1, (uint32_t)(uint8_t)comp((char)s.alt)});
	for (auto &d : e.dels) r.dels.push_back(pga_del_t{len - d.pos - d.len, d.len});
	for (auto &i : e.inss) r.inss.push_back(Ins{len - i.first, revcomp(i.second)});
	std::stable_sort(r.subs.begin(), r.subs.end(), [](const pga_sub_t &a, const pga_sub_t &b) { return a.pos < b.pos; });
	std::stable_sort(r.dels.begin(), r.dels.end(), [](const pga_del_t &a, const pga_del_t &b) { return a.pos < b.pos; });
	std::stable_sort(r.inss.begin(), r.inss.end(), [](const Ins &a, const Ins &b) { return a.first < b.first; });
	return r;
}
static Member edit_concat(const Member &a, const Member &b, uint32_t shift)
{
	Member r = a;
	for (auto &i : b.inss) {
		bool found = false;
		for (auto &p : r.inss) if (p.first == i.first + shift) { p.second += i.second; found = true; break; }
		if (!found) r.inss.push_back(Ins{i.first + shift, i.second});
	}
	for (auto &d : b.dels) r.dels.push_back(pga_del_t{d.pos + shift, d.len});
	for (auto &s : b.subs) r.subs.push_back(pga_sub_t{s.pos + shift, s.alt});
	return r;
}

template <class T> struct Exact {                                       // n entries, not one more
	std::unique_ptr<T[]> p; size_t n;
	explicit Exact(size_t n_) : p(n_ ? new T[n_]() : nullptr), n(n_) {}
	T *get() { return p.get(); }
};

static std::mt19937 rng(20260117);
static uint32_t rnd(uint32_t n) { return n ? (uint32_t)(rng() % n) : 0u; }

static std::string letters(uint32_t n, bool may_be_bad)
{
	std::string s;
	for (uint32_t i = 0; i < n; ++i) s.push_back("ACGTNRY"[rnd(7)]);
	if (may_be_bad && n && rnd(12) == 0) s[rnd(n)] = rnd(2) ? 'a' : 'X';
	return s;
}
// positions of a list of n entries over [0, hi]: style 0 strictly increasing where there is room, 1 sorted with repeats, 2 any order
static std::vector<uint32_t> positions(uint32_t n, uint32_t hi, int style)
{
	std::vector<uint32_t> p;
	if (style == 0 && n <= hi + 1) {
		std::vector<uint32_t> all(hi + 1);
		for (uint32_t i = 0; i <= hi; ++i) all[i] = i;
		std::shuffle(all.begin(), all.end(), rng);
		p.assign(all.begin(), all.begin() + n);
		std::sort(p.begin(), p.end());
		return p;
	}
	for (uint32_t i = 0; i < n; ++i) p.push_back(rnd(hi + 1));
	if (style != 2) std::sort(p.begin(), p.end());
	return p;
}
static int style() { const uint32_t r = rnd(6); return r < 4 ? 0 : (int)r - 3; }                // mostly the usual lists
static uint32_t list_len() { static const uint32_t k[] = {0, 0, 1, 2, 3, 5, 63, 64, 65, 130}; return k[rnd(10)]; }

static Member random_member(uint32_t L)
{
	Member m;
	if (L) {
		auto ps = positions(list_len(), L - 1, style());
		for (uint32_t p : ps) m.subs.push_back(pga_sub_t{p, (uint32_t)(uint8_t)letters(1, true)[0]});
		auto pd = positions(list_len(), L - 1, style());
		for (uint32_t p : pd) m.dels.push_back(pga_del_t{p, rnd(L - p + 1)});
	}
	auto pi = positions(list_len(), L, style());
	static const uint32_t il[] = {0, 1, 1, 2, 15, 16, 17, 40};
	for (uint32_t p : pi) m.inss.push_back(Ins{p, letters(il[rnd(8)], true)});
	if (rnd(3) == 0) {                                                    // the boundary, in its sorted place unless the list holds it already
		if (rnd(2)) m.inss.insert(m.inss.begin(), Ins{0u, letters(1 + rnd(20), false)}); else m.inss.push_back(Ins{L, letters(1 + rnd(20), false)});
	}
	if (rnd(4) == 0) m.inss.insert(m.inss.begin() + rnd((uint32_t)m.inss.size() + 1), Ins{rnd(2) ? 0u : L, letters(rnd(5), false)});
	return m;
}

int main()
{
	static const uint32_t cons_len[] = {0, 1, 15, 16, 17, 31, 32, 33, 100, 300};
	uint64_t n_checked = 0, n_slow = 0, n_boundary = 0, n_bad = 0;
	for (int round = 0; round < 40; ++round) {
		// ---- a graph and a batch of edges ----
		const uint32_t nb = 2 + rnd(6);
		const uint32_t depth_of[] = {0, 1, 2, 3, 5, 70};
		std::vector<Block> blocks(nb);
		std::vector<uint32_t> depth_class(nb);
		for (uint32_t b = 0; b < nb; ++b) {
			depth_class[b] = rnd(3);                                            // (blocks of one class share a depth and can be joined)
			const uint32_t depth = round % 20 == 7 ? depth_of[5 - depth_class[b]] : depth_of[(round + depth_class[b]) % 5];
			blocks[b].cons = letters(cons_len[rnd(10)], true);
			for (uint32_t k = 0; k < depth; ++k) blocks[b].mem.push_back(random_member((uint32_t)blocks[b].cons.size()));
		}
		std::vector<pga_rc_block_t> B; std::vector<pga_rc_member_t> M; std::vector<pga_sub_t> S; std::vector<pga_del_t> D; std::vector<pga_ins_t> I;
		std::string iseq(5, '?');
		for (const Block &b : blocks) {
			B.push_back(pga_rc_block_t{b.cons.data(), (uint32_t)b.cons.size(), (uint32_t)b.mem.size()});
			for (const Member &m : b.mem) {
				M.push_back(pga_rc_member_t{(uint32_t)m.subs.size(), (uint32_t)m.dels.size(), (uint32_t)m.inss.size()});
				S.insert(S.end(), m.subs.begin(), m.subs.end()); D.insert(D.end(), m.dels.begin(), m.dels.end());
				for (auto &x : m.inss) { I.push_back(pga_ins_t{x.first, (uint32_t)x.second.size(), (uint64_t)iseq.size()}); iseq += x.second; }
			}
		}
		std::vector<pga_merge_edge_t> E; std::vector<uint32_t> partner;
		for (uint32_t tries = 0; tries < 12; ++tries) {
			const uint32_t l = rnd(nb), r = rnd(nb);
			if (blocks[l].mem.size() != blocks[r].mem.size()) continue;
			E.push_back(pga_merge_edge_t{l, r, (int32_t)rnd(2), (int32_t)rnd(2)});
			std::vector<uint32_t> perm(blocks[l].mem.size());
			for (uint32_t k = 0; k < perm.size(); ++k) perm[k] = k;
			std::shuffle(perm.begin(), perm.end(), rng);
			partner.insert(partner.end(), perm.begin(), perm.end());
		}
		// ---- the tables ----
		RowGraph G;
		row_graph_init(G, "merge_emu", (int64_t)nb, B.data(), M.data(), S.data(), D.data(), I.data(), iseq.data(), true, 1);
		MgTables T;
		mg_build_tables(G, (int64_t)E.size(), E.data(), partner.data(), T);
		const uint64_t n_mem = T.mem.size();
		// ---- the "device" ----
		Exact<uint32_t> flags(n_mem), first_l(n_mem), b_cnt(n_mem), n_ins(n_mem), lead(T.n_lead), edge_bad(E.size());
		Exact<mg_u64> b_sum(n_mem), ins_off(n_mem + 1);
		for (uint64_t o = 0; o < n_mem; ++o) first_l.get()[o] = MG_NONE;
		MgDev V;
		V.mem = T.mem.data(); V.n_mem = n_mem; V.subs = S.data(); V.dels = D.data(); V.inss = I.data(); V.cum = T.cum.data();
		V.flags = flags.get(); V.first_l = first_l.get(); V.b_cnt = b_cnt.get(); V.b_sum = b_sum.get(); V.n_ins = n_ins.get(); V.lead = lead.get();
		V.edge_bad = edge_bad.get(); V.ins_off = ins_off.get();
		const unsigned grid = 1 + rnd(3);                                       // (fewer waves than members: the grid-stride loops are walked)
		emu_launch(dim3(grid), dim3(MG_THREADS), [&] { k_merge_lists(V); });
		emu_launch(dim3(grid), dim3(MG_THREADS), [&] { k_merge_count(V); });
		mg_u64 run = 0;
		for (uint64_t o = 0; o < n_mem; ++o) { ins_off.get()[o] = run; run += n_ins.get()[o]; }   // (stands in for k_merge_scan)
		ins_off.get()[n_mem] = run;
		Exact<pga_sub_t> o_subs(T.n_sub); Exact<pga_del_t> o_dels(T.n_del); Exact<pga_ins_t> o_inss(run); Exact<RowRun> runs(T.n_runs);
		for (size_t r = 0; r < T.n_runs; ++r) runs.get()[r] = RowRun{0xdeadbeefu, 0xdeadbeefu, ~0ULL};
		for (size_t r = 0; r < T.cons_runs.size(); ++r) runs.get()[r] = T.cons_runs[r];
		emu_launch(dim3(grid), dim3(MG_THREADS), [&] { k_merge_write(V, o_subs.get(), o_dels.get(), o_inss.get(), runs.get()); });
		for (size_t r = 0; r < T.n_runs; ++r) if (runs.get()[r].kind == 0xdeadbeefu) { printf("round %d: run %zu was not written\n", round, r); return 1; }
		const uint64_t il = T.ins_lo < T.ins_hi ? T.ins_lo : 0, ih = T.ins_lo < T.ins_hi ? T.ins_hi : 0;
		Exact<char> d_iseq(ih - il), d_cons(T.cons.size()), d_out(T.units * ROW_LETTERS);
		if (ih > il) memcpy(d_iseq.get(), iseq.data() + il, ih - il);
		if (!T.cons.empty()) memcpy(d_cons.get(), T.cons.data(), T.cons.size());
		Exact<uint32_t> row_flags(T.jobs.size());
		if (!T.jobs.empty())
			emu_launch(dim3(2), dim3(ROW_THREADS), [&] { k_rows<false>(T.jobs.data(), (int)T.jobs.size(), 0, T.units, runs.get(), d_cons.get(), d_iseq.get(), il, d_out.get(),
			                                                             row_flags.get(), 0u, nullptr, nullptr, nullptr); });
		std::vector<uint32_t> status(E.size(), 0);
		for (size_t e = 0; e < E.size(); ++e) if (edge_bad.get()[e]) status[e] = 2;
		for (size_t j = 0; j < T.jobs.size(); ++j) if (row_flags.get()[j] & ROW_BAD_COMP) status[T.job_edge[j]] = 2;
		const char *out_cons = d_out.get(), *out_ins = d_out.get() + T.cons_units * ROW_LETTERS;
		// ---- against the direct construction ----
		uint64_t o = 0, p0 = 0, at_s = 0, at_d = 0, at_i = 0;
		for (size_t e = 0; e < E.size(); ++e) {
			const Block &bl = blocks[E[e].left], &br = blocks[E[e].right];
			g_bad = false;
			const uint32_t Ll = (uint32_t)bl.cons.size(), Lr = (uint32_t)br.cons.size();
			const std::string cons = (E[e].left_rc ? revcomp(bl.cons) : bl.cons) + (E[e].right_rc ? revcomp(br.cons) : br.cons);
			if (cons.size() && memcmp(out_cons + T.cons_off[e], cons.data(), cons.size())) { printf("round %d edge %zu: consensus differs\n", round, e); return 1; }
			if (T.member_off[e] != o) { printf("round %d edge %zu: member_off\n", round, e); return 1; }
			for (uint32_t k = 0; k < bl.mem.size(); ++k, ++o) {
				const Member &ml = bl.mem[k], &mr = br.mem[partner[p0 + k]];
				const Member want = edit_concat(E[e].left_rc ? edit_revcomp(ml, Ll) : ml, E[e].right_rc ? edit_revcomp(mr, Lr) : mr, Ll);
				const MgMem &Q = T.mem[o];
				if (Q.o_sub != at_s || Q.o_del != at_d || ins_off.get()[o] != at_i || n_ins.get()[o] != want.inss.size() || Q.row_off % ROW_LETTERS) {
					printf("round %d edge %zu member %u: offsets or the insertion count (%u, expected %zu)\n", round, e, k, n_ins.get()[o], want.inss.size()); return 1;
				}
				for (size_t t = 0; t < want.subs.size(); ++t) if (o_subs.get()[at_s + t].pos != want.subs[t].pos || o_subs.get()[at_s + t].alt != want.subs[t].alt) { printf("round %d edge %zu member %u: substitution %zu\n", round, e, k, t); return 1; }
				for (size_t t = 0; t < want.dels.size(); ++t) if (o_dels.get()[at_d + t].pos != want.dels[t].pos || o_dels.get()[at_d + t].len != want.dels[t].len) { printf("round %d edge %zu member %u: deletion %zu\n", round, e, k, t); return 1; }
				uint64_t next = Q.row_off;
				for (size_t t = 0; t < want.inss.size(); ++t) {
					const pga_ins_t x = o_inss.get()[at_i + t];
					if (x.pos != want.inss[t].first || x.len != want.inss[t].second.size() || x.seq_off != next || (x.len && memcmp(out_ins + x.seq_off, want.inss[t].second.data(), x.len))) {
						printf("round %d edge %zu member %u: insertion %zu (pos %u len %u off %llu; expected pos %u len %zu off %llu)\n", round, e, k, t, x.pos, x.len, (unsigned long long)x.seq_off,
						       want.inss[t].first, want.inss[t].second.size(), (unsigned long long)next); return 1;
					}
					next += x.len;
				}
				at_s += want.subs.size(); at_d += want.dels.size(); at_i += want.inss.size();
				n_slow += (flags.get()[o] & MG_SLOW_INS) != 0; n_boundary += first_l.get()[o] != MG_NONE && b_cnt.get()[o];
				++n_checked;
			}
			if ((status[e] == 2) != g_bad) { printf("round %d edge %zu: status %u, the direct construction says %d\n", round, e, status[e], (int)g_bad); return 1; }
			n_bad += g_bad;
			p0 += bl.mem.size();
		}
		if (at_s != T.n_sub || at_d != T.n_del || at_i != run) { printf("round %d: totals\n", round); return 1; }
	}
	if (n_checked < 300 || n_slow < 50 || n_boundary < 30 || n_bad < 10) { printf("the generator is too tame: %llu members, %llu slow, %llu boundary, %llu bad\n", (unsigned long long)n_checked, (unsigned long long)n_slow, (unsigned long long)n_boundary, (unsigned long long)n_bad); return 1; }
	printf("merge_emu OK: %llu output members (%llu on the slow insertion path, %llu boundary merges), %llu rejected edges\n", (unsigned long long)n_checked, (unsigned long long)n_slow, (unsigned long long)n_boundary, (unsigned long long)n_bad);
	return 0;
}
