// pga_detach_idx.h without a device: the host tables of dt_build_tables, then k_detach_count, the offsets and k_detach_pack under
// dev/emu/hip_emu.h, then k_rows<false> (pga_rows.h) over the orphans' rows, every buffer allocated at exactly the size the kernels may
// touch -- under the address sanitizer an access one entry out is an error -- against a direct scalar construction of
// detach_unaligned_nodes (detach_unaligned.rs:24-114): Edit::aligned_count (edits.rs:439-442), Edit::apply (edits.rs:307-329) letter by
// letter, reverse_complement (io/seq.rs:9-33).  The device's decision is compared with the host's member by member.  The emulator has no
// wave intrinsics: k_detach_scan of pga_detach.hip is NOT run here; a plain loop over dt_scan_value stands in for it.
// Build and run (host only):  g++ -std=c++17 -g -O1 -DPGA_EMU -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined
//                             tests/emu/detach_emu.cpp -o detach_emu && ./detach_emu
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include "../../dev/emu/hip_emu.h"
#include "../../pangraph_amd/csrc/pga_detach_idx.h"

using namespace pga;

typedef std::pair<uint32_t, std::string> Ins;
struct Member { std::vector<pga_sub_t> subs; std::vector<pga_del_t> dels; std::vector<Ins> inss; uint64_t node_id; int reverse; };
struct Block { std::string cons; std::vector<Member> mem; };

template <class T> struct Exact {                                       // n entries, not one more
	std::unique_ptr<T[]> p; size_t n;
	explicit Exact(size_t n_) : p(n_ ? new T[n_]() : nullptr), n(n_) {}
	T *get() { return p.get(); }
};

static std::mt19937 rng(20260412);
static uint32_t rnd(uint32_t n) { return n ? (uint32_t)(rng() % n) : 0u; }
static uint64_t next_node = 1;

static std::string letters(uint32_t n, int bad)                         // bad: 0 none, 1 maybe a letter without a complement or a '-'
{
	std::string s;
	for (uint32_t i = 0; i < n; ++i) s.push_back("ACGTNRY"[rnd(7)]);
	if (bad && n && rnd(10) == 0) s[rnd(n)] = "aX-"[rnd(3)];
	return s;
}

// Edit::apply without the last step (a literal '-' stays and is reported), then the strand
static std::string direct_apply(const std::string &cons, const Member &e, bool &gap, bool &bad)
{
	std::vector<int> q(cons.begin(), cons.end());
	for (auto &s : e.subs) q[s.pos] = (int)(s.alt & 255u);
	for (auto &d : e.dels) for (uint32_t p = d.pos; p < d.pos + d.len; ++p) q[p] = -1;
	std::vector<Ins> ins = e.inss;
	std::stable_sort(ins.begin(), ins.end());
	for (size_t i = ins.size(); i-- > 0;) q.insert(q.begin() + ins[i].first, ins[i].second.begin(), ins[i].second.end());
	std::string s;
	for (int c : q) if (c >= 0) s.push_back((char)c);
	gap = s.find('-') != std::string::npos; bad = false;
	if (!e.reverse) return s;
	std::string r;
	for (size_t i = s.size(); i-- > 0;) { const uint8_t t = h_comp.t[(uint8_t)s[i]]; if (!t) bad = true; r.push_back(t ? (char)t : s[i]); }
	return r;
}

static Member member(int reverse) { Member m; m.node_id = next_node; next_node += 1 + rnd(1000); m.reverse = reverse; return m; }
// n entries in each list over a consensus of L letters, deletions of one letter (their sum stays under L where n < L)
static Member kept_member(uint32_t L, uint32_t n)
{
	Member m = member((int)rnd(2));
	for (uint32_t t = 0; t < n; ++t) {
		m.subs.push_back(pga_sub_t{(t * 2) % L, (uint32_t)"ACGT"[t & 3]});
		m.dels.push_back(pga_del_t{t % L, 1u});
		m.inss.push_back(Ins{t % (L + 1), letters(1 + t % 3, 0)});
	}
	return m;
}
// an unaligned member whose sequence has `len` letters from one insertion at `pos`
static Member orphan(uint32_t L, uint32_t len, uint32_t pos, int reverse)
{
	Member m = member(reverse);
	if (L) m.dels.push_back(pga_del_t{0u, L});
	if (len) m.inss.push_back(Ins{pos, letters(len, 0)});
	return m;
}

static std::vector<Block> edge_batch()
{
	std::vector<Block> B;
	auto blk = [&](uint32_t L) { B.push_back(Block{letters(L, 0), {}}); return &B.back(); };
	Block *b;
	b = blk(20); b->mem = {orphan(20, 5, 0, 0), kept_member(20, 0), kept_member(20, 1)};                       // first
	b = blk(20); b->mem = {kept_member(20, 2), kept_member(20, 0), orphan(20, 7, 20, 1)};                      // last
	b = blk(9);  b->mem = {orphan(9, 3, 4, 0), orphan(9, 0, 0, 1), orphan(9, 2, 9, 1)};                        // all
	b = blk(33); b->mem = {kept_member(33, 3), orphan(33, 1, 0, 1), orphan(33, 1, 33, 0), kept_member(33, 1)}; // two neighbours
	blk(12);                                                                                                    // no member
	b = blk(0);  b->mem = {orphan(0, 0, 0, 0), orphan(0, 6, 0, 1), orphan(0, 0, 0, 1)};                        // cons_len == 0
	b = blk(40);
	{ Member u = member(0); u.dels = {pga_del_t{0, 20}, pga_del_t{20, 20}}; Member k = member(1); k.dels = {pga_del_t{0, 20}, pga_del_t{20, 19}}; b->mem = {u, k}; }
	{ Member u = member(1); u.dels = {pga_del_t{0, 20}, pga_del_t{5, 15}, pga_del_t{0, 5}}; u.subs = {pga_sub_t{30, 'T'}, pga_sub_t{3, 'G'}}; b->mem.push_back(u); }   // the sum, not the union
	b = blk(300); for (uint32_t n : {0u, 1u, 63u, 64u, 65u, 130u}) b->mem.push_back(kept_member(300, n));
	b = blk(200);
	{ Member u = member(1); for (uint32_t t = 0; t < 200; ++t) u.dels.push_back(pga_del_t{t, 1u}); u.inss = {Ins{100, letters(21, 0)}}; b->mem = {kept_member(200, 5), u}; }
	b = blk(64);
	{ const uint32_t lens[] = {0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 4097}; int k = 0;
	  for (uint32_t n : lens) for (int rev = 0; rev < 2; ++rev, ++k) b->mem.push_back(orphan(64, n, k % 3 == 0 ? 0u : k % 3 == 1 ? 31u : 64u, rev)); }
	b = blk(50);
	{ Member u = member(1); u.dels = {pga_del_t{0, 50}}; u.inss = {Ins{50, "ACGTT"}, Ins{0, "GGA"}, Ins{25, "TTTTTTTTTTTTTTTTTTC"}, Ins{25, "AC"}, Ins{0, ""}}; b->mem = {u, kept_member(50, 4)}; }
	return B;
}

static std::vector<Block> random_batch()
{
	static const uint32_t cons_len[] = {0, 1, 15, 16, 17, 31, 32, 33, 100, 300};
	static const uint32_t list_len[] = {0, 0, 1, 2, 3, 5, 63, 64, 65, 130};
	std::vector<Block> B(1 + rnd(8));
	for (Block &b : B) {
		const uint32_t L = cons_len[rnd(10)], depth = rnd(8) == 0 ? 70 : rnd(6);
		b.cons = letters(L, 1);
		for (uint32_t k = 0; k < depth; ++k) {
			Member m = member((int)rnd(2));
			if (L) {
				for (uint32_t t = list_len[rnd(10)]; t-- > 0;) m.subs.push_back(pga_sub_t{rnd(L), (uint32_t)(uint8_t)letters(1, 1)[0]});
				for (uint32_t t = list_len[rnd(10)]; t-- > 0;) { const uint32_t p = rnd(L); m.dels.push_back(pga_del_t{p, rnd(std::min(L - p, 4u) + 1)}); }
				if (rnd(4) == 0) { m.dels.insert(m.dels.begin() + rnd((uint32_t)m.dels.size() + 1), pga_del_t{0u, L}); }
				else if (rnd(6) == 0) { const uint32_t cut = rnd(L + 1); m.dels.push_back(pga_del_t{cut, L - cut}); m.dels.push_back(pga_del_t{0u, cut}); }
			}
			for (uint32_t t = list_len[rnd(10)] % 7; t-- > 0;) m.inss.push_back(Ins{rnd(L + 1), letters(rnd(40), 1)});
			b.mem.push_back(m);
		}
	}
	return B;
}

static uint64_t n_members, n_orphans, n_bad, n_gap, n_rev;

static int run(const std::vector<Block> &blocks, int round)
{
	std::vector<pga_rc_block_t> B; std::vector<pga_rc_member_t> M; std::vector<pga_sub_t> S; std::vector<pga_del_t> D; std::vector<pga_ins_t> I;
	std::vector<pga_detach_member_t> W; std::vector<const Member*> flat; std::vector<uint32_t> blk_of;
	std::string iseq(5, '?');
	for (const Block &b : blocks) {
		B.push_back(pga_rc_block_t{b.cons.data(), (uint32_t)b.cons.size(), (uint32_t)b.mem.size()});
		for (const Member &m : b.mem) {
			M.push_back(pga_rc_member_t{(uint32_t)m.subs.size(), (uint32_t)m.dels.size(), (uint32_t)m.inss.size()});
			W.push_back(pga_detach_member_t{m.node_id, m.reverse, 0});
			flat.push_back(&m); blk_of.push_back((uint32_t)B.size() - 1);
			S.insert(S.end(), m.subs.begin(), m.subs.end()); D.insert(D.end(), m.dels.begin(), m.dels.end());
			for (auto &x : m.inss) { I.push_back(pga_ins_t{x.first, (uint32_t)x.second.size(), (uint64_t)iseq.size()}); iseq += x.second; }
		}
	}
	// ---- the tables ----
	RowGraph G;
	row_graph_init(G, "detach_emu", (int64_t)B.size(), B.data(), M.data(), S.data(), D.data(), I.data(), iseq.data(), true, 1);
	DtTables T;
	dt_build_tables(G, W.data(), 1, T);
	const uint64_t n_mem = G.n_mem, n_orph = T.orphans.size();
	// ---- the "device" ----
	Exact<uint32_t> cons_len(n_mem), unal(n_mem);
	Exact<dt_u64> del_sum(n_mem), off(DT_SCANS * (n_mem + 1));
	for (uint64_t m = 0; m < n_mem; ++m) cons_len.get()[m] = B[blk_of[m]].cons_len;
	DtDev V;
	V.n_mem = n_mem; V.n_blocks_in = B.size(); V.cap_orphans = n_orph;
	V.members = M.data(); V.cons_len = cons_len.get(); V.sub_off = G.sub_off.data(); V.del_off = G.del_off.data(); V.ins_off = G.ins_off.data();
	V.subs = S.data(); V.dels = D.data(); V.inss = I.data(); V.who = W.data();
	V.del_sum = del_sum.get(); V.unal = unal.get(); V.off = off.get();
	const unsigned grid = 1 + rnd(3);                                       // (fewer waves than members: the grid-stride loops are walked)
	emu_launch(dim3(grid), dim3(DT_THREADS), [&] { k_detach_count(V); });
	for (int q = 0; q < DT_SCANS; ++q) {                                    // (stands in for k_detach_scan)
		dt_u64 run = 0;
		for (uint64_t m = 0; m < n_mem; ++m) { off.get()[q * (n_mem + 1) + m] = run; run += dt_scan_value(M[m], unal.get()[m], q); }
		off.get()[q * (n_mem + 1) + n_mem] = run;
		if (run != T.tot[q]) { printf("round %d: total %d: the device %llu, the host %llu\n", round, q, run, (unsigned long long)T.tot[q]); return 1; }
	}
	Exact<pga_rc_member_t> o_mem(n_mem); Exact<pga_sub_t> o_subs(T.tot[DT_SUB]); Exact<pga_del_t> o_dels(T.tot[DT_DEL]); Exact<pga_ins_t> o_inss(T.tot[DT_INS]);
	Exact<int64_t> map(n_mem); Exact<pga_detach_orphan_t> orph(n_orph);
	for (uint64_t m = 0; m < n_mem; ++m) { map.get()[m] = -1; o_mem.get()[m] = pga_rc_member_t{~0u, ~0u, ~0u}; }
	emu_launch(dim3(grid), dim3(DT_THREADS), [&] { k_detach_pack(V, o_mem.get(), o_subs.get(), o_dels.get(), o_inss.get(), map.get(), orph.get()); });
	const RowTable &R = T.rows;
	const uint64_t il = R.ins_lo < R.ins_hi ? R.ins_lo : 0, ih = R.ins_lo < R.ins_hi ? R.ins_hi : 0;
	Exact<char> d_iseq(ih - il), d_cons(R.cons.size()), d_out(R.units * ROW_LETTERS);
	if (ih > il) memcpy(d_iseq.get(), iseq.data() + il, ih - il);
	if (!R.cons.empty()) memcpy(d_cons.get(), R.cons.data(), R.cons.size());
	Exact<uint32_t> row_flags(R.jobs.size());
	if (!R.jobs.empty())
		emu_launch(dim3(2), dim3(ROW_THREADS), [&] { k_rows<false>(R.jobs.data(), (int)R.jobs.size(), 0, R.units, R.runs.data(), d_cons.get(), d_iseq.get(), il, d_out.get(),
		                                                             row_flags.get(), ROW_GAP, nullptr, nullptr, nullptr); });
	std::vector<uint32_t> o_flags(n_orph, 0);
	for (size_t j = 0; j < R.jobs.size(); ++j) o_flags[R.job_row[j]] = row_flags.get()[j];
	// ---- against the direct construction ----
	uint64_t kept = 0, at_s = 0, at_d = 0, at_i = 0, k = 0, n_kept = 0;
	for (uint64_t m = 0; m < n_mem; ++m) { dt_u64 sum = 0; for (auto &d : flat[m]->dels) sum += d.len; n_kept += !(sum >= B[blk_of[m]].cons_len); }
	std::vector<uint32_t> kept_in(B.size(), 0);
	for (uint64_t m = 0; m < n_mem; ++m) {
		const Member &e = *flat[m];
		dt_u64 sum = 0;
		for (auto &d : e.dels) sum += d.len;
		const bool u = sum >= B[blk_of[m]].cons_len;
		if (unal.get()[m] != (uint32_t)u || T.unal[m] != (uint8_t)u || del_sum.get()[m] != sum) { printf("round %d member %llu: the decision (device %u, host %u, direct %d)\n", round, (unsigned long long)m, unal.get()[m], T.unal[m], (int)u); return 1; }
		if (!u) {
			++kept_in[blk_of[m]];
			const pga_rc_member_t c = o_mem.get()[kept];
			if (map.get()[m] != (int64_t)kept || c.n_subs != e.subs.size() || c.n_dels != e.dels.size() || c.n_inss != e.inss.size()) { printf("round %d member %llu: kept record\n", round, (unsigned long long)m); return 1; }
			if ((c.n_subs && memcmp(o_subs.get() + at_s, e.subs.data(), c.n_subs * sizeof(pga_sub_t))) || (c.n_dels && memcmp(o_dels.get() + at_d, e.dels.data(), c.n_dels * sizeof(pga_del_t))) ||
			    (c.n_inss && memcmp(o_inss.get() + at_i, I.data() + G.ins_off[m], c.n_inss * sizeof(pga_ins_t)))) { printf("round %d member %llu: kept lists\n", round, (unsigned long long)m); return 1; }
			at_s += c.n_subs; at_d += c.n_dels; at_i += c.n_inss; ++kept;
			continue;
		}
		bool gap, bad;
		const std::string want = direct_apply(blocks[blk_of[m]].cons, e, gap, bad);
		const pga_detach_orphan_t O = orph.get()[k];
		const pga_rc_member_t c = o_mem.get()[n_kept + k];
		if (map.get()[m] != (int64_t)(n_kept + k) || c.n_subs || c.n_dels || c.n_inss || O.member != m || O.node_id != e.node_id || O.block != B.size() + k || T.orphans[k] != m) { printf("round %d member %llu: orphan record\n", round, (unsigned long long)m); return 1; }
		if (T.len[k] != want.size() || T.cons_off[k] % ROW_LETTERS || (want.size() && memcmp(d_out.get() + T.cons_off[k], want.data(), want.size()))) { printf("round %d member %llu: orphan letters\n", round, (unsigned long long)m); return 1; }
		const int status = (o_flags[k] & ROW_BAD_COMP) ? 2 : (o_flags[k] & ROW_GAP) ? 3 : 0;
		if (status != (bad ? 2 : gap ? 3 : 0)) { printf("round %d member %llu: status %d, the direct construction says bad %d gap %d\n", round, (unsigned long long)m, status, (int)bad, (int)gap); return 1; }
		n_bad += bad; n_gap += gap && !bad; n_rev += e.reverse != 0; ++k;
	}
	if (kept != n_kept || k != n_orph || at_s != T.tot[DT_SUB] || at_d != T.tot[DT_DEL] || at_i != T.tot[DT_INS] || kept_in != T.kept_in) { printf("round %d: totals\n", round); return 1; }
	n_members += n_mem; n_orphans += n_orph;
	return 0;
}

int main()
{
	// XXH64: the two values of the specification, and the stream of id((NodeId(2), "GGGGGGGG"))
	std::vector<uint8_t> buf;
	if (xxh64_bytes((const uint8_t*)"", 0, 0) != 0xEF46DB3751D8E999ULL || xxh64_bytes((const uint8_t*)"a", 1, 0) != 0xD24EC4F1A98C6E5BULL) { printf("XXH64 misses the specification's values\n"); return 1; }
	const uint64_t id = dt_block_id(2, "GGGGGGGG", 8, buf);
	const uint8_t stream[24] = {2, 0, 0, 0, 0, 0, 0, 0, 8, 0, 0, 0, 0, 0, 0, 0, 'G', 'G', 'G', 'G', 'G', 'G', 'G', 'G'};
	if (buf.size() != 24 || memcmp(buf.data(), stream, 24) || id != xxh64_bytes(stream, 24, 0)) { printf("the block id stream\n"); return 1; }
	if (run(edge_batch(), -1)) return 1;
	const uint64_t edge_members = n_members, edge_orphans = n_orphans;
	if (n_bad || n_gap) { printf("the edge batch holds a rejected orphan\n"); return 1; }
	for (int round = 0; round < 40; ++round) if (run(random_batch(), round)) return 1;
	if (n_members < 600 || n_orphans < 150 || n_bad < 5 || n_gap < 5 || n_rev < 50) { printf("the generator is too tame: %llu members, %llu orphans, %llu bad, %llu gap, %llu reverse\n", (unsigned long long)n_members, (unsigned long long)n_orphans, (unsigned long long)n_bad, (unsigned long long)n_gap, (unsigned long long)n_rev); return 1; }
	printf("detach_emu OK: edge batch %llu members (%llu orphans); in all %llu members, %llu orphans (%llu reverse), %llu rejected complements, %llu gaps\n", (unsigned long long)edge_members, (unsigned long long)edge_orphans,
	       (unsigned long long)n_members, (unsigned long long)n_orphans, (unsigned long long)n_rev, (unsigned long long)n_bad, (unsigned long long)n_gap);
	return 0;
}
