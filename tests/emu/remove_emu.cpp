// pga_remove_idx.h without a device: validation and the tables, then every kernel of the header (and the graph checks of pga_topo_idx.h before
// them) under dev/emu/hip_emu.h, with every buffer allocated at exactly the size the kernels may touch (under the address sanitizer an access
// one entry out is an error), against a direct scalar construction of Pangraph::remove_path (pangraph.rs:110-132) for every path that is
// not kept: members dropped one by one, lists appended member after member.
// Build and run (host only):  g++ -std=c++17 -g -O1 -DPGA_EMU -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined
//                             tests/emu/remove_emu.cpp -o remove_emu && ./remove_emu
#include <cstdio>
#include <cstring>
#include <memory>
#include <numeric>
#include <random>
#include <set>
#include <string>
#include "../../dev/emu/hip_emu.h"
#include "../../pangraph_amd/csrc/pga_remove_idx.h"

using namespace pga;

template <class T> struct Exact {                                       // n entries, not one more
	std::unique_ptr<T[]> p; size_t n;
	explicit Exact(size_t n_) : p(n_ ? new T[n_]() : nullptr), n(n_) {}
	T *get() { return p.get(); }
	T &operator[](size_t i) { return p[i]; }
};

static std::mt19937 rng(20261019);
static uint32_t rnd(uint32_t n) { return n ? (uint32_t)(rng() % n) : 0u; }
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "remove_emu: %s:%d: %s (case %d)\n", __FILE__, __LINE__, #c, g_case); return false; } } while (0)
static int g_case = -1;

struct Case {
	std::vector<pga_topo_block_t> B; std::vector<pga_topo_path_t> P; std::vector<pga_topo_node_t> N;
	std::vector<pga_rc_block_t> RB; std::vector<pga_rc_member_t> M; std::vector<pga_sub_t> S; std::vector<pga_del_t> D; std::vector<pga_ins_t> I;
	std::string seq; std::vector<uint8_t> keep;
};
struct Out {
	std::vector<pga_topo_block_t> B; std::vector<pga_topo_path_t> P; std::vector<pga_topo_node_t> N;
	std::vector<pga_rc_member_t> M; std::vector<pga_sub_t> S; std::vector<pga_del_t> D; std::vector<pga_ins_t> I; std::string seq;
	std::vector<long long> mmap; std::vector<int32_t> pmap;
};

// ---------------------------------------------------------------- cases: random blocks on random paths, members with lists of every length
static const uint32_t LENGTHS[] = {0, 0, 0, 1, 2, 63, 64, 65, 130};
static Case generate(uint32_t n_blocks, uint32_t max_depth, uint32_t n_paths, uint32_t filler, uint32_t long_list, uint32_t keep_in)
{
	Case G;
	std::set<uint64_t> ids;
	while (ids.size() < n_blocks) ids.insert(1 + rnd(100000));
	for (uint64_t id : ids) {
		if (rnd(6) == 0) G.B.push_back(pga_topo_block_t{0, 7, 3, 0, 0});                // a dead entry
		G.B.push_back(pga_topo_block_t{id, 40 + rnd(60), 0, 1, 0});
	}
	{ uint64_t last = 0; for (auto &b : G.B) if (b.alive) last = b.block_id; else b.block_id = last; }
	std::vector<std::vector<uint32_t>> walk(n_paths);
	std::vector<uint32_t> alive;
	for (uint32_t b = 0; b < G.B.size(); ++b) if (G.B[b].alive) alive.push_back(b);
	for (uint32_t b : alive) for (uint32_t d = 1 + rnd(max_depth); d; --d) walk[rnd(n_paths)].push_back(b);
	for (uint32_t f = 0; f < filler; ++f) walk[f % 2 ? 0 : n_paths - 1].push_back(alive[rnd((uint32_t)alive.size())]);
	uint64_t nid = 1000;
	for (uint32_t p = 0; p < n_paths; ++p) {
		if (p == 1) walk[p].clear();                                                      // an empty path
		std::shuffle(walk[p].begin(), walk[p].end(), rng);
		pga_topo_path_t P{10 + 3 * (uint64_t)p, G.N.size(), (uint32_t)walk[p].size(), (int32_t)rnd(2)};
		uint64_t at = 1000 * (uint64_t)p;
		for (uint32_t b : walk[p]) { G.N.push_back(pga_topo_node_t{++nid, at, at + G.B[b].cons_len, b, G.B[b].depth++, (int32_t)rnd(2), 0}); at += G.B[b].cons_len + 1; }
		G.P.push_back(P);
		G.keep.push_back((uint8_t)(rnd(keep_in) ? 0 : 1 + rnd(200)));
	}
	if (filler) { G.keep[0] = 0; G.keep[n_paths - 1] = 1; }                                  // half of the filler goes, half stays
	std::vector<std::vector<uint32_t>> perm(G.B.size());
	for (size_t b = 0; b < G.B.size(); ++b) { perm[b].resize(G.B[b].alive ? G.B[b].depth : 0); std::iota(perm[b].begin(), perm[b].end(), 0u); std::shuffle(perm[b].begin(), perm[b].end(), rng); }
	for (auto &n : G.N) n.member = perm[n.block][n.member];
	static const char pool[] = "ACGTACGTTGCA";
	G.seq.assign(200 + rnd(100), 'A');
	for (char &c : G.seq) c = pool[rnd(12)];
	for (size_t b = 0; b < G.B.size(); ++b) {
		G.RB.push_back(pga_rc_block_t{pool + b % 5, G.B[b].cons_len, G.B[b].alive ? G.B[b].depth : 0u});
		for (uint32_t m = 0; G.B[b].alive && m < G.B[b].depth; ++m) {
			pga_rc_member_t X{LENGTHS[rnd(9)], LENGTHS[rnd(9)], LENGTHS[rnd(9)]};
			if (long_list && G.M.size() % 7 == 3) { X.n_subs = long_list + rnd(9); X.n_inss = long_list / 2 + rnd(9); }
			for (uint32_t k = 0; k < X.n_subs; ++k) G.S.push_back(pga_sub_t{rnd(100), 'A' + rnd(20)});
			for (uint32_t k = 0; k < X.n_dels; ++k) G.D.push_back(pga_del_t{rnd(100), rnd(7)});
			for (uint32_t k = 0; k < X.n_inss; ++k) { const uint32_t len = rnd(5) ? rnd(41) : 0; G.I.push_back(pga_ins_t{rnd(100), len, rnd((uint32_t)G.seq.size() - len + 1)}); }
			G.M.push_back(X);
		}
	}
	return G;
}

// ---------------------------------------------------------------- the direct construction
static Out direct(const Case &G, uint32_t flags)
{
	Out D;
	std::vector<uint64_t> first(G.B.size() + 1, 0);
	for (size_t b = 0; b < G.B.size(); ++b) first[b + 1] = first[b] + G.RB[b].n_members;
	std::vector<int> kept(G.M.size(), 0);
	for (size_t p = 0; p < G.P.size(); ++p) for (uint64_t i = G.P[p].node_off; i < G.P[p].node_off + G.P[p].n_nodes; ++i) kept[first[G.N[i].block] + G.N[i].member] = G.keep[p] ? 1 : 0;
	uint64_t s = 0, d = 0, x = 0;
	std::vector<uint32_t> rank(G.M.size(), 0);
	for (size_t b = 0; b < G.B.size(); ++b) {
		uint32_t n = 0;
		for (uint64_t m = first[b]; m < first[b + 1]; ++m) {
			const pga_rc_member_t &X = G.M[m];
			if (kept[m]) {
				rank[m] = n++;
				D.mmap.push_back((long long)D.M.size()); D.M.push_back(X);
				D.S.insert(D.S.end(), G.S.begin() + s, G.S.begin() + s + X.n_subs); D.D.insert(D.D.end(), G.D.begin() + d, G.D.begin() + d + X.n_dels);
				for (uint64_t k = x; k < x + X.n_inss; ++k) {
					pga_ins_t I = G.I[k];
					if (flags & PGA_REMOVE_COMPACT_LETTERS) { I.seq_off = D.seq.size(); D.seq += G.seq.substr(G.I[k].seq_off, I.len); }
					D.I.push_back(I);
				}
			} else D.mmap.push_back(-1);
			s += X.n_subs; d += X.n_dels; x += X.n_inss;
		}
		const bool alive = G.B[b].alive && (n || G.B[b].depth == 0);
		D.B.push_back(alive ? pga_topo_block_t{G.B[b].block_id, G.B[b].cons_len, n, 1, 0} : pga_topo_block_t{G.B[b].block_id, 0, 0, 0, 0});
	}
	for (size_t p = 0; p < G.P.size(); ++p) {
		if (!G.keep[p]) { D.pmap.push_back(-1); continue; }
		D.pmap.push_back((int32_t)D.P.size());
		D.P.push_back(pga_topo_path_t{G.P[p].path_id, D.N.size(), G.P[p].n_nodes, G.P[p].circular});
		for (uint64_t i = G.P[p].node_off; i < G.P[p].node_off + G.P[p].n_nodes; ++i) { pga_topo_node_t A = G.N[i]; A.member = rank[first[A.block] + A.member]; D.N.push_back(A); }
	}
	return D;
}

// ---------------------------------------------------------------- the kernels in the order of pga_remove.hip
struct ScanBufs {
	Exact<rm_u64> tile_sum, tile_off, off; RmScan S;
	ScanBufs(uint64_t n, uint32_t n_q) : tile_sum((size_t)n_q * ((n + RM_TILE - 1) / RM_TILE)), tile_off((size_t)n_q * ((n + RM_TILE - 1) / RM_TILE + 1)), off((size_t)n_q * (n + 1)),
		S{n, (uint32_t)((n + RM_TILE - 1) / RM_TILE), n_q, tile_sum.get(), tile_off.get(), off.get()} {}
};
template <class Val> static void scan(const RmScan &S, const Val &val, unsigned grid)
{
	if (S.n_tiles) emu_launch(dim3(std::min<unsigned>(grid, S.n_tiles)), dim3(RM_THREADS), [&] { k_ts_sums<rm_u64, Val>(S, val); });
	emu_launch(dim3(1), dim3(RM_THREADS), [&] { k_ts_scan<rm_u64>(S); });
	if (S.n_tiles) emu_launch(dim3(std::min<unsigned>(grid, S.n_tiles)), dim3(RM_THREADS), [&] { k_ts_offsets<rm_u64, Val>(S, val); });
}

// returns false on a CHECK; `refused` says whether the device checks stopped the call (nothing behind them has run then)
static bool emulated(const Case &G, unsigned grid, uint32_t flags, bool null_seq, uint64_t seq_len, Out &O, uint32_t terr[TP_ERRS], rm_u64 err[RM_ERRS], bool &refused)
{
	RmTables R;
	rm_validate((int64_t)G.B.size(), G.B.data(), (int64_t)G.P.size(), G.P.data(), (int64_t)G.N.size(), G.N.data(), G.RB.data(), G.M.data(), G.S.data(), G.D.data(), G.I.data(), G.keep.data(), flags, R);
	const uint64_t nn = G.N.size(), np = G.P.size(), nb = G.B.size(), nm = R.n_members;
	refused = false;
	CHECK(nm == G.M.size() && R.n_subs == G.S.size() && R.n_dels == G.D.size() && R.n_inss == G.I.size());
	Exact<pga_topo_node_t> nodes(nn), onodes(R.n_out_nodes); Exact<pga_topo_path_t> paths(np); Exact<pga_topo_block_t> blocks(nb), oblocks(nb);
	Exact<uint32_t> depth(nb), first(nb + 1), mkeep(nm), pathof(nn), slot_cnt(nm), blk_cnt(nb), te(TP_ERRS); Exact<uint8_t> keep(np); Exact<rm_u64> newoff(np), e(RM_ERRS);
	Exact<pga_rc_member_t> members(nm); Exact<pga_sub_t> subs(G.S.size()); Exact<pga_del_t> dels(G.D.size()); Exact<pga_ins_t> inss(G.I.size()); Exact<char> seq(null_seq ? 0 : seq_len);
	Exact<tp_u64> key(nn);
	std::copy(G.N.begin(), G.N.end(), nodes.get()); std::copy(G.P.begin(), G.P.end(), paths.get()); std::copy(G.B.begin(), G.B.end(), blocks.get());
	std::copy(R.T.depth.begin(), R.T.depth.end(), depth.get()); std::copy(R.T.slot_first.begin(), R.T.slot_first.end(), first.get());
	std::copy(G.keep.begin(), G.keep.end(), keep.get()); std::copy(R.path_new_off.begin(), R.path_new_off.end(), newoff.get());
	std::copy(G.M.begin(), G.M.end(), members.get()); std::copy(G.S.begin(), G.S.end(), subs.get()); std::copy(G.D.begin(), G.D.end(), dels.get()); std::copy(G.I.begin(), G.I.end(), inss.get());
	if (!null_seq) std::copy(G.seq.begin(), G.seq.begin() + seq_len, seq.get());
	std::fill(te.get(), te.get() + TP_ERRS, TP_NONE); std::fill(e.get(), e.get() + RM_ERRS, RM_NONE);
	TpDev T;
	memset(&T, 0, sizeof(T));
	T.n_nodes = nn; T.n_paths = np; T.n_blocks = nb; T.n_slots = nm;
	T.nodes = nodes.get(); T.paths = paths.get(); T.depth = depth.get(); T.slot_first = first.get(); T.path_of = pathof.get(); T.key = key.get();
	T.slot_cnt = slot_cnt.get(); T.blk_cnt = blk_cnt.get(); T.err = te.get();
	ScanBufs b_mem(nm, RM_QS);
	RmDev V;
	memset(&V, 0, sizeof(V));
	V.n_nodes = nn; V.n_paths = np; V.n_blocks = nb; V.n_members = nm; V.ins_seq_len = seq_len; V.flags = flags;
	V.nodes = nodes.get(); V.paths = paths.get(); V.blocks = blocks.get(); V.slot_first = first.get(); V.path_of = pathof.get(); V.keep = keep.get(); V.path_new_off = newoff.get();
	V.members = members.get(); V.subs = subs.get(); V.dels = dels.get(); V.inss = inss.get(); V.ins_seq = null_seq ? nullptr : seq.get();
	V.mkeep = mkeep.get(); V.err = e.get(); V.scan[RM_SCAN_MEMBERS] = b_mem.S;
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_keys(T); });
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_check(T); });
	emu_launch(dim3(grid), dim3(RM_THREADS), [&] { k_remove_mark(V); });
	scan(V.scan[RM_SCAN_MEMBERS], RmMemberValue{V}, grid);
	std::copy(te.get(), te.get() + TP_ERRS, terr); std::copy(e.get(), e.get() + RM_ERRS, err);
	for (int i = 0; i < TP_ERRS; ++i) if (terr[i] != TP_NONE) { refused = true; return true; }
	const rm_u64 *tot = b_mem.off.get();
	auto total = [&](int q) { return tot[(size_t)q * (nm + 1) + nm]; };
	CHECK(total(RM_Q_IN_SUB) == R.n_subs && total(RM_Q_IN_DEL) == R.n_dels && total(RM_Q_IN_INS) == R.n_inss);
	const uint64_t nm_out = total(RM_Q_KEPT), ns_out = total(RM_Q_OUT_SUB), nd_out = total(RM_Q_OUT_DEL), ni_out = total(RM_Q_OUT_INS);
	Exact<pga_rc_member_t> omembers(nm_out); Exact<pga_sub_t> osubs(ns_out); Exact<pga_del_t> odels(nd_out); Exact<pga_ins_t> oinss(ni_out); Exact<long long> map(nm);
	V.o_blocks = oblocks.get(); V.o_nodes = onodes.get(); V.o_members = omembers.get(); V.o_subs = osubs.get(); V.o_dels = odels.get(); V.o_inss = oinss.get(); V.member_map = map.get();
	emu_launch(dim3(grid), dim3(RM_THREADS), [&] { k_remove_blocks(V); });
	emu_launch(dim3(grid), dim3(RM_THREADS), [&] { k_remove_members(V); });
	emu_launch(dim3(grid), dim3(RM_THREADS), [&] { k_remove_nodes(V); });
	if (ns_out) emu_launch(dim3(grid), dim3(RM_THREADS), [&] { k_remove_copy<RM_LIST_SUB>(V); });
	if (nd_out) emu_launch(dim3(grid), dim3(RM_THREADS), [&] { k_remove_copy<RM_LIST_DEL>(V); });
	if (ni_out) emu_launch(dim3(grid), dim3(RM_THREADS), [&] { k_remove_copy<RM_LIST_INS>(V); });
	ScanBufs b_let(ni_out, 1);
	uint64_t nl_out = 0;
	std::unique_ptr<Exact<char>> oseq;
	if (flags & PGA_REMOVE_COMPACT_LETTERS) {
		V.scan[RM_SCAN_LETTERS] = b_let.S;
		scan(V.scan[RM_SCAN_LETTERS], RmLetterValue{V}, grid);
		std::copy(e.get(), e.get() + RM_ERRS, err);
		for (int i = 0; i < RM_ERRS; ++i) if (err[i] != RM_NONE) { refused = true; return true; }
		nl_out = b_let.off[ni_out];
		oseq.reset(new Exact<char>(nl_out));
		V.o_ins_seq = oseq->get();
		if (nl_out) emu_launch(dim3(grid), dim3(RM_THREADS), [&] { k_remove_letters(V); });
		if (ni_out) emu_launch(dim3(grid), dim3(RM_THREADS), [&] { k_remove_seq_off(V); });
	}
	O.B.assign(oblocks.get(), oblocks.get() + nb); O.P = R.o_paths; O.N.assign(onodes.get(), onodes.get() + onodes.n);
	O.M.assign(omembers.get(), omembers.get() + nm_out); O.S.assign(osubs.get(), osubs.get() + ns_out); O.D.assign(odels.get(), odels.get() + nd_out);
	O.I.assign(oinss.get(), oinss.get() + ni_out); O.mmap.assign(map.get(), map.get() + nm); O.pmap = R.path_map;
	if (nl_out) O.seq.assign(oseq->get(), nl_out);
	return true;
}

template <class T> static bool same(const std::vector<T> &a, const std::vector<T> &b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }

static bool run_case(const Case &G, unsigned grid, uint32_t flags)
{
	Out E, D = direct(G, flags);
	uint32_t terr[TP_ERRS]; rm_u64 err[RM_ERRS]; bool refused;
	if (!emulated(G, grid, flags, false, G.seq.size(), E, terr, err, refused)) return false;
	CHECK(!refused);
	CHECK(same(E.B, D.B)); CHECK(same(E.P, D.P)); CHECK(same(E.N, D.N)); CHECK(same(E.M, D.M)); CHECK(same(E.S, D.S)); CHECK(same(E.D, D.D)); CHECK(same(E.I, D.I));
	CHECK(E.seq == D.seq); CHECK(same(E.mmap, D.mmap)); CHECK(same(E.pmap, D.pmap));
	return true;
}

template <class F> static bool refused_by_host(F f) { try { f(); } catch (std::runtime_error &) { return true; } return false; }

int main()
{
	size_t n_big = 0, n_dies = 0, n_removed = 0, n_long = 0;
	for (g_case = 0; g_case < 6; ++g_case) {
		const int kind = g_case;                          // 3: more than one tile of members; 4: lists of several tiles
		const Case G = kind == 3 ? generate(30, 12, 5, 2 * RM_TILE + rnd(50), 0, 2) : kind == 4 ? generate(6, 4, 3, 0, 2 * RM_TILE + 5, 2)
		             : generate(4 + rnd(8), 4, 2 + rnd(4), 0, 0, g_case == 0 ? 1 : g_case == 1 ? 1000000 : 2);
		if (!run_case(G, 1 + rnd(3), (uint32_t)(g_case & 1)) || ((kind == 2 || kind == 4) && !run_case(G, 2, (uint32_t)(~g_case & 1)))) return 1;
		const Out D = direct(G, 0);
		n_big += G.M.size() > (size_t)RM_TILE; n_long += G.S.size() > (size_t)2 * RM_TILE;
		for (size_t b = 0; b < G.B.size(); ++b) n_dies += G.B[b].alive && !D.B[b].alive;
		for (long long m : D.mmap) n_removed += m < 0;
	}
	if (n_big < 1 || n_dies < 5 || n_removed < 100 || n_long < 1) {
		fprintf(stderr, "remove_emu: the generator lost its cases (%zu big, %zu blocks die, %zu members removed, %zu long lists)\n", n_big, n_dies, n_removed, n_long);
		return 1;
	}
	// ---- what is refused: on the host, and by the kernels before an index is derived
	g_case = -2;
	Case H;
	auto fits = [](const Case &Y) {                       // a kept insertion with letters, two nodes in one block, a dead block
		bool kept_ins = false, dead = false;
		std::vector<uint64_t> first(Y.B.size() + 1, 0);
		for (size_t b = 0; b < Y.B.size(); ++b) { first[b + 1] = first[b] + Y.RB[b].n_members; dead = dead || !Y.B[b].alive; }
		std::vector<uint64_t> ioff(Y.M.size() + 1, 0);
		for (size_t m = 0; m < Y.M.size(); ++m) ioff[m + 1] = ioff[m] + Y.M[m].n_inss;
		for (size_t p = 0; p < Y.P.size(); ++p) if (Y.keep[p]) for (uint64_t i = Y.P[p].node_off; i < Y.P[p].node_off + Y.P[p].n_nodes; ++i) {
			const uint64_t m = first[Y.N[i].block] + Y.N[i].member;
			for (uint64_t k = ioff[m]; k < ioff[m + 1]; ++k) kept_ins = kept_ins || Y.I[k].len;
		}
		size_t i = 1; while (i < Y.N.size() && Y.N[i].block != Y.N[0].block) ++i;
		return kept_ins && dead && i < Y.N.size() && Y.keep[0];
	};
	do H = generate(10, 4, 3, 0, 0, 2); while (!fits(H));
	auto host = [&](const Case &X, uint32_t flags, bool null_keep = false, bool null_members = false) {
		RmTables R;
		rm_validate((int64_t)X.B.size(), X.B.data(), (int64_t)X.P.size(), X.P.data(), (int64_t)X.N.size(), X.N.data(), X.RB.data(), null_members ? nullptr : X.M.data(), X.S.data(), X.D.data(), X.I.data(),
		            null_keep ? nullptr : X.keep.data(), flags, R);
	};
	host(H, 1);
	bool ok = true;
	size_t dead = 0; while (H.B[dead].alive) ++dead;
	Case X = H; X.N[0].member = X.B[X.N[0].block].depth;               ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.N[0].block = (uint32_t)X.B.size();                        ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.N[0].block = (uint32_t)dead;                              ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.P[1].node_off += 1;                                       ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.P[2].path_id = X.P[0].path_id;                            ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.RB[X.N[0].block].n_members += 1;                          ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.RB[dead].n_members = 1;                                   ok = ok && refused_by_host([&] { host(X, 0); });
	X = H;                                                             ok = ok && refused_by_host([&] { host(X, 2); });
	X = H;                                                             ok = ok && refused_by_host([&] { host(X, 0, true); });
	X = H;                                                             ok = ok && refused_by_host([&] { host(X, 0, false, true); });
	X = H; X.P.clear(); X.N.clear(); X.keep.clear();                   ok = ok && refused_by_host([&] { host(X, 0); });   // members, and no path to hold them
	if (!ok) { fprintf(stderr, "remove_emu: malformed input was accepted by the host\n"); return 1; }
	auto device = [&](const Case &Y, uint32_t flags, bool null_seq, uint64_t seq_len, int which) {
		Out E; uint32_t terr[TP_ERRS]; rm_u64 err[RM_ERRS]; bool refused;
		if (!emulated(Y, 2, flags, null_seq, seq_len, E, terr, err, refused)) return false;
		return refused && (which < 0 ? terr[-which - 1] != TP_NONE : err[which] != RM_NONE) && E.N.empty() && E.M.empty();
	};
	{ X = H; size_t i = 1; while (X.N[i].block != X.N[0].block) ++i; X.N[i].member = X.N[0].member; ok = ok && device(X, 0, false, X.seq.size(), -(TP_E_SLOT + 1)); }
	{ X = H; X.B[X.N[0].block].depth += 1; X.RB[X.N[0].block].n_members += 1; X.M.push_back(pga_rc_member_t{0, 0, 0}); ok = ok && device(X, 0, false, X.seq.size(), -(TP_E_DEPTH + 1)); }
	ok = ok && device(H, 1, true, H.seq.size(), RM_E_INS_NULL);
	ok = ok && device(H, 1, false, 3, RM_E_INS_RANGE);
	{ X = H; for (auto &I : X.I) I.seq_off = ~0ULL - 2; ok = ok && device(X, 1, false, X.seq.size(), RM_E_INS_RANGE); }      // (seq_off + len wraps)
	{ Out E; uint32_t terr[TP_ERRS]; rm_u64 err[RM_ERRS]; bool refused; ok = ok && emulated(H, 2, 0, true, 0, E, terr, err, refused) && !refused && same(E.I, direct(H, 0).I); }   // without the flag the letters are not needed
	if (!ok) { fprintf(stderr, "remove_emu: malformed input passed the kernels' checks\n"); return 1; }
	// ---- no path at all, and the lookup at its edges
	{ Case Z; Z.B.push_back(pga_topo_block_t{5, 9, 0, 0, 0}); Z.RB.push_back(pga_rc_block_t{nullptr, 9, 0}); RmTables R;
	  rm_validate(1, Z.B.data(), 0, nullptr, 0, nullptr, Z.RB.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 0, R); if (R.n_out_nodes || R.n_members) return 1; }
	const rm_u64 offs[6] = {0, 2, 2, 2, 5, 5};
	if (ts_last_le(offs, 0, 5, 0) != 0 || ts_last_le(offs, 0, 5, 1) != 0 || ts_last_le(offs, 0, 5, 2) != 3 || ts_last_le(offs, 0, 5, 4) != 3 || ts_last_le(offs, 3, 4, 4) != 3) { fprintf(stderr, "remove_emu: a lookup is off\n"); return 1; }
	printf("remove_emu OK (%zu graphs of more than one tile, %zu blocks die, %zu members removed, %zu with long lists)\n", n_big, n_dies, n_removed, n_long);
	return 0;
}
