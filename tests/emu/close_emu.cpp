// pga_close_idx.h without a device: validation and the tables, then every kernel of the header (and the copies of pga_assemble_idx.h it
// drives) under dev/emu/hip_emu.h, with every buffer allocated at exactly the size the kernels may touch (under the address sanitizer an
// access one entry out is an error), against a direct scalar construction: the fate of every member followed through the two member_maps,
// the blocks after sorted by id, block after block, slot after slot, every list appended from where the member has it.
// Every file named on the command line is a named case of tests/close_gen.py (close_gen.dump: the tables of the call and host_close's
// expectation); it goes through the same kernels and is held against both the scalar construction and that expectation.
// The random instances are made here: a flat graph with dead entries, some blocks updated, members leaving in either stage, block kinds 0 / 1 / 2,
// singleton ids below, between and above the survivors'.  The singleton ids are sorted with std::sort where the device uses rocPRIM.
// Build and run (host only):  g++ -std=c++17 -g -O1 -DPGA_EMU -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined
//                             tests/emu/close_emu.cpp -o close_emu && ./close_emu [case files]
#include <cstdio>
#include <cstring>
#include <memory>
#include <numeric>
#include <random>
#include <set>
#include <string>
#include "../../dev/emu/hip_emu.h"
#include "../../pangraph_amd/csrc/pga_close_idx.h"

using namespace pga;

template <class T> struct Exact {                                       // n entries, not one more
	std::unique_ptr<T[]> p; size_t n;
	explicit Exact(size_t n_) : p(n_ ? new T[n_]() : nullptr), n(n_) {}
	template <class V> explicit Exact(const V &v) : Exact(v.size()) { std::copy(v.begin(), v.end(), p.get()); }
	T *get() { return p.get(); }
	T &operator[](size_t i) { return p[i]; }
	void fill(int byte) { if (n) memset(p.get(), byte, n * sizeof(T)); }
};

static std::mt19937 rng(20261021);
static uint32_t rnd(uint32_t n) { return n ? (uint32_t)(rng() % n) : 0u; }
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "close_emu: %s:%d: %s (case %d)\n", __FILE__, __LINE__, #c, g_case); return false; } } while (0)
static int g_case = -1;
static const char CONS[] = "ACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCA";

struct Lists { std::vector<pga_sub_t> S; std::vector<pga_del_t> D; std::vector<pga_ins_t> I; };
struct Case {
	std::vector<pga_topo_block_t> GB; std::vector<pga_topo_path_t> GP; std::vector<pga_topo_node_t> GN;
	std::vector<pga_rc_block_t> RB; std::vector<pga_rc_member_t> M; Lists B; std::string seq, rc_seq;
	std::vector<pga_detach_member_t> who; std::vector<uint32_t> upd;
	std::vector<pga_rc_block_t> B1, B2; std::vector<int64_t> map1, map2; std::vector<pga_detach_orphan_t> O1, O2;
	std::vector<pga_rc_block_res_t> RCB; std::vector<pga_mapvar_res_t> RCM; std::vector<pga_rc_member_t> M2; Lists L2;
	pga_detach_out_t d1() const { return pga_detach_out_t{(int64_t)B1.size(), (int64_t)O1.size(), (pga_rc_block_t*)B1.data(), nullptr, nullptr, nullptr, nullptr, nullptr, (int64_t*)map1.data(), (pga_detach_orphan_t*)O1.data()}; }
	pga_detach_out_t d2() const { return pga_detach_out_t{(int64_t)B2.size(), (int64_t)O2.size(), (pga_rc_block_t*)B2.data(), (pga_rc_member_t*)M2.data(), (pga_sub_t*)L2.S.data(), (pga_del_t*)L2.D.data(), (pga_ins_t*)L2.I.data(), nullptr, (int64_t*)map2.data(), (pga_detach_orphan_t*)O2.data()}; }
	pga_rc_out_t rc() const { pga_rc_out_t r; memset(&r, 0, sizeof(r)); r.blocks = (pga_rc_block_res_t*)RCB.data(); r.members = (pga_mapvar_res_t*)RCM.data(); r.cons = (char*)CONS; r.ins_seq = (char*)rc_seq.data(); return r; }
};
struct Out {
	std::vector<pga_topo_block_t> GB; std::vector<pga_topo_node_t> GN; std::vector<ClBlock> rec;
	std::vector<pga_rc_member_t> M; Lists L; std::string seq;
	std::vector<pga_detach_member_t> who; std::vector<long long> origin; std::vector<uint32_t> bmap; std::vector<pga_detach_orphan_t> orph;
};

static const uint32_t LENGTHS[] = {0, 0, 0, 1, 2, 63, 64, 65, 130};
static pga_rc_member_t add_lists(Lists &L, uint32_t seq_len, uint32_t long_list)
{
	pga_rc_member_t X{LENGTHS[rnd(9)], LENGTHS[rnd(9)], LENGTHS[rnd(9)]};
	if (long_list) { X.n_subs = long_list + rnd(9); X.n_inss = long_list / 2 + rnd(9); }
	for (uint32_t k = 0; k < X.n_subs; ++k) L.S.push_back(pga_sub_t{rnd(100), 'A' + rnd(20)});
	for (uint32_t k = 0; k < X.n_dels; ++k) L.D.push_back(pga_del_t{rnd(100), rnd(7)});
	static const uint32_t EDGES[] = {1, 63, 64, 65, 127, 128};
	for (uint32_t k = 0; k < X.n_inss; ++k) { const uint32_t len = rnd(5) == 0 ? 0 : rnd(9) == 0 ? EDGES[rnd(6)] : rnd(41); L.I.push_back(pga_ins_t{rnd(100), len, rnd(seq_len - len + 1)}); }
	return X;
}

// upd_one_in: one alive block in so many is updated; leave_one_in: a member leaves in a stage with that chance (0: nobody leaves)
// force_depth: block 1 is alive, has exactly so many members and is updated (0: as it comes); force_before: the members of block 0 then
static Case generate(uint32_t n_blocks, uint32_t max_depth, uint32_t upd_one_in, uint32_t leave_one_in, uint32_t long_list, uint32_t force_depth = 0, uint32_t force_before = 0)
{
	Case G;
	static const char pool[] = "ACGTACGTTGCA";
	G.seq.assign(5000 + rnd(100), 'A'); G.rc_seq.assign(300 + rnd(100), 'A');
	for (char &c : G.seq) c = pool[rnd(12)];
	for (char &c : G.rc_seq) c = pool[rnd(12)];
	std::set<uint64_t> id_set;
	while (id_set.size() < n_blocks) id_set.insert(((uint64_t)rng() << 32 | rng()) >> (rnd(3) ? 0 : 20) | (rnd(3) ? 0 : 1ULL << 63));
	std::vector<uint64_t> ids(id_set.begin(), id_set.end());
	uint64_t nid = 1000;
	std::vector<std::pair<uint32_t, uint32_t>> slots;
	for (uint32_t b = 0; b < n_blocks; ++b) {
		const bool dead = rnd(7) == 0 && !(force_depth && b < 2);
		const uint32_t n = dead ? 0 : force_depth && b == 1 ? force_depth : force_depth && b == 0 ? force_before : rnd(max_depth + 1);
		G.GB.push_back(pga_topo_block_t{ids[b], dead ? 0u : 40 + rnd(60), n, dead ? 0 : 1, 0});
		G.RB.push_back(pga_rc_block_t{CONS + rnd(8), G.GB[b].cons_len, n});
		for (uint32_t m = 0; m < n; ++m) {
			G.M.push_back(add_lists(G.B, (uint32_t)G.seq.size(), long_list && G.M.size() % 7 == 3 ? long_list : 0));
			nid += 1 + rnd(5);
			G.who.push_back(pga_detach_member_t{nid, (int32_t)rnd(2), 0});
			slots.push_back({b, m});
		}
	}
	std::vector<uint32_t> first(n_blocks + 1, 0);
	for (uint32_t b = 0; b < n_blocks; ++b) first[b + 1] = first[b] + G.GB[b].depth;
	std::shuffle(slots.begin(), slots.end(), rng);
	for (size_t i = 0; i < slots.size();) {
		const uint32_t n = std::min<size_t>(rnd(6), slots.size() - i);
		G.GP.push_back(pga_topo_path_t{10 + G.GP.size(), i, n, (int32_t)rnd(2)});
		for (uint32_t k = 0; k < n; ++k, ++i) {
			const pga_detach_member_t &W = G.who[first[slots[i].first] + slots[i].second];
			G.GN.push_back(pga_topo_node_t{W.node_id, rnd(1000), rnd(1000), slots[i].first, slots[i].second, W.reverse, 0});
		}
	}
	for (uint32_t b = 0; b < n_blocks; ++b) if (G.GB[b].alive && (force_depth ? b == 1 || (b > 1 && rnd(upd_one_in) == 0) : rnd(upd_one_in) == 0)) G.upd.push_back(b);
	std::shuffle(G.upd.begin(), G.upd.end(), rng);
	const size_t nu = G.upd.size();
	// ---- new ids for the singletons: unique, below, between and above the survivors'
	std::set<uint64_t> fresh;
	auto new_id = [&]() { for (;;) { const uint64_t x = rnd(8) == 0 ? rnd(4) : rnd(8) == 0 ? ~0ULL - rnd(4) : ((uint64_t)rng() << 32 | rng()); if (!id_set.count(x) && fresh.insert(x).second) return x; } };
	// ---- the first stage
	uint64_t m = 0;
	std::vector<int> gone1;
	for (size_t j = 0; j < nu; ++j) for (uint32_t s = 0; s < G.GB[G.upd[j]].depth; ++s) gone1.push_back(leave_one_in && rnd(leave_one_in) == 0);
	const uint64_t nm1 = gone1.size(), k1 = nm1 - std::accumulate(gone1.begin(), gone1.end(), 0);
	G.map1.resize(nm1);
	uint64_t kept_at = 0;
	for (size_t j = 0; j < nu; ++j) {
		uint32_t kept = 0;
		for (uint32_t s = 0; s < G.GB[G.upd[j]].depth; ++s, ++m) {
			if (!gone1[m]) { G.map1[m] = (int64_t)kept_at++; ++kept; continue; }
			G.map1[m] = (int64_t)(k1 + G.O1.size());
			G.O1.push_back(pga_detach_orphan_t{m, G.who[first[G.upd[j]] + s].node_id, new_id(), (uint32_t)(nu + G.O1.size()), rnd(4) ? rnd(50) : 0u, 0, 0});
		}
		G.B1.push_back(pga_rc_block_t{G.RB[G.upd[j]].consensus, G.RB[G.upd[j]].cons_len, kept});
	}
	for (const auto &O : G.O1) G.B1.push_back(pga_rc_block_t{CONS + rnd(8), O.len, 1});
	// ---- the reconsensus and the second stage
	uint64_t kept2_at = 0, m1 = 0;
	std::vector<int> gone2;
	for (size_t j = 0; j < nu; ++j) {
		const int kind = (int)rnd(3);
		G.RCB.push_back(pga_rc_block_res_t{kind, kind ? 30 + rnd(70) : G.RB[G.upd[j]].cons_len, rnd(8), 0, 0, 0, 0, 0, 0});
		for (uint32_t s = 0; s < G.B1[j].n_members; ++s) gone2.push_back(kind == 2 && leave_one_in && rnd(leave_one_in) == 0);
	}
	const uint64_t k2 = k1 - std::accumulate(gone2.begin(), gone2.end(), 0);
	G.map2.resize(k1); G.RCM.resize(k1);
	for (auto &R : G.RCM) memset(&R, 0, sizeof(R));
	for (size_t j = 0; j < nu; ++j) {
		uint32_t kept = 0;
		for (uint32_t s = 0; s < G.B1[j].n_members; ++s, ++m1) {
			if (!gone2[m1]) { G.map2[m1] = (int64_t)kept2_at++; ++kept; G.M2.push_back(add_lists(G.L2, (uint32_t)G.rc_seq.size(), long_list && m1 % 5 == 1 ? long_list : 0)); continue; }
			G.map2[m1] = (int64_t)(k2 + G.O2.size());
			uint64_t src = 0; while ((uint64_t)G.map1[src] != m1) ++src;
			size_t jj = 0; uint64_t before = 0; while (before + G.GB[G.upd[jj]].depth <= src) before += G.GB[G.upd[jj++]].depth;
			G.O2.push_back(pga_detach_orphan_t{m1, G.who[first[G.upd[jj]] + (src - before)].node_id, new_id(), (uint32_t)(nu + G.O2.size()), rnd(4) ? rnd(50) : 0u, 0, 0});
		}
		G.B2.push_back(pga_rc_block_t{CONS + G.RCB[j].cons_off, G.RCB[j].cons_len, kept});
	}
	for (const auto &O : G.O2) G.B2.push_back(pga_rc_block_t{CONS + rnd(8), O.len, 1});
	return G;
}

static void append_lists(Out &D, const Lists &L, const std::string &letters, uint64_t s, uint64_t d, uint64_t i, const pga_rc_member_t &X)
{
	D.M.push_back(X);
	D.L.S.insert(D.L.S.end(), L.S.begin() + s, L.S.begin() + s + X.n_subs); D.L.D.insert(D.L.D.end(), L.D.begin() + d, L.D.begin() + d + X.n_dels);
	for (uint64_t k = i; k < i + X.n_inss; ++k) {
		D.L.I.push_back(pga_ins_t{L.I[k].pos, L.I[k].len, D.seq.size()});
		D.seq.append(letters, L.I[k].seq_off, L.I[k].len);
	}
}

// the scalar construction: every member's fate, then the blocks after in id order
static Out direct(const Case &G)
{
	Out D;
	const size_t nb = G.GB.size(), nu = G.upd.size(), n1 = G.O1.size();
	std::vector<uint64_t> first(nb + 1, 0), off[3];
	for (size_t b = 0; b < nb; ++b) first[b + 1] = first[b] + G.GB[b].depth;
	for (int q = 0; q < 3; ++q) off[q].assign(G.M.size() + 1, 0);
	for (size_t a = 0; a < G.M.size(); ++a) { off[0][a + 1] = off[0][a] + G.M[a].n_subs; off[1][a + 1] = off[1][a] + G.M[a].n_dels; off[2][a + 1] = off[2][a] + G.M[a].n_inss; }
	std::vector<uint64_t> off2[3];
	for (int q = 0; q < 3; ++q) off2[q].assign(G.M2.size() + 1, 0);
	for (size_t f = 0; f < G.M2.size(); ++f) { off2[0][f + 1] = off2[0][f] + G.M2[f].n_subs; off2[1][f + 1] = off2[1][f] + G.M2[f].n_dels; off2[2][f + 1] = off2[2][f] + G.M2[f].n_inss; }
	std::vector<int> upd_of(nb, -1);
	for (size_t j = 0; j < nu; ++j) upd_of[G.upd[j]] = (int)j;
	struct After { uint64_t id; int kind; uint32_t src; };
	std::vector<After> after;
	for (size_t b = 0; b < nb; ++b) if (G.GB[b].alive) after.push_back(After{G.GB[b].block_id, upd_of[b] < 0 ? CL_K_SURVIVOR : CL_K_UPDATED, upd_of[b] < 0 ? (uint32_t)b : (uint32_t)upd_of[b]});
	for (size_t k = 0; k < n1 + G.O2.size(); ++k) after.push_back(After{(k < n1 ? G.O1[k] : G.O2[k - n1]).block_id, CL_K_SINGLETON, (uint32_t)k});
	std::sort(after.begin(), after.end(), [](const After &x, const After &y) { return x.id < y.id; });
	// the merged member behind every place of the two stages
	std::vector<uint64_t> mfirst(nu + 1, 0), src1(G.map1.size()), src2(G.map2.size());
	for (size_t j = 0; j < nu; ++j) mfirst[j + 1] = mfirst[j] + G.GB[G.upd[j]].depth;
	for (size_t m = 0; m < G.map1.size(); ++m) src1[G.map1[m]] = m;
	const uint64_t k1 = G.map2.size(), k2 = G.M2.size();
	for (size_t m1 = 0; m1 < k1; ++m1) src2[G.map2[m1]] = src1[m1];
	auto global = [&](uint64_t m) { size_t j = 0; while (mfirst[j + 1] <= m) ++j; return first[G.upd[j]] + (m - mfirst[j]); };
	D.bmap.assign(nb, TP_NONE); D.orph.resize(n1 + G.O2.size());
	std::vector<ClWhere> where(G.M.size(), ClWhere{TP_NONE, TP_NONE});
	uint64_t f2 = 0;
	std::vector<uint64_t> r2first(nu + 1, 0);
	for (size_t j = 0; j < nu; ++j) r2first[j + 1] = r2first[j] + G.B2[j].n_members;
	for (uint32_t i = 0; i < after.size(); ++i) {
		const After &X = after[i];
		auto place = [&](uint64_t a, uint32_t slot, bool orphan) {
			D.origin.push_back((long long)a); D.who.push_back(pga_detach_member_t{G.who[a].node_id, orphan ? 0 : G.who[a].reverse, 0});
			where[a] = ClWhere{i | (orphan ? CL_ORPHAN : 0u), slot};
		};
		if (X.kind == CL_K_SURVIVOR) {
			const pga_topo_block_t &B = G.GB[X.src];
			D.GB.push_back(pga_topo_block_t{B.block_id, B.cons_len, B.depth, 1, 0}); D.rec.push_back(ClBlock{CL_K_SURVIVOR, X.src, B.depth, 0});
			D.bmap[X.src] = i;
			for (uint32_t s = 0; s < B.depth; ++s) { const uint64_t a = first[X.src] + s; place(a, s, false); append_lists(D, G.B, G.seq, off[0][a], off[1][a], off[2][a], G.M[a]); }
		} else if (X.kind == CL_K_UPDATED) {
			const uint32_t j = X.src, depth = G.B2[j].n_members;
			D.GB.push_back(pga_topo_block_t{G.GB[G.upd[j]].block_id, G.RCB[j].cons_len, depth, 1, 0}); D.rec.push_back(ClBlock{CL_K_UPDATED, j, depth, 0});
			D.bmap[G.upd[j]] = i;
			for (uint32_t s = 0; s < depth; ++s) { const uint64_t f = r2first[j] + s; place(global(src2[f]), s, false); append_lists(D, G.L2, G.rc_seq, off2[0][f], off2[1][f], off2[2][f], G.M2[f]); }
		} else {
			const uint32_t k = X.src;
			pga_detach_orphan_t O = k < n1 ? G.O1[k] : G.O2[k - n1];
			const uint64_t a = global(k < n1 ? O.member : src1[O.member]);
			D.GB.push_back(pga_topo_block_t{O.block_id, O.len, 1, 1, 0}); D.rec.push_back(ClBlock{CL_K_SINGLETON, k, 1, 0});
			place(a, 0, true); append_lists(D, G.B, G.seq, 0, 0, 0, pga_rc_member_t{0, 0, 0});
			O.member = a; O.block = i; D.orph[k] = O;
		}
	}
	(void)f2; (void)k2;
	for (const pga_topo_node_t &N : G.GN) {
		const ClWhere W = where[first[N.block] + N.member];
		pga_topo_node_t A = N;
		A.block = W.block & ~CL_ORPHAN; A.member = W.slot; if (W.block & CL_ORPHAN) A.reverse = 0;
		D.GN.push_back(A);
	}
	return D;
}

// ---------------------------------------------------------------- the kernels in the order of pga_close.hip
struct ScanBufs {
	Exact<cl_u64> tile_sum, tile_off, off; RmScan S;
	ScanBufs(uint64_t n, uint32_t n_q) : tile_sum((size_t)n_q * ((n + CL_TILE - 1) / CL_TILE)), tile_off((size_t)n_q * ((n + CL_TILE - 1) / CL_TILE + 1)), off((size_t)n_q * (n + 1)),
		S{n, (uint32_t)((n + CL_TILE - 1) / CL_TILE), n_q, tile_sum.get(), tile_off.get(), off.get()} {}
};
template <class Val> static void scan(const RmScan &S, const Val &val, unsigned grid)
{
	if (S.n_tiles) emu_launch(dim3(std::min<unsigned>(grid, S.n_tiles)), dim3(CL_THREADS), [&] { k_ts_sums<cl_u64, Val>(S, val); });
	emu_launch(dim3(1), dim3(CL_THREADS), [&] { k_ts_scan<cl_u64>(S); });
	if (S.n_tiles) emu_launch(dim3(std::min<unsigned>(grid, S.n_tiles)), dim3(CL_THREADS), [&] { k_ts_offsets<cl_u64, Val>(S, val); });
}
static void validate(const Case &G, uint32_t flags, ClTables &C)
{
	const pga_detach_out_t d1 = G.d1(), d2 = G.d2();
	const pga_rc_out_t rc = G.rc();
	cl_validate((int64_t)G.GB.size(), G.GB.data(), (int64_t)G.GP.size(), G.GP.data(), (int64_t)G.GN.size(), G.GN.data(), G.RB.data(), G.M.data(), G.B.S.data(), G.B.D.data(), G.B.I.data(),
	            G.who.data(), (int64_t)G.upd.size(), G.upd.data(), &d1, &rc, &d2, flags, C);
}

struct Errs { uint32_t topo[TP_ERRS]; cl_u64 cl[CL_ERRS]; as_u64 as[AS_ERRS]; };
// returns false on a CHECK; `refused` says whether the device checks stopped the call (nothing behind them has run then)
static bool emulated(const Case &G, unsigned grid, uint64_t seq_len, uint64_t rc_seq_len, Out &O, Errs &E, bool &refused)
{
	ClTables C;
	validate(G, 0, C);
	const uint64_t nb = G.GB.size(), np = G.GP.size(), nn = G.GN.size(), nu = G.upd.size(), nm = C.n_before, nm1 = C.n_merged, k1 = C.n_k1, k2 = C.n_k2;
	const uint64_t no = C.n_o1 + C.n_o2, na = C.alive_id.size(), nbo = C.n_out_blocks, nmo = C.n_out_members;
	refused = false;
	CHECK(nm == G.M.size() && nm1 == G.map1.size() && k1 == G.map2.size() && k2 == G.M2.size() && C.before_tot[0] == G.B.S.size() && C.second_tot[2] == G.L2.I.size());
	Exact<pga_topo_node_t> nodes(G.GN), onodes(nn); Exact<pga_topo_path_t> paths(G.GP); Exact<pga_topo_block_t> blocks(G.GB), oblocks(nbo);
	Exact<uint32_t> depth(C.T.depth), first(C.T.slot_first), upd(G.upd), rclen(C.rc_len), ablock(C.alive_block), aupd(C.alive_upd), bmap(nb), sorph(no), pathof(nn), cnts(nm + nb), terr((size_t)TP_ERRS);
	Exact<int32_t> kinds(C.kinds); Exact<tp_u64> key(nn);
	Exact<cl_u64> mfirst(C.mfirst), r1first(C.r1first), r2first(C.r2first), aid(C.alive_id), sid(no), fin(k2), osrc(no), err((size_t)CL_ERRS), aerr((size_t)AS_ERRS);
	Exact<long long> map1(G.map1), map2(G.map2), origin(nmo);
	Exact<pga_rc_member_t> members(G.M), members2(G.M2), omembers(nmo);
	Exact<pga_sub_t> subs(G.B.S), subs2(G.L2.S); Exact<pga_del_t> dels(G.B.D), dels2(G.L2.D); Exact<pga_ins_t> inss(G.B.I), inss2(G.L2.I);
	Exact<char> letters(seq_len + rc_seq_len);
	Exact<pga_detach_orphan_t> orph(C.orphans), oorph(no); Exact<pga_detach_member_t> who(G.who), owho(nmo);
	Exact<ClBlock> rec(nbo); Exact<ClWhere> where(nm); Exact<AsDesc> desc(nmo);
	std::copy(G.seq.begin(), G.seq.begin() + seq_len, letters.get()); std::copy(G.rc_seq.begin(), G.rc_seq.begin() + rc_seq_len, letters.get() + seq_len);
	terr.fill(0xff); err.fill(0xff); aerr.fill(0xff); fin.fill(0xff); osrc.fill(0xff); rec.fill(0xff); where.fill(0xff); bmap.fill(0xff);
	{   // the singleton ids, sorted with their orphan numbers
		std::vector<std::pair<cl_u64, uint32_t>> s;
		for (uint64_t k = 0; k < no; ++k) s.push_back({C.orphans[k].block_id, (uint32_t)k});
		std::stable_sort(s.begin(), s.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
		for (uint64_t k = 0; k < no; ++k) { sid[k] = s[k].first; sorph[k] = s[k].second; }
	}
	TpDev T;
	memset(&T, 0, sizeof(T));
	T.n_nodes = nn; T.n_paths = np; T.n_blocks = nb; T.n_slots = nm;
	T.nodes = nodes.get(); T.paths = paths.get(); T.depth = depth.get(); T.slot_first = first.get(); T.path_of = pathof.get(); T.key = key.get();
	T.slot_cnt = cnts.get(); T.blk_cnt = cnts.get() + nm; T.err = terr.get();
	ScanBufs b_before(nm, 3), b_second(k2, 3), b_kept1(nm1, 1), b_kept2(k1, 1), b_blocks(nbo, 1), b_out(nmo, 3);
	ClDev V;
	memset(&V, 0, sizeof(V));
	V.n_upd = nu; V.n_merged = nm1; V.n_k1 = k1; V.n_k2 = k2; V.n_o1 = C.n_o1; V.n_orphans = no; V.n_alive = na; V.n_blocks = nb; V.n_out_blocks = nbo; V.n_nodes = nn;
	V.blocks = blocks.get(); V.nodes = nodes.get(); V.first_member = first.get(); V.upd = upd.get(); V.mfirst = mfirst.get(); V.r1first = r1first.get(); V.r2first = r2first.get();
	V.rc_len = rclen.get(); V.kinds = kinds.get(); V.map1 = map1.get(); V.map2 = map2.get(); V.members2 = members2.get(); V.orphans = orph.get(); V.who = who.get();
	V.alive_id = aid.get(); V.alive_block = ablock.get(); V.alive_upd = aupd.get(); V.sing_id = sid.get(); V.sing_orphan = sorph.get(); V.fin_src = fin.get(); V.orph_src = osrc.get();
	V.o_rec = rec.get(); V.o_blocks = oblocks.get(); V.block_map = bmap.get(); V.where = where.get(); V.o_who = owho.get(); V.o_orphans = oorph.get(); V.o_nodes = onodes.get(); V.err = err.get();
	V.A.n_out_members = nmo; V.A.ins_seq_len = seq_len; V.A.p_ins_seq_len = rc_seq_len;
	V.A.members = members.get(); V.A.subs = subs.get(); V.A.dels = dels.get(); V.A.inss = inss.get();
	V.A.p_subs = subs2.get(); V.A.p_dels = dels2.get(); V.A.p_inss = inss2.get(); V.A.letters = letters.get();
	V.A.desc = desc.get(); V.A.o_members = omembers.get(); V.A.origin = origin.get(); V.A.err = aerr.get();
	V.scan[CL_SCAN_BEFORE] = b_before.S; V.scan[CL_SCAN_SECOND] = b_second.S; V.scan[CL_SCAN_KEPT1] = b_kept1.S; V.scan[CL_SCAN_KEPT2] = b_kept2.S;
	V.scan[CL_SCAN_BLOCKS] = b_blocks.S; V.A.scan[AS_SCAN_OUT] = b_out.S;
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_keys(T); });
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_check(T); });
	scan(V.scan[CL_SCAN_BEFORE], AsBeforeValue{V.A}, grid);
	scan(V.scan[CL_SCAN_SECOND], ClSecondValue{V}, grid);
	scan(V.scan[CL_SCAN_KEPT1], ClKeptValue{V.map1, k1}, grid);
	scan(V.scan[CL_SCAN_KEPT2], ClKeptValue{V.map2, k2}, grid);
	emu_launch(dim3(grid), dim3(CL_THREADS), [&] { k_close_stage<1>(V); });
	emu_launch(dim3(grid), dim3(CL_THREADS), [&] { k_close_stage<2>(V); });
	emu_launch(dim3(grid), dim3(CL_THREADS), [&] { k_close_chain(V); });
	emu_launch(dim3(grid), dim3(CL_THREADS), [&] { k_close_rank(V); });
	scan(V.scan[CL_SCAN_BLOCKS], ClDepthValue{V}, grid);
	emu_launch(dim3(grid), dim3(CL_THREADS), [&] { k_close_desc(V); });
	emu_launch(dim3(grid), dim3(CL_THREADS), [&] { k_close_nodes(V); });
	scan(V.A.scan[AS_SCAN_OUT], AsOutValue{V.A}, grid);
	auto read_errs = [&]() {
		std::copy(terr.get(), terr.get() + TP_ERRS, E.topo); std::copy(err.get(), err.get() + CL_ERRS, E.cl); std::copy(aerr.get(), aerr.get() + AS_ERRS, E.as);
		for (uint32_t x : E.topo) if (x != TP_NONE) return true;
		for (cl_u64 x : E.cl) if (x != CL_NONE) return true;
		for (as_u64 x : E.as) if (x != AS_NONE) return true;
		return false;
	};
	if (read_errs()) { refused = true; return true; }
	CHECK(b_blocks.off[nbo] == nmo);
	const uint64_t ns_out = b_out.off[0 * (nmo + 1) + nmo], nd_out = b_out.off[1 * (nmo + 1) + nmo], ni_out = b_out.off[2 * (nmo + 1) + nmo];
	Exact<pga_sub_t> osubs(ns_out); Exact<pga_del_t> odels(nd_out); Exact<pga_ins_t> oinss(ni_out);
	V.A.o_subs = osubs.get(); V.A.o_dels = odels.get(); V.A.o_inss = oinss.get();
	if (ns_out) emu_launch(dim3(grid), dim3(AS_THREADS), [&] { k_assemble_copy<RM_LIST_SUB>(V.A); });
	if (nd_out) emu_launch(dim3(grid), dim3(AS_THREADS), [&] { k_assemble_copy<RM_LIST_DEL>(V.A); });
	if (ni_out) emu_launch(dim3(grid), dim3(AS_THREADS), [&] { k_assemble_copy<RM_LIST_INS>(V.A); });
	ScanBufs b_let(ni_out, 1);
	V.A.scan[AS_SCAN_LETTERS] = b_let.S;
	scan(V.A.scan[AS_SCAN_LETTERS], AsLetterValue{V.A}, grid);
	if (read_errs()) { refused = true; return true; }
	const uint64_t nl_out = b_let.off[ni_out];
	Exact<char> oseq(nl_out);
	V.A.o_ins_seq = oseq.get();
	if (nl_out) emu_launch(dim3(grid), dim3(AS_THREADS), [&] { k_assemble_letters(V.A); });
	if (ni_out) emu_launch(dim3(grid), dim3(AS_THREADS), [&] { k_assemble_seq_off(V.A); });
	O.GB.assign(oblocks.get(), oblocks.get() + nbo); O.GN.assign(onodes.get(), onodes.get() + nn); O.rec.assign(rec.get(), rec.get() + nbo);
	O.M.assign(omembers.get(), omembers.get() + nmo); O.L.S.assign(osubs.get(), osubs.get() + ns_out); O.L.D.assign(odels.get(), odels.get() + nd_out);
	O.L.I.assign(oinss.get(), oinss.get() + ni_out); O.who.assign(owho.get(), owho.get() + nmo); O.origin.assign(origin.get(), origin.get() + nmo);
	O.bmap.assign(bmap.get(), bmap.get() + nb); O.orph.assign(oorph.get(), oorph.get() + no);
	if (nl_out) O.seq.assign(oseq.get(), nl_out);
	return true;
}

template <class T> static bool same(const std::vector<T> &a, const std::vector<T> &b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }

static bool run_case(const Case &G, unsigned grid)
{
	Out E, D = direct(G);
	Errs err; bool refused;
	if (!emulated(G, grid, G.seq.size(), G.rc_seq.size(), E, err, refused)) return false;
	CHECK(!refused);
	CHECK(same(E.GB, D.GB)); CHECK(same(E.rec, D.rec)); CHECK(same(E.GN, D.GN)); CHECK(same(E.M, D.M)); CHECK(same(E.L.S, D.L.S)); CHECK(same(E.L.D, D.L.D)); CHECK(same(E.L.I, D.L.I));
	CHECK(E.seq == D.seq); CHECK(same(E.who, D.who)); CHECK(same(E.origin, D.origin)); CHECK(same(E.bmap, D.bmap)); CHECK(same(E.orph, D.orph));
	for (size_t i = 1; i < E.GB.size(); ++i) CHECK(E.GB[i - 1].block_id < E.GB[i].block_id);
	return true;
}

// ---------------------------------------------------------------- a named case of tests/close_gen.py from its file (close_gen.dump)
struct Reader {
	std::string buf; size_t at = 0; bool ok = true;
	template <class T> std::vector<T> take()
	{
		std::vector<T> v;
		if (at + 8 > buf.size()) { ok = false; return v; }
		uint64_t n; memcpy(&n, buf.data() + at, 8); at += 8;
		if (n % sizeof(T) || at + n > buf.size()) { ok = false; return v; }
		v.resize(n / sizeof(T));
		if (n) memcpy(v.data(), buf.data() + at, n);
		at += n;
		return v;
	}
	std::string text() { const std::vector<char> v = take<char>(); return std::string(v.begin(), v.end()); }
	std::vector<pga_rc_block_t> blocks() { std::vector<pga_rc_block_t> B; const std::vector<uint32_t> v = take<uint32_t>(); for (size_t i = 0; i + 1 < v.size(); i += 2) B.push_back(pga_rc_block_t{CONS, v[i], v[i + 1]}); return B; }
};
static bool load(const char *file, Case &G, Out &X)
{
	Reader R;
	FILE *f = fopen(file, "rb");
	if (!f) return false;
	char tmp[1 << 16]; size_t n;
	while ((n = fread(tmp, 1, sizeof(tmp), f)) > 0) R.buf.append(tmp, n);
	fclose(f);
	G.GB = R.take<pga_topo_block_t>(); G.GP = R.take<pga_topo_path_t>(); G.GN = R.take<pga_topo_node_t>(); G.RB = R.blocks(); G.M = R.take<pga_rc_member_t>();
	G.B.S = R.take<pga_sub_t>(); G.B.D = R.take<pga_del_t>(); G.B.I = R.take<pga_ins_t>(); G.seq = R.text(); G.who = R.take<pga_detach_member_t>(); G.upd = R.take<uint32_t>();
	G.B1 = R.blocks(); G.map1 = R.take<int64_t>(); G.O1 = R.take<pga_detach_orphan_t>(); G.B2 = R.blocks(); G.map2 = R.take<int64_t>(); G.O2 = R.take<pga_detach_orphan_t>();
	G.RCB = R.take<pga_rc_block_res_t>(); G.RCM = R.take<pga_mapvar_res_t>(); G.rc_seq = R.text(); G.M2 = R.take<pga_rc_member_t>();
	G.L2.S = R.take<pga_sub_t>(); G.L2.D = R.take<pga_del_t>(); G.L2.I = R.take<pga_ins_t>();
	for (auto &B : G.RCB) B.cons_off = 0;                                    // (no consensus letter is read here: every pointer leads to CONS)
	X.GB = R.take<pga_topo_block_t>(); X.GN = R.take<pga_topo_node_t>(); X.M = R.take<pga_rc_member_t>(); X.L.S = R.take<pga_sub_t>(); X.L.D = R.take<pga_del_t>(); X.L.I = R.take<pga_ins_t>();
	X.seq = R.text(); X.origin = R.take<long long>(); X.bmap = R.take<uint32_t>();
	return R.ok && R.at == R.buf.size();
}
// the kernels on a named case, against the scalar construction AND against what the Python side expects (host_close, flattened)
static bool run_file(const char *file)
{
	Case G; Out X;
	if (!load(file, G, X)) { fprintf(stderr, "close_emu: cannot read %s\n", file); return false; }
	Out E, D = direct(G);
	Errs err; bool refused;
	if (!emulated(G, 2, G.seq.size(), G.rc_seq.size(), E, err, refused)) return false;
	CHECK(!refused);
	CHECK(same(E.GB, D.GB)); CHECK(same(E.rec, D.rec)); CHECK(same(E.GN, D.GN)); CHECK(same(E.M, D.M)); CHECK(same(E.L.S, D.L.S)); CHECK(same(E.L.D, D.L.D)); CHECK(same(E.L.I, D.L.I));
	CHECK(E.seq == D.seq); CHECK(same(E.who, D.who)); CHECK(same(E.origin, D.origin)); CHECK(same(E.bmap, D.bmap)); CHECK(same(E.orph, D.orph));
	CHECK(same(E.GB, X.GB)); CHECK(same(E.GN, X.GN)); CHECK(same(E.M, X.M)); CHECK(same(E.L.S, X.L.S)); CHECK(same(E.L.D, X.L.D)); CHECK(same(E.L.I, X.L.I));
	CHECK(E.seq == X.seq); CHECK(same(E.origin, X.origin)); CHECK(same(E.bmap, X.bmap));
	return true;
}

template <class F> static bool refused_by_host(F f) { try { f(); } catch (std::runtime_error &) { return true; } return false; }

int main(int argc, char **argv)
{
	// ---- the named cases of tests/close_gen.py, one file each
	for (int a = 1; a < argc; ++a) { g_case = 1000 + a; if (!run_file(argv[a])) { fprintf(stderr, "close_emu: %s\n", argv[a]); return 1; } }
	size_t n_big = 0, n_o1 = 0, n_o2 = 0, n_long = 0, n_empty = 0, n_dead = 0;
	for (g_case = 0; g_case < 9; ++g_case) {
		const int kind = g_case;                          // 3: more than one tile of members; 4: lists of several tiles; 5: everything updated; 6: nobody leaves; 7: nothing updated
		const Case G = kind == 3 ? generate(700, 4, 3, 4, 0) : kind == 4 ? generate(8, 4, 2, 4, 2 * CL_TILE + 5) : kind == 5 ? generate(30, 3, 1, 2, 0) : kind == 6 ? generate(20, 4, 2, 0, 0)
		               : kind == 7 ? generate(20, 4, 1u << 30, 4, 0) : generate(6 + rnd(12), 5, 2, 3, 0);
		if (!run_case(G, 1 + rnd(3))) return 1;
		const Out D = direct(G);
		n_big += D.M.size() > (size_t)CL_TILE; n_long += D.L.S.size() > (size_t)2 * CL_TILE; n_o1 += G.O1.size(); n_o2 += G.O2.size();
		for (size_t j = 0; j < G.upd.size(); ++j) n_empty += G.B2[j].n_members == 0 && G.GB[G.upd[j]].depth != 0;
		for (const auto &B : G.GB) n_dead += !B.alive;
	}
	if (n_big < 1 || n_o1 < 20 || n_o2 < 5 || n_long < 1 || n_empty < 1 || n_dead < 3) {
		fprintf(stderr, "close_emu: the generator lost its cases (%zu big, %zu + %zu orphans, %zu long lists, %zu emptied blocks, %zu dead entries)\n", n_big, n_o1, n_o2, n_long, n_empty, n_dead);
		return 1;
	}
	// ---- one updated block of 1023 / 1024 / 1025 members, and one that straddles a tile edge behind 1000 survivors' members
	for (uint32_t target : {(uint32_t)CL_TILE - 1, (uint32_t)CL_TILE, (uint32_t)CL_TILE + 1, 100u}) {
		g_case = 100 + (int)target;
		const Case G = generate(4, 3, 2, 5, 0, target, target == 100 ? 1000 : 2);
		if (!run_case(G, target == (uint32_t)CL_TILE ? 2 : 1)) return 1;
	}
	// ---- what is refused: on the host, and by the kernels before an index is derived
	g_case = -2;
	Case H;
	auto fits = [](const Case &Y) {
		if (Y.upd.size() < 2 || Y.O1.size() < 2 || Y.O2.size() < 1 || Y.L2.I.empty() || Y.B.I.empty()) return false;
		bool letters2 = false, letters = false, two_kept = false;
		for (const auto &I : Y.L2.I) letters2 = letters2 || I.len;
		uint64_t a = 0, at = 0;                                // a survivor's insertion with letters behind the first three of the buffer
		for (size_t b = 0; b < Y.GB.size(); ++b) for (uint32_t s = 0; s < Y.GB[b].depth; ++s, ++a) {
			const bool updated = std::find(Y.upd.begin(), Y.upd.end(), (uint32_t)b) != Y.upd.end();
			for (uint32_t k = 0; k < Y.M[a].n_inss; ++k, ++at) letters = letters || (!updated && Y.B.I[at].len && Y.B.I[at].seq_off + Y.B.I[at].len > 3);
		}
		for (size_t m = 0; m + 1 < Y.map1.size(); ++m) two_kept = two_kept || (Y.map1[m] + 1 == Y.map1[m + 1]);
		return letters && letters2 && two_kept && Y.B1[0].n_members && Y.B1[1].n_members;
	};
	do H = generate(14, 5, 2, 3, 0); while (!fits(H));
	auto host = [&](const Case &X, uint32_t flags) { ClTables C; validate(X, flags, C); };
	host(H, 0); host(H, 1);
	bool ok = true;
	Case X = H;                                                        ok = ok && refused_by_host([&] { host(X, 2); });
	X = H; X.upd[0] = (uint32_t)X.GB.size();                           ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.upd[1] = X.upd[0];                                        ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.GB[X.upd[0]].alive = 0;                                   ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.RB[X.upd[0]].n_members += 1;                              ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.B1.pop_back();                                            ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.B2.push_back(X.B2.back());                                ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.RCB[0].kind = -3;                                         ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.RCM[0].status = 7;                                        ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.O1[0].status = 2;                                         ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.O2[0].status = 3;                                         ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.B1[0].n_members += 1;                                     ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.GP[0].node_off += 1;                                      ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; { size_t b = 0; while (!X.GB[b].alive) ++b; X.RB[b].cons_len += 1; }   ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.O1[0].block += 1;                                         ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.B2[X.upd.size()].cons_len += 1;                           ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.RCB[0].kind = 0; X.RCB[0].cons_len = X.RB[X.upd[0]].cons_len + 1;    ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.GN[0].member = X.GB[X.GN[0].block].depth;                 ok = ok && refused_by_host([&] { host(X, 0); });
	if (!ok) { fprintf(stderr, "close_emu: malformed input was accepted by the host\n"); return 1; }
	auto device = [&](const Case &Y, uint64_t seq_len, uint64_t rc_seq_len, int set, int which) {
		Out E; Errs err; bool refused;
		if (!emulated(Y, 1, seq_len, rc_seq_len, E, err, refused)) return false;
		const bool hit = set == 0 ? err.topo[which] != TP_NONE : set == 1 ? err.cl[which] != CL_NONE : err.as[which] != AS_NONE;
		return refused && hit && E.M.empty() && E.L.S.empty();
	};
	const size_t ns = H.seq.size(), nr = H.rc_seq.size();
	{ X = H; X.B1[0].n_members += 1; X.B1[1].n_members -= 1; ok = ok && device(X, ns, nr, 1, CL_E_DEPTH1); }
	{ X = H; size_t m = 0; while (X.map1[m] + 1 != X.map1[m + 1]) ++m; std::swap(X.map1[m], X.map1[m + 1]); ok = ok && device(X, ns, nr, 1, CL_E_MAP1); }
	{ X = H; X.map1[0] = -1; ok = ok && device(X, ns, nr, 1, CL_E_MAP1); }
	{ X = H; X.map1[0] = (int64_t)X.map1.size(); ok = ok && device(X, ns, nr, 1, CL_E_MAP1); }
	{ X = H; X.map1[0] = X.map1[1]; ok = ok && device(X, ns, nr, 1, CL_E_MAP1); }
	{ X = H; X.O1[0].member = X.O1[1].member; ok = ok && device(X, ns, nr, 1, CL_E_MAP1); }
	{ X = H; X.map2[0] = -5; ok = ok && device(X, ns, nr, 1, CL_E_MAP2); }
	{ X = H; X.map2[X.O2[0].member] = X.map2[X.O2[0].member ? 0 : 1]; ok = ok && device(X, ns, nr, 1, CL_E_MAP2); }
	{ X = H; size_t j = 0; uint64_t at = 0; while (at + X.B1[j].n_members <= X.O2[0].member) at += X.B1[j++].n_members; X.RCB[j].kind = 1; ok = ok && device(X, ns, nr, 1, CL_E_KIND); }
	{ X = H; size_t b = 0; while (!X.GB[b].alive) ++b; X.O1[0].block_id = X.GB[b].block_id; ok = ok && device(X, ns, nr, 1, CL_E_ID); }
	{ X = H; X.O1[1].block_id = X.O2[0].block_id; ok = ok && device(X, ns, nr, 1, CL_E_ID); }
	{ X = H; X.GN[1].block = X.GN[0].block; X.GN[1].member = X.GN[0].member; ok = ok && device(X, ns, nr, 0, TP_E_SLOT); }
	ok = ok && device(H, ns, 0, 2, AS_E_SEQ_RANGE);
	ok = ok && device(H, 3, nr, 2, AS_E_SEQ_RANGE);
	{ X = H; for (auto &I : X.L2.I) I.seq_off = ~0ULL - 2; ok = ok && device(X, ns, nr, 2, AS_E_SEQ_RANGE); }                             // (seq_off + len wraps)
	if (!ok) { fprintf(stderr, "close_emu: malformed input passed the kernels' checks\n"); return 1; }
	// ---- pga_rc_detach_args
	{
		const pga_detach_out_t d1 = H.d1(); const pga_rc_out_t rc = H.rc();
		const size_t nu = H.upd.size(), k1 = H.map2.size();
		std::vector<pga_detach_member_t> wm;
		size_t n_first = 0;
		for (size_t j = 0; j < nu; ++j) { uint64_t f = 0; for (uint32_t b = 0; b < H.upd[j]; ++b) f += H.GB[b].depth; for (uint32_t s = 0; s < H.GB[H.upd[j]].depth; ++s) wm.push_back(H.who[f + s]); n_first += H.GB[H.upd[j]].depth; }
		Case Y = H;
		for (size_t m1 = 0; m1 < k1; ++m1) { Y.RCM[m1].n_subs = (uint32_t)m1; Y.RCM[m1].n_dels = 2; Y.RCM[m1].n_inss = 7; }
		const pga_rc_out_t rc2 = Y.rc();
		Exact<pga_rc_block_t> B(nu); Exact<pga_rc_member_t> M(k1); Exact<pga_detach_member_t> W(k1);
		cl_detach_args((int64_t)nu, &d1, wm.data(), &rc2, B.get(), M.get(), W.get());
		for (size_t j = 0; j < nu; ++j) ok = ok && B[j].consensus == rc.cons + H.RCB[j].cons_off && B[j].cons_len == H.RCB[j].cons_len && B[j].n_members == H.B1[j].n_members;
		for (size_t m1 = 0; m1 < k1; ++m1) ok = ok && M[m1].n_subs == m1 && M[m1].n_dels == 2 && M[m1].n_inss == 7;
		for (size_t m = 0; m < n_first; ++m) if ((uint64_t)H.map1[m] < k1) ok = ok && W[H.map1[m]].node_id == wm[m].node_id && W[H.map1[m]].reverse == wm[m].reverse;
		if (!ok) { fprintf(stderr, "close_emu: pga_rc_detach_args is off\n"); return 1; }
	}
	printf("close_emu OK (%d named cases, %zu graphs of more than one tile, %zu + %zu orphans, %zu with long lists, %zu emptied blocks, %zu dead entries)\n", argc - 1, n_big, n_o1, n_o2, n_long, n_empty, n_dead);
	return 0;
}
