// pga_apply_idx.h without a device: validation and the tables, then every kernel of the header (and the splice of pga_topo_idx.h behind them)
// under dev/emu/hip_emu.h -- the radix sorts and the scans of pga_apply.hip replaced by std::stable_sort and plain loops -- with every buffer
// allocated at exactly the size the kernels may touch (under the address sanitizer an access one entry out is an error), against a direct
// scalar construction of the graph update of a merge (reweave.rs:359-401 and 445-450 over pangraph.rs:68-107, graph_merging.rs:156-165):
// maps keyed by id, a path rebuilt node after node.
// Build and run (host only):  g++ -std=c++17 -g -O1 -DPGA_EMU -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined
//                             tests/emu/apply_emu.cpp -o apply_emu && ./apply_emu
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <numeric>
#include <random>
#include <set>
#include <string>
#include "../../dev/emu/hip_emu.h"
#include "../../pangraph_amd/csrc/pga_apply_idx.h"
#include "../../pangraph_amd/csrc/pga_detach_idx.h"

using namespace pga;

template <class T> struct Exact {                                       // n entries, not one more
	std::unique_ptr<T[]> p; size_t n;
	explicit Exact(size_t n_) : p(n_ ? new T[n_]() : nullptr), n(n_) {}
	T *get() { return p.get(); }
	T &operator[](size_t i) { return p[i]; }
};

static std::mt19937 rng(20261019);
static uint32_t rnd(uint32_t n) { return n ? (uint32_t)(rng() % n) : 0u; }
static uint64_t rnd64() { return ((uint64_t)rng() << 32) | rng(); }
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "apply_emu: %s:%d: %s (case %d)\n", __FILE__, __LINE__, #c, g_case); return false; } } while (0)
static int g_case = -1;

struct Case {
	std::vector<pga_topo_block_t> B; std::vector<pga_topo_path_t> P; std::vector<pga_topo_node_t> N;
	std::vector<pga_apply_cut_t> cut; std::vector<pga_plan_interval_t> iv; std::vector<pga_slice_res_t> S; std::vector<pga_slice_member_t> M;
};
struct Out {
	std::vector<pga_topo_node_t> fresh, N; std::vector<uint64_t> old, src; std::vector<pga_apply_block_t> made; std::vector<uint32_t> map;
	std::vector<pga_topo_path_t> P; std::vector<pga_topo_block_t> B;
};

// ---------------------------------------------------------------- cases: random blocks on random paths, some of them cut
static Case generate(uint32_t n_blocks, uint32_t max_depth, uint32_t n_paths, uint32_t max_intervals, uint32_t filler)
{
	Case G;
	std::set<uint64_t> ids;
	while (ids.size() < n_blocks) ids.insert(rnd(4) ? 1 + rnd(100000) : rnd64() | (1ULL << 63));
	for (uint64_t id : ids) {
		if (rnd(6) == 0) G.B.push_back(pga_topo_block_t{0, 7, 3, 0, 0});                // a dead entry
		G.B.push_back(pga_topo_block_t{id, 40 + rnd(60), 0, 1, 0});
	}
	{ uint64_t last = 0; for (auto &b : G.B) if (b.alive) last = b.block_id; else b.block_id = last; }
	std::vector<std::vector<uint32_t>> walk(n_paths);
	std::vector<uint32_t> alive;
	for (uint32_t b = 0; b < G.B.size(); ++b) if (G.B[b].alive) alive.push_back(b);
	for (uint32_t b : alive) for (uint32_t d = rnd(max_depth + 1); d; --d) walk[rnd(n_paths)].push_back(b);
	for (uint32_t f = 0; f < filler; ++f) walk[0].push_back(alive[0]);
	uint64_t nid = 1000;
	for (uint32_t p = 0; p < n_paths; ++p) {
		std::shuffle(walk[p].begin(), walk[p].end(), rng);
		pga_topo_path_t P{10 + 3 * (uint64_t)p, G.N.size(), (uint32_t)walk[p].size(), (int32_t)rnd(2)};
		uint64_t at = 1000 * (uint64_t)p;
		for (uint32_t b : walk[p]) { G.N.push_back(pga_topo_node_t{++nid, at, at + G.B[b].cons_len, b, G.B[b].depth++, (int32_t)rnd(2), 0}); at += G.B[b].cons_len + 1; }
		G.P.push_back(P);
	}
	std::vector<std::vector<uint32_t>> perm(G.B.size());
	for (size_t b = 0; b < G.B.size(); ++b) { perm[b].resize(G.B[b].alive ? G.B[b].depth : 0); std::iota(perm[b].begin(), perm[b].end(), 0u); std::shuffle(perm[b].begin(), perm[b].end(), rng); }
	for (auto &n : G.N) n.member = perm[n.block][n.member];
	// the cut: every third alive block or so, but never the filler's; an aligned interval waits for the next one to be its partner
	std::set<uint64_t> used(ids);
	auto fresh_id = [&] { uint64_t id; do id = rnd(3) ? 1 + rnd(200000) : rnd64(); while (!used.insert(id).second); return id; };
	int64_t waiting = -1;
	for (uint32_t b : alive) {
		if (b == alive[0] || rnd(3)) continue;
		const uint32_t n_int = 1 + rnd(max_intervals), len = G.B[b].cons_len / n_int;
		G.cut.push_back(pga_apply_cut_t{b, n_int, G.iv.size()});
		for (uint32_t j = 0; j < n_int; ++j) {
			pga_plan_interval_t I{};
			I.start = j * len + (j && len > 1 ? rnd(2) : 0); I.end = (j + 1) * len; I.match = -1;   // (a gap between two intervals is legal)
			if (rnd(3) == 0) {
				I.aligned = 1;
				if (waiting < 0) { I.new_block_id = fresh_id(); I.is_anchor = (int32_t)rnd(2); waiting = (int64_t)G.iv.size(); }
				else { I.new_block_id = G.iv[waiting].new_block_id; I.is_anchor = !G.iv[waiting].is_anchor; waiting = -1; }
			} else I.new_block_id = fresh_id();
			G.iv.push_back(I);
			pga_slice_res_t R{G.M.size(), 0, 0};
			for (uint32_t m = 0; m < G.B[b].depth; ++m) {
				if (rnd(5) == 0) { ++R.n_dropped; continue; }
				pga_slice_member_t X{};
				X.member = m; X.reverse = (int32_t)rnd(2); X.pos_start = rnd64() >> 20; X.pos_end = X.pos_start + rnd(1000);
				G.M.push_back(X); ++R.n_kept;
			}
			G.S.push_back(R);
		}
	}
	if (waiting >= 0) { G.iv[waiting].aligned = 0; G.iv[waiting].is_anchor = 0; }
	return G;
}

// ---------------------------------------------------------------- the direct construction
static uint64_t hash_words(std::initializer_list<uint64_t> w)
{
	std::vector<uint8_t> b;
	for (uint64_t x : w) for (int i = 0; i < 8; ++i) b.push_back((uint8_t)(x >> (8 * i)));
	return xxh64_bytes(b.data(), b.size(), 0);
}
static Out direct(const Case &G)
{
	Out D;
	std::map<std::pair<uint32_t, uint32_t>, size_t> where;               // (block, member) -> position
	std::vector<uint64_t> path_id(G.N.size());
	for (const auto &P : G.P) for (uint64_t i = P.node_off; i < P.node_off + P.n_nodes; ++i) { where[{G.N[i].block, G.N[i].member}] = i; path_id[i] = P.path_id; }
	std::map<uint32_t, size_t> cut_of;
	for (size_t c = 0; c < G.cut.size(); ++c) cut_of[G.cut[c].block] = c;
	struct Made { int32_t kind = 0; uint64_t ia = 0, ib = 0; uint32_t len = 0; std::vector<std::pair<uint64_t, uint64_t>> members; };   // (node id, k)
	std::map<uint64_t, Made> made;
	std::vector<uint64_t> block_of_member(G.M.size());
	D.fresh.resize(G.M.size()); D.old.resize(G.M.size());
	for (const auto &C : G.cut) for (uint32_t j = 0; j < C.n_intervals; ++j) {
		const uint64_t s = C.first_interval + j;
		const auto &I = G.iv[s];
		Made &X = made[I.new_block_id];
		if (!I.aligned) { X.kind = 0; X.ia = s; X.len = I.end - I.start; }
		else { X.kind = 1; if (I.is_anchor) { X.ia = s; X.len = I.end - I.start; } else X.ib = s; }
		for (uint64_t k = G.S[s].member_off; k < G.S[s].member_off + G.S[s].n_kept; ++k) {
			const auto &M = G.M[k];
			const size_t i = where.at({C.block, M.member});
			const uint64_t id = hash_words({I.new_block_id, path_id[i], (uint64_t)(M.reverse ? 1 : 0), M.pos_start, M.pos_end});
			D.fresh[k] = pga_topo_node_t{id, M.pos_start, M.pos_end, 0, 0, M.reverse ? 1 : 0, 0};
			D.old[k] = G.N[i].node_id;
			X.members.push_back({id, k});
			block_of_member[k] = I.new_block_id;
		}
	}
	std::map<uint64_t, pga_topo_block_t> table;
	std::map<uint64_t, uint32_t> old_index;
	for (size_t b = 0; b < G.B.size(); ++b) if (G.B[b].alive && !cut_of.count((uint32_t)b)) { table[G.B[b].block_id] = pga_topo_block_t{G.B[b].block_id, G.B[b].cons_len, G.B[b].depth, 1, 0}; old_index[G.B[b].block_id] = (uint32_t)b; }
	for (const auto &kv : made) table[kv.first] = pga_topo_block_t{kv.first, kv.second.len, (uint32_t)kv.second.members.size(), 1, 0};
	std::map<uint64_t, uint32_t> index;
	for (const auto &kv : table) { index[kv.first] = (uint32_t)D.B.size(); D.B.push_back(kv.second); }
	D.map.assign(G.B.size(), TP_NONE);
	for (const auto &kv : old_index) D.map[kv.second] = index[kv.first];
	for (auto &kv : made) {
		std::sort(kv.second.members.begin(), kv.second.members.end());
		D.made.push_back(pga_apply_block_t{index[kv.first], kv.second.kind, kv.second.ia, kv.second.kind ? kv.second.ib : 0, D.src.size()});
		for (size_t s = 0; s < kv.second.members.size(); ++s) {
			const uint64_t k = kv.second.members[s].second;
			D.fresh[k].block = index[kv.first]; D.fresh[k].member = (uint32_t)s;
			D.src.push_back(k);
		}
	}
	for (const auto &P : G.P) {
		pga_topo_path_t Q{P.path_id, D.N.size(), 0, P.circular};
		for (uint64_t i = P.node_off; i < P.node_off + P.n_nodes; ++i) {
			const auto &A = G.N[i];
			if (!cut_of.count(A.block)) { pga_topo_node_t K = A; K.block = D.map[A.block]; D.N.push_back(K); continue; }
			const auto &C = G.cut[cut_of[A.block]];
			std::vector<pga_topo_node_t> mine;
			for (uint32_t j = 0; j < C.n_intervals; ++j) {
				const auto &R = G.S[C.first_interval + j];
				for (uint64_t k = R.member_off; k < R.member_off + R.n_kept; ++k) if (G.M[k].member == A.member) mine.push_back(D.fresh[k]);
			}
			if (A.reverse) std::reverse(mine.begin(), mine.end());
			D.N.insert(D.N.end(), mine.begin(), mine.end());
		}
		Q.n_nodes = (uint32_t)(D.N.size() - Q.node_off);
		D.P.push_back(Q);
	}
	return D;
}

// ---------------------------------------------------------------- the kernels, the sorts and the scans between them as plain loops
static void scan(const uint32_t *in, uint32_t *out, size_t n) { uint32_t run = 0; for (size_t i = 0; i < n; ++i) { out[i] = run; run += in[i]; } }
template <class K> static void sort_pairs(const K *kin, K *kout, const uint32_t *vin, uint32_t *vout, size_t n)
{
	std::vector<size_t> at(n);
	std::iota(at.begin(), at.end(), (size_t)0);
	std::stable_sort(at.begin(), at.end(), [&](size_t a, size_t b) { return kin[a] < kin[b]; });
	for (size_t i = 0; i < n; ++i) { kout[i] = kin[at[i]]; vout[i] = vin[at[i]]; }
}

static bool emulated(const Case &G, unsigned grid, Out &O, uint32_t terr[TP_ERRS], uint32_t err[AP_ERRS])
{
	ApTables A;
	ap_validate((int64_t)G.B.size(), G.B.data(), (int64_t)G.P.size(), G.P.data(), (int64_t)G.N.size(), G.N.data(), (int64_t)G.cut.size(), G.cut.data(), G.iv.data(), G.S.data(), G.M.data(), A);
	const uint64_t nn = G.N.size(), np = G.P.size(), nb = G.B.size(), nc = G.cut.size(), ni = A.n_intervals, nm = A.n_members, ne = A.entries.size(), ns = A.surv_ids.size();
	Exact<pga_topo_node_t> nodes(nn); Exact<pga_topo_path_t> paths(np); Exact<pga_topo_block_t> blocks(nb);
	std::copy(G.N.begin(), G.N.end(), nodes.get()); std::copy(G.P.begin(), G.P.end(), paths.get()); std::copy(G.B.begin(), G.B.end(), blocks.get());
	Exact<uint32_t> depth(nb), first(nb + 1), cutof(nb), matoff(nc + 1), ivcut(ni), iventry(ni), survrank(nb), iota(std::max(nm, ne));
	Exact<pga_apply_cut_t> cut(nc); Exact<pga_plan_interval_t> iv(ni); Exact<pga_slice_res_t> slices(ni); Exact<pga_slice_member_t> members(nm);
	Exact<ApEntry> entries(ne); Exact<tp_u64> eids(ne), seids(ne), survids(ns);
	std::copy(A.T.depth.begin(), A.T.depth.end(), depth.get()); std::copy(A.T.slot_first.begin(), A.T.slot_first.end(), first.get());
	std::copy(A.cut_of.begin(), A.cut_of.end(), cutof.get()); std::copy(A.mat_off.begin(), A.mat_off.end(), matoff.get());
	std::copy(A.iv_cut.begin(), A.iv_cut.end(), ivcut.get()); std::copy(A.iv_entry.begin(), A.iv_entry.end(), iventry.get());
	std::copy(A.surv_rank.begin(), A.surv_rank.end(), survrank.get()); std::iota(iota.get(), iota.get() + iota.n, 0u);
	std::copy(G.cut.begin(), G.cut.end(), cut.get()); std::copy(G.iv.begin(), G.iv.begin() + ni, iv.get()); std::copy(G.S.begin(), G.S.begin() + ni, slices.get());
	std::copy(G.M.begin(), G.M.begin() + nm, members.get()); std::copy(A.entries.begin(), A.entries.end(), entries.get());
	std::copy(A.entry_ids.begin(), A.entry_ids.end(), eids.get()); std::copy(A.surv_ids.begin(), A.surv_ids.end(), survids.get());
	Exact<uint32_t> pathof(nn), slot_cnt(A.T.n_slots), blk_cnt(nb), te(TP_ERRS), e(AP_ERRS);
	Exact<tp_u64> key(nn);
	std::fill(te.get(), te.get() + TP_ERRS, TP_NONE); std::fill(e.get(), e.get() + AP_ERRS, TP_NONE);
	TpDev T;
	memset(&T, 0, sizeof(T));
	T.n_nodes = nn; T.n_paths = np; T.n_blocks = nb; T.n_slots = A.T.n_slots;
	T.nodes = nodes.get(); T.paths = paths.get(); T.depth = depth.get(); T.slot_first = first.get(); T.path_of = pathof.get(); T.key = key.get();
	T.slot_cnt = slot_cnt.get(); T.blk_cnt = blk_cnt.get(); T.err = te.get();
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_keys(T); });
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_check(T); });
	Exact<uint32_t> slotpos(A.T.n_slots), mat(A.n_mat + 1), matscan(A.n_mat + 1), mslice(nm), ment(nm);
	Exact<pga_topo_node_t> fresh(nm); Exact<uint64_t> old(nm), msrc(nm); Exact<tp_u64> nkey(nm), nkey_s(nm);
	Exact<uint32_t> sentry(ne), erank(ne), rindex(ne), rdepth(ne + 1), rmoff(ne + 1), bmap(nb);
	Exact<pga_topo_block_t> oblocks(ns + ne); Exact<pga_apply_block_t> onew(ne);
	Exact<uint32_t> byid(nm), key2(nm), key2s(nm), byslot(nm);
	ApDev V;
	memset(&V, 0, sizeof(V));
	V.n_nodes = nn; V.n_paths = np; V.n_blocks = nb; V.n_intervals = ni; V.n_members = nm; V.n_mat = A.n_mat; V.n_entries = ne; V.n_surv = ns;
	V.nodes = nodes.get(); V.paths = paths.get(); V.blocks = blocks.get(); V.depth = depth.get(); V.slot_first = first.get(); V.path_of = pathof.get();
	V.cut_of = cutof.get(); V.cut = cut.get(); V.mat_off = matoff.get(); V.iv_cut = ivcut.get(); V.iv_entry = iventry.get();
	V.intervals = iv.get(); V.slices = slices.get(); V.members = members.get();
	V.slot_pos = slotpos.get(); V.mat = mat.get(); V.mat_scan = matscan.get(); V.m_slice = mslice.get(); V.m_ent = ment.get();
	V.o_new = fresh.get(); V.o_old = old.get(); V.node_key = nkey.get(); V.err = e.get();
	V.entries = entries.get(); V.sorted_ids = seids.get(); V.sorted_entry = sentry.get(); V.surv_ids = survids.get(); V.surv_rank = survrank.get();
	V.entry_rank = erank.get(); V.rank_index = rindex.get(); V.rank_depth = rdepth.get(); V.rank_moff = rmoff.get();
	V.block_map = bmap.get(); V.o_blocks = oblocks.get(); V.o_new_blocks = onew.get();
	V.by_id = byid.get(); V.key2 = key2.get(); V.key2_sorted = key2s.get(); V.by_slot = byslot.get(); V.member_src = msrc.get();
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_apply_slot_pos(V); });
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_apply_members(V); });
	sort_pairs(eids.get(), seids.get(), iota.get(), sentry.get(), ne);
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_apply_entries(V); });
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_apply_survivors(V); });
	scan(rdepth.get(), rmoff.get(), ne + 1);
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_apply_new_blocks(V); });
	sort_pairs(nkey.get(), nkey_s.get(), iota.get(), byid.get(), nm);
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_apply_key2(V); });
	sort_pairs(key2.get(), key2s.get(), byid.get(), byslot.get(), nm);
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_apply_slots(V); });
	std::copy(te.get(), te.get() + TP_ERRS, terr); std::copy(e.get(), e.get() + AP_ERRS, err);
	for (int i = 0; i < TP_ERRS; ++i) if (terr[i] != TP_NONE) return true;
	for (int i = 0; i < AP_ERRS; ++i) if (err[i] != TP_NONE) return true;
	const uint32_t n_tiles = (uint32_t)((nn + TP_TILE - 1) / TP_TILE);
	Exact<pga_topo_node_t> ordered(nm), nodes2(nn), onodes(A.n_out_nodes); Exact<pga_topo_path_t> opaths(np);
	Exact<uint32_t> cnt(nn), repl(nn), tsum(n_tiles), toff(n_tiles + 1), poff(nn + 1);
	V.ordered = ordered.get(); V.nodes2 = nodes2.get(); V.cnt = cnt.get(); V.repl = repl.get();
	scan(mat.get(), matscan.get(), A.n_mat + 1);
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_apply_order(V); });
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_apply_positions(V); });
	T.nodes = nodes2.get(); T.o_new = ordered.get(); T.cnt = cnt.get(); T.repl = repl.get(); T.n_tiles = n_tiles; T.tile_sum = tsum.get(); T.tile_off = toff.get(); T.pos_off = poff.get();
	T.o_nodes = onodes.get(); T.o_paths = opaths.get();
	if (n_tiles) {
		emu_launch(dim3(std::min<unsigned>(grid, n_tiles)), dim3(TP_THREADS), [&] { k_topo_tile_sums(T); });
		emu_launch(dim3(1), dim3(TP_THREADS), [&] { k_topo_tile_scan(T); });
		CHECK(toff[n_tiles] == A.n_out_nodes);
		emu_launch(dim3(std::min<unsigned>(grid, n_tiles)), dim3(TP_THREADS), [&] { k_topo_splice(T); });
	}
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_paths(T); });
	O.fresh.assign(fresh.get(), fresh.get() + nm); O.old.assign(old.get(), old.get() + nm); O.src.assign(msrc.get(), msrc.get() + nm);
	O.made.assign(onew.get(), onew.get() + ne); O.map.assign(bmap.get(), bmap.get() + nb);
	O.N.assign(onodes.get(), onodes.get() + onodes.n); O.P.assign(opaths.get(), opaths.get() + np); O.B.assign(oblocks.get(), oblocks.get() + oblocks.n);
	return true;
}

template <class T> static bool same(const std::vector<T> &a, const std::vector<T> &b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }

static bool run_case(const Case &G, unsigned grid)
{
	Out E, D = direct(G);
	uint32_t terr[TP_ERRS], err[AP_ERRS];
	if (G.cut.empty()) { ApTables A; ap_validate((int64_t)G.B.size(), G.B.data(), (int64_t)G.P.size(), G.P.data(), (int64_t)G.N.size(), G.N.data(), 0, nullptr, nullptr, nullptr, nullptr, A); return true; }   // (no launch)
	if (!emulated(G, grid, E, terr, err)) return false;
	for (int i = 0; i < TP_ERRS; ++i) CHECK(terr[i] == TP_NONE);
	for (int i = 0; i < AP_ERRS; ++i) CHECK(err[i] == TP_NONE);
	CHECK(same(E.fresh, D.fresh)); CHECK(same(E.old, D.old)); CHECK(same(E.made, D.made)); CHECK(same(E.src, D.src)); CHECK(same(E.map, D.map));
	CHECK(same(E.B, D.B)); CHECK(same(E.P, D.P)); CHECK(same(E.N, D.N));
	return true;
}

template <class F> static bool refused(F f) { try { f(); } catch (std::runtime_error &) { return true; } return false; }

int main()
{
	size_t n_cut = 0, n_big = 0, n_pairs = 0, n_empty = 0, n_rev = 0;
	for (g_case = 0; g_case < 10; ++g_case) {
		const bool big = g_case % 5 == 4, many = g_case % 5 == 3;           // more than one tile of the splice; 40 intervals on a block
		const Case G = generate(big ? 30 : 4 + rnd(8), big ? 12 : 4, 1 + rnd(4), many ? 40 : 4, big ? 2 * TP_TILE + rnd(50) : 0);
		if (!run_case(G, big ? 3 : 1 + rnd(3))) return 1;
		n_cut += G.cut.size(); n_big += G.N.size() > (size_t)TP_TILE;
		for (const auto &I : G.iv) n_pairs += I.aligned && I.is_anchor;
		for (const auto &R : G.S) n_empty += R.n_kept == 0;
		for (const auto &C : G.cut) for (const auto &N : G.N) n_rev += N.block == C.block && N.reverse && C.n_intervals > 1;
	}
	if (n_cut < 10 || n_big < 2 || n_pairs < 3 || n_empty < 3 || n_rev < 5) {
		fprintf(stderr, "apply_emu: the generator lost its cases (%zu cut blocks, %zu big, %zu pairs, %zu empty slices, %zu reverse nodes cut)\n", n_cut, n_big, n_pairs, n_empty, n_rev);
		return 1;
	}
	// ---- what is refused: on the host, and by the kernels before an index is derived
	g_case = -2;
	Case H;
	// H: two cut blocks and a survivor, two unaligned intervals, and the first slice keeps two members whose old nodes lie on one path
	auto old_path = [](const Case &Y, uint32_t member) {
		for (size_t i = 0; i < Y.N.size(); ++i) if (Y.N[i].block == Y.cut[0].block && Y.N[i].member == member) return tp_path_of(Y.P.data(), Y.P.size(), i);
		return TP_NONE;
	};
	auto fits = [&](const Case &Y) {
		if (Y.cut.size() < 2 || Y.S[0].n_kept < 2 || old_path(Y, Y.M[0].member) != old_path(Y, Y.M[1].member)) return false;
		size_t unaligned = 0, surv = 0;
		for (const auto &I : Y.iv) unaligned += !I.aligned;
		for (size_t b = 0; b < Y.B.size(); ++b) { bool is_cut = false; for (const auto &C : Y.cut) is_cut = is_cut || C.block == b; surv += Y.B[b].alive && !is_cut; }
		return unaligned >= 2 && surv >= 1;
	};
	do H = generate(10, 4, 2, 4, 0); while (!fits(H));
	auto host = [&](const Case &X) { ApTables A; ap_validate((int64_t)X.B.size(), X.B.data(), (int64_t)X.P.size(), X.P.data(), (int64_t)X.N.size(), X.N.data(), (int64_t)X.cut.size(), X.cut.data(), X.iv.data(), X.S.data(), X.M.data(), A); };
	host(H);
	bool ok = true;
	Case X = H; X.cut[0].block = (uint32_t)X.B.size();                  ok = ok && refused([&] { host(X); });
	X = H; X.cut[1].block = X.cut[0].block;                             ok = ok && refused([&] { host(X); });
	X = H; X.B[X.cut[0].block].alive = 0;                               ok = ok && refused([&] { host(X); });
	X = H; X.cut[0].n_intervals = 0;                                    ok = ok && refused([&] { host(X); });
	X = H; X.cut[1].first_interval += 1;                                ok = ok && refused([&] { host(X); });
	X = H; X.iv[0].end = X.iv[0].start;                                 ok = ok && refused([&] { host(X); });
	X = H; X.S[1].member_off += 1;                                      ok = ok && refused([&] { host(X); });
	X = H; X.N[0].member = X.B[X.N[0].block].depth;                     ok = ok && refused([&] { host(X); });
	X = H; X.iv[0].aligned = 1; X.iv[0].is_anchor = 1; X.iv[0].new_block_id = 999999999;   ok = ok && refused([&] { host(X); });
	if (!ok) { fprintf(stderr, "apply_emu: malformed input was accepted by the host\n"); return 1; }
	auto device = [&](const Case &Y, int which) {
		Out E; uint32_t terr[TP_ERRS], err[AP_ERRS];
		if (!emulated(Y, 2, E, terr, err)) return false;
		return (which < 0 ? terr[-which - 1] : err[which]) != TP_NONE && E.N.empty();
	};
	X = H; X.M[0].member = X.B[X.cut[0].block].depth + 5;               ok = ok && device(X, AP_E_MEMBER);
	X = H; X.M[1].member = X.M[0].member;                               ok = ok && device(X, AP_E_TWICE);
	{ X = H; size_t a = 0; while (X.iv[a].aligned) ++a; size_t b = a + 1; while (X.iv[b].aligned) ++b;
	  X.iv[b].new_block_id = X.iv[a].new_block_id; ok = ok && device(X, AP_E_NEWDUP); }
	{ X = H; size_t a = 0; while (X.iv[a].aligned) ++a;
	  for (size_t s = 0; s < X.B.size(); ++s) { bool is_cut = false; for (const auto &C : X.cut) is_cut = is_cut || C.block == s; if (X.B[s].alive && !is_cut) X.iv[a].new_block_id = X.B[s].block_id; }
	  ok = ok && device(X, AP_E_CONFLICT); }
	X = H; X.M[1] = X.M[0]; X.M[1].member = H.M[1].member;               // two members of one slice with one strand and position, their old nodes on one path
	ok = ok && device(X, AP_E_NODEDUP);
	{ X = H; size_t i = 1; while (i < X.N.size() && X.N[i].block != X.N[0].block) ++i; if (i < X.N.size()) { X.N[i].member = X.N[0].member; ok = ok && device(X, -(TP_E_SLOT + 1)); } }
	if (!ok) { fprintf(stderr, "apply_emu: malformed input passed the kernels' checks\n"); return 1; }
	// ---- an empty cut, and the lookups at their edges
	{ ApTables A; Case Z = H; Z.cut.clear(); ap_validate((int64_t)Z.B.size(), Z.B.data(), (int64_t)Z.P.size(), Z.P.data(), (int64_t)Z.N.size(), Z.N.data(), 0, nullptr, nullptr, nullptr, nullptr, A); }
	const pga_slice_res_t offs[5] = {{0, 2, 0}, {2, 0, 0}, {2, 0, 0}, {2, 3, 0}, {5, 0, 0}};
	const tp_u64 ids[3] = {5, 9, ~0ULL};
	if (ap_slice_of(offs, 5, 0) != 0 || ap_slice_of(offs, 5, 1) != 0 || ap_slice_of(offs, 5, 2) != 3 || ap_slice_of(offs, 5, 4) != 3 ||
	    ap_below(ids, 3, 0) != 0 || ap_below(ids, 3, 5) != 0 || ap_below(ids, 3, 6) != 1 || ap_below(ids, 3, ~0ULL) != 2 || ap_below(ids, 0, 7) != 0) { fprintf(stderr, "apply_emu: a lookup is off\n"); return 1; }
	printf("apply_emu OK (%zu cut blocks, %zu graphs of more than one tile, %zu merged pairs, %zu empty slices)\n", n_cut, n_big, n_pairs, n_empty);
	return 0;
}
