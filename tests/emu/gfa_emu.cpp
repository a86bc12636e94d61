// pga_gfa_idx.h without a device: validation and the tables, then every kernel of the header (and the graph checks, run heads and run starts
// of pga_topo_idx.h) under dev/emu/hip_emu.h, with every buffer allocated at exactly the size the kernels may touch (under the address
// sanitizer an access one entry out is an error), against a direct scalar construction of io/gfa.rs:79-279: segments in a map, paths
// filtered into new vectors, links counted in a map, the text printed line by line.  The tiles are cut at several sizes, so that every kind
// of item is cut by a tile edge somewhere; std::sort stands in for the two radix sorts, a loop for the scan over the run heads.
// Build and run (host only):  g++ -std=c++17 -g -O1 -DPGA_EMU -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined
//                             tests/emu/gfa_emu.cpp -o gfa_emu && ./gfa_emu
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <set>
#include <string>
#include "../../dev/emu/hip_emu.h"
#include "../../pangraph_amd/csrc/pga_gfa_idx.h"

using namespace pga;

template <class T> struct Exact {                                       // n entries, not one more
	std::unique_ptr<T[]> p; size_t n;
	explicit Exact(size_t n_) : p(n_ ? new T[n_]() : nullptr), n(n_) {}
	T *get() { return p.get(); }
	T &operator[](size_t i) { return p[i]; }
};

static std::mt19937_64 rng(20261020);
static uint32_t rnd(uint32_t n) { return n ? (uint32_t)(rng() % n) : 0u; }
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "gfa_emu: %s:%d: %s (case %d)\n", __FILE__, __LINE__, #c, g_case); return false; } } while (0)
static int g_case = -1;

struct Case {
	std::vector<pga_topo_block_t> B; std::vector<pga_topo_path_t> P; std::vector<pga_topo_node_t> N;
	std::vector<std::string> cons, names; std::vector<const char*> cons_p, names_p; std::vector<uint32_t> name_len;
	void point() { cons_p.clear(); names_p.clear(); name_len.clear(); for (auto &c : cons) cons_p.push_back(c.data()); for (auto &s : names) { names_p.push_back(s.data()); name_len.push_back((uint32_t)s.size()); } }
};
struct Out {
	std::vector<pga_gfa_segment_t> S; std::vector<pga_topo_edge_t> L; std::vector<pga_gfa_path_t> P; std::vector<pga_gfa_step_t> T; std::string text;
};

// ---------------------------------------------------------------- cases: blocks with ids of every width, paths that visit a block twice
static Case generate(uint32_t n_blocks, uint32_t n_paths, uint32_t max_len, uint32_t filler)
{
	Case G;
	static const uint64_t EDGE[] = {9, 10, 99, 100, 9999999999999999999ULL, 10000000000000000000ULL, ~0ULL};
	std::set<uint64_t> ids(EDGE, EDGE + 7);
	while (ids.size() < n_blocks) ids.insert(rnd(4) ? 1 + rnd(100000) : rng());
	for (uint64_t id : ids) {
		if (rnd(6) == 0) G.B.push_back(pga_topo_block_t{id ? id - 1 : 0, 7, 3, 0, 0});       // a dead entry (its id is not held against the others)
		G.B.push_back(pga_topo_block_t{id, rnd(5) ? 1 + rnd(max_len) : 0u, 0, 1, 0});
	}
	std::vector<uint32_t> alive;
	for (uint32_t b = 0; b < G.B.size(); ++b) if (G.B[b].alive) alive.push_back(b);
	std::vector<std::vector<uint32_t>> walk(n_paths);
	for (uint32_t b : alive) for (uint32_t d = 1 + rnd(4); d; --d) walk[rnd(n_paths)].push_back(b);
	for (uint32_t f = 0; f < filler; ++f) walk[0].push_back(alive[rnd((uint32_t)alive.size())]);
	uint64_t nid = 1000;
	static const char pool[] = "ACGTACGTTGCA";
	for (uint32_t p = 0; p < n_paths; ++p) {
		if (p == 1) walk[p].clear();                                                      // an empty path
		std::shuffle(walk[p].begin(), walk[p].end(), rng);
		G.P.push_back(pga_topo_path_t{10 + 3 * (uint64_t)p, G.N.size(), (uint32_t)walk[p].size(), (int32_t)rnd(2)});
		for (uint32_t b : walk[p]) G.N.push_back(pga_topo_node_t{++nid, 0, 0, b, G.B[b].depth++, (int32_t)rnd(2), 0});
		std::string name = p == 2 ? "" : "path \xc3\xa9 " + std::to_string(p);
		if (p == 0) name.append(rnd(300), 'n');
		G.names.push_back(name);
	}
	for (auto &b : G.B) { std::string c(b.cons_len, 'A'); for (char &x : c) x = pool[rnd(12)]; G.cons.push_back(c); }
	G.point();
	return G;
}

// ---------------------------------------------------------------- the direct construction (by block id, as the reference holds them)
static Out direct(const Case &G, const pga_gfa_params_t &prm)
{
	Out D;
	struct Seg { uint32_t block; uint64_t length, depth; bool dup; };
	std::map<uint64_t, Seg> segs;
	for (uint32_t b = 0; b < G.B.size(); ++b) if (G.B[b].alive) segs[G.B[b].block_id] = Seg{b, G.B[b].cons_len, G.B[b].depth, false};
	for (auto &P : G.P) { std::set<uint32_t> seen; for (uint64_t i = P.node_off; i < P.node_off + P.n_nodes; ++i) if (!seen.insert(G.N[i].block).second) segs[G.B[G.N[i].block].block_id].dup = true; }
	typedef std::pair<uint64_t, int> SN;
	std::map<std::tuple<uint64_t, uint64_t, int, int>, uint32_t> links;
	std::set<uint64_t> used;
	std::vector<std::pair<uint32_t, std::vector<SN>>> paths;
	for (uint32_t p = 0; p < G.P.size(); ++p) {
		std::vector<SN> kept;
		for (uint64_t i = G.P[p].node_off; i < G.P[p].node_off + G.P[p].n_nodes; ++i) {
			const Seg &S = segs[G.B[G.N[i].block].block_id];
			if (S.length >= prm.min_len && S.length <= prm.max_len && S.depth >= prm.min_depth && S.depth <= prm.max_depth && !(prm.no_duplicated && S.dup)) kept.push_back(SN(G.B[G.N[i].block].block_id, G.N[i].reverse ? 1 : 0));
		}
		if (kept.empty()) continue;
		auto add = [&](SN a, SN b) {
			if (!(a.first < b.first || (a.first == b.first && a.second == 0))) { const SN x = a; a = SN(b.first, !b.second); b = SN(x.first, !x.second); }
			++links[std::make_tuple(a.first, b.first, a.second, b.second)];
		};
		for (size_t k = 0; k + 1 < kept.size(); ++k) add(kept[k], kept[k + 1]);
		if (G.P[p].circular) add(kept.back(), kept[0]);
		D.P.push_back(pga_gfa_path_t{p, (uint32_t)kept.size(), D.T.size(), 0});
		for (auto &k : kept) { used.insert(k.first); D.T.push_back(pga_gfa_step_t{segs[k.first].block, k.second}); }
		paths.push_back(std::make_pair(p, kept));
	}
	std::string &t = D.text;
	t = "H\tVN:Z:1.0\n";
	if (!used.empty()) t += "# blocks\n";
	for (uint64_t id : used) {
		const Seg &S = segs[id];
		D.S.push_back(pga_gfa_segment_t{S.block, (uint32_t)S.depth, (uint32_t)S.length, S.dup ? 1 : 0, t.size()});
		t += "S\t" + std::to_string(id) + "\t" + (prm.include_sequences ? G.cons[S.block] : std::string("*")) + "\tRC:i:" + std::to_string(S.depth * S.length) + "\tLN:i:" + std::to_string(S.length) + (S.dup ? "\tTP:Z:duplicated" : "") + "\n";
	}
	if (!links.empty()) t += "# edges\n";
	for (auto &kv : links) {
		uint64_t b1, b2; int s1, s2; std::tie(b1, b2, s1, s2) = kv.first;
		D.L.push_back(pga_topo_edge_t{segs[b1].block, segs[b2].block, s1, s2, kv.second, 0});
		t += "L\t" + std::to_string(b1) + "\t" + (s1 ? "-" : "+") + "\t" + std::to_string(b2) + "\t" + (s2 ? "-" : "+") + "\t*\tRC:i:" + std::to_string(kv.second) + "\n";
	}
	if (!paths.empty()) t += "# paths\n";
	for (size_t k = 0; k < paths.size(); ++k) {
		D.P[k].byte_off = t.size();
		t += "P\t" + G.names[paths[k].first] + "\t";
		for (size_t j = 0; j < paths[k].second.size(); ++j) t += (j ? "," : "") + std::to_string(paths[k].second[j].first) + (paths[k].second[j].second ? "-" : "+");
		t += std::string("\t*") + (G.P[paths[k].first].circular ? "\tTP:Z:circular" : "") + "\n";
	}
	return D;
}

// ---------------------------------------------------------------- the kernels in the order of pga_gfa.hip
struct ScanBufs {
	Exact<gf_u64> tile_sum, tile_off, off; GfScan S; TsArray<gf_u64> val;
	ScanBufs(const gf_u64 *val_, uint64_t n) : tile_sum((n + GF_TILE - 1) / GF_TILE), tile_off((n + GF_TILE - 1) / GF_TILE + 1), off(n + 1),
		S{n, (uint32_t)((n + GF_TILE - 1) / GF_TILE), 1, tile_sum.get(), tile_off.get(), off.get()}, val{val_} {}
};
static void scan(const ScanBufs &B, unsigned grid)
{
	const GfScan &S = B.S;
	if (S.n_tiles) emu_launch(dim3(std::min<unsigned>(grid, S.n_tiles)), dim3(GF_THREADS), [&] { k_ts_sums<gf_u64, TsArray<gf_u64>>(S, B.val); });
	emu_launch(dim3(1), dim3(GF_THREADS), [&] { k_ts_scan<gf_u64>(S); });
	if (S.n_tiles) emu_launch(dim3(std::min<unsigned>(grid, S.n_tiles)), dim3(GF_THREADS), [&] { k_ts_offsets<gf_u64, TsArray<gf_u64>>(S, B.val); });
}

// returns false on a CHECK; `refused`: the device checks stopped the call
static bool emulated(const Case &G, unsigned grid, const pga_gfa_params_t &prm, const std::vector<uint64_t> &tile_sizes, Out &O, uint32_t terr[TP_ERRS], bool &refused,
                     size_t *n_cut = nullptr)
{
	TpTables T;
	gf_validate((int64_t)G.B.size(), G.B.data(), (int64_t)G.P.size(), G.P.data(), (int64_t)G.N.size(), G.N.data(), G.cons_p.data(), &prm, PGA_GFA_STEPS, T);
	const uint64_t nn = G.N.size(), np = G.P.size(), nb = G.B.size();
	refused = false;
	Exact<pga_topo_node_t> nodes(nn); Exact<pga_topo_path_t> paths(np); Exact<pga_topo_block_t> blocks(nb);
	Exact<uint32_t> depth(nb), first(nb + 1), pathof(nn), slot_cnt(T.n_slots), blk_cnt(nb), te(TP_ERRS), dup(nb), used(nb), steppath(nn), head(nn + 1), hoff(nn + 1), rstart(nn + 1);
	Exact<tp_u64> key(nn), k0(nn), k1(nn); Exact<gf_u64> keep(nn), psteps(2 * np);
	Exact<pga_gfa_step_t> steps(nn); Exact<pga_topo_edge_t> links(nn);
	std::copy(G.N.begin(), G.N.end(), nodes.get()); std::copy(G.P.begin(), G.P.end(), paths.get()); std::copy(G.B.begin(), G.B.end(), blocks.get());
	std::copy(T.depth.begin(), T.depth.end(), depth.get()); std::copy(T.slot_first.begin(), T.slot_first.end(), first.get());
	std::fill(te.get(), te.get() + TP_ERRS, TP_NONE); std::fill(k0.get(), k0.get() + nn, TP_NOKEY);
	TpDev K;
	memset(&K, 0, sizeof(K));
	K.n_nodes = nn; K.n_paths = np; K.n_blocks = nb; K.n_slots = T.n_slots;
	K.nodes = nodes.get(); K.paths = paths.get(); K.depth = depth.get(); K.slot_first = first.get(); K.path_of = pathof.get(); K.key = key.get();
	K.slot_cnt = slot_cnt.get(); K.blk_cnt = blk_cnt.get(); K.err = te.get();
	ScanBufs b_keep(keep.get(), nn);
	GfDev V;
	memset(&V, 0, sizeof(V));
	V.n_nodes = nn; V.n_paths = np; V.n_blocks = nb; V.nodes = nodes.get(); V.paths = paths.get(); V.blocks = blocks.get(); V.path_of = pathof.get(); V.prm = prm;
	V.dup = dup.get(); V.used = used.get(); V.keep = keep.get(); V.koff = b_keep.S.off; V.steps = steps.get(); V.step_path = steppath.get(); V.path_steps = psteps.get(); V.links = links.get();
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_keys(K); });
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_check(K); });
	V.dkey = key.get(); V.dskey = k1.get();
	emu_launch(dim3(grid), dim3(GF_THREADS), [&] { k_gfa_dupkeys(V); });
	std::copy(key.get(), key.get() + nn, k1.get()); std::sort(k1.get(), k1.get() + nn);
	emu_launch(dim3(grid), dim3(GF_THREADS), [&] { k_gfa_dupflags(V); });
	emu_launch(dim3(grid), dim3(GF_THREADS), [&] { k_gfa_keep(V); });
	scan(b_keep, grid);
	emu_launch(dim3(grid), dim3(GF_THREADS), [&] { k_gfa_steps(V); });
	emu_launch(dim3(grid), dim3(GF_THREADS), [&] { k_gfa_path_steps(V); });
	V.lkey = k0.get(); V.lskey = k1.get(); V.head_off = hoff.get(); V.run_start = rstart.get();
	K.skey = k1.get(); K.head = head.get(); K.head_off = hoff.get(); K.run_start = rstart.get();
	emu_launch(dim3(grid), dim3(GF_THREADS), [&] { k_gfa_link_keys(V); });
	std::copy(k0.get(), k0.get() + nn, k1.get()); std::sort(k1.get(), k1.get() + nn);
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_heads(K); });
	{ uint32_t run = 0; for (uint64_t i = 0; i <= nn; ++i) { hoff[i] = run; run += head[i]; } }
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_runs(K); });
	emu_launch(dim3(grid), dim3(GF_THREADS), [&] { k_gfa_links(V); });
	std::copy(te.get(), te.get() + TP_ERRS, terr);
	for (int i = 0; i < TP_ERRS; ++i) if (terr[i] != TP_NONE) { refused = true; return true; }
	const uint64_t n_steps = b_keep.off[nn], n_links = hoff[nn];
	CHECK(n_steps <= nn && n_links <= n_steps);
	GfTables H;
	gf_tables((int64_t)nb, G.B.data(), (int64_t)np, G.P.data(), G.cons_p.data(), G.names_p.data(), G.name_len.data(), prm, used.get(), dup.get(), psteps.get(), n_steps, n_links, H);
	O.T.assign(steps.get(), steps.get() + n_steps); O.L.assign(links.get(), links.get() + n_links);
	O.text = "H\tVN:Z:1.0\n";
	if (n_steps == 0) { CHECK(H.segs.empty() && H.paths.empty() && n_links == 0); return true; }
	const uint64_t n_seg = H.segs.size(), n_rows = H.rows.size(), n_items = 4 + n_seg + n_links + n_steps + 2 * n_rows;
	Exact<pga_gfa_segment_t> segs(n_seg); Exact<GfRow> rows(n_rows); Exact<gf_u64> len(n_items), rowoff(n_rows);
	std::copy(H.segs.begin(), H.segs.end(), segs.get()); std::copy(H.rows.begin(), H.rows.end(), rows.get());
	ScanBufs b_items(len.get(), n_items);
	V.n_seg = n_seg; V.n_links = n_links; V.n_rows = n_rows; V.n_steps = n_steps; V.n_items = n_items;
	V.segs = segs.get(); V.rows = rows.get(); V.len = len.get(); V.off = b_items.S.off; V.row_off = rowoff.get();
	emu_launch(dim3(grid), dim3(GF_THREADS), [&] { k_gfa_lens(V); });
	scan(b_items, grid);
	emu_launch(dim3(grid), dim3(GF_THREADS), [&] { k_gfa_row_off(V); });
	const uint64_t n_bytes = b_items.off[n_items];
	for (uint64_t k = 0; k < n_seg; ++k) H.segs[k].byte_off = b_items.off[2 + k];
	for (uint64_t k = 0; k < n_rows; ++k) H.paths[k].byte_off = rowoff[k];
	O.S = H.segs; O.P = H.paths;
	// ---- the tiles, at every size asked for: the same text each time; the letters and names are the host's
	std::string last;
	for (uint64_t tb : tile_sizes) {
		std::string text;
		size_t si = 0, pi = 0;
		for (uint64_t t0 = 0; t0 < n_bytes; t0 += tb) {
			const uint64_t t1 = std::min(n_bytes, t0 + tb);
			Exact<char> tile(t1 - t0);
			memset(tile.get(), '?', t1 - t0);
			GfDev W = V;
			W.tile = tile.get(); W.t0 = t0; W.t1 = t1;
			emu_launch(dim3(grid), dim3(GF_THREADS), [&] { k_gfa_tile(W); });
			gf_host_fill(H, G.B.data(), G.cons_p.data(), G.names_p.data(), prm.include_sequences != 0, tile.get(), t0, t1, si, pi);
			text.append(tile.get(), t1 - t0);
			if (n_cut) for (uint64_t x = 0; x < n_items; ++x) *n_cut += b_items.off[x] < t1 && b_items.off[x + 1] > t1;
		}
		CHECK(text.size() == n_bytes);
		CHECK(last.empty() || last == text);
		last = text;
	}
	O.text = last;
	return true;
}

template <class T> static bool same(const std::vector<T> &a, const std::vector<T> &b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }

static bool run_case(const Case &G, unsigned grid, const pga_gfa_params_t &prm, const std::vector<uint64_t> &tiles, size_t *n_cut = nullptr, size_t *n_dropped = nullptr)
{
	Out E, D = direct(G, prm);
	uint32_t terr[TP_ERRS]; bool refused;
	if (!emulated(G, grid, prm, tiles, E, terr, refused, n_cut)) return false;
	CHECK(!refused);
	if (E.text != D.text) {
		size_t at = 0; while (at < E.text.size() && at < D.text.size() && E.text[at] == D.text[at]) ++at;
		fprintf(stderr, "gfa_emu: the text differs at byte %zu of %zu / %zu\n---- expected\n%s\n---- got\n%s\n", at, D.text.size(), E.text.size(), D.text.substr(at > 40 ? at - 40 : 0, 120).c_str(), E.text.substr(at > 40 ? at - 40 : 0, 120).c_str());
	}
	CHECK(E.text == D.text); CHECK(same(E.S, D.S)); CHECK(same(E.L, D.L)); CHECK(same(E.P, D.P)); CHECK(same(E.T, D.T));
	if (n_dropped) *n_dropped += G.N.size() - D.T.size();
	return true;
}

template <class F> static bool refused_by_host(F f, const char *what = "") { try { f(); } catch (std::runtime_error &e) { return strstr(e.what(), what) != nullptr; } return false; }

int main()
{
	const pga_gfa_params_t ALL{0, ~0ULL, 0, ~0ULL, 0, 0};
	size_t n_cut = 0, n_dropped = 0, n_big = 0;
	for (g_case = 0; g_case < 8; ++g_case) {
		const bool big = g_case == 5;                          // more than two tiles of positions and of items
		const Case G = big ? generate(40, 4, 30, 2 * GF_TILE + 77) : generate(8 + rnd(10), 3 + rnd(4), g_case == 3 ? 400 : 40, 0);
		pga_gfa_params_t prm = ALL;
		prm.include_sequences = g_case & 1;
		if (g_case == 2) { prm.min_len = 10; prm.max_len = 30; }
		if (g_case == 4) { prm.min_depth = 2; prm.max_depth = 3; }
		if (g_case == 6) prm.no_duplicated = 1;
		if (g_case == 7) prm.min_len = 1000000;                 // everything is filtered
		const std::vector<uint64_t> tiles = big ? std::vector<uint64_t>{4096, 1000003} : std::vector<uint64_t>{251, 1000003};
		if (!run_case(G, 1 + rnd(3), prm, tiles, &n_cut, &n_dropped)) return 1;
		n_big += G.N.size() > (size_t)2 * GF_TILE;
	}
	if (n_cut < 40 || n_dropped < 30 || n_big != 1) { fprintf(stderr, "gfa_emu: the generator lost its cases (%zu items cut, %zu nodes dropped, %zu big)\n", n_cut, n_dropped, n_big); return 1; }
	// ---- a hand-made graph: self links, both wraps, neighbours across a filtered node
	{
		g_case = 100;
		Case G;
		G.B = {pga_topo_block_t{5, 4, 3, 1, 0}, pga_topo_block_t{6, 9, 1, 1, 0}, pga_topo_block_t{7, 4, 2, 1, 0}};
		G.P = {pga_topo_path_t{0, 0, 3, 1}, pga_topo_path_t{1, 3, 1, 1}, pga_topo_path_t{2, 4, 2, 0}};
		G.N = {pga_topo_node_t{1, 0, 0, 0, 0, 0, 0}, pga_topo_node_t{2, 0, 0, 1, 0, 0, 0}, pga_topo_node_t{3, 0, 0, 2, 0, 1, 0}, pga_topo_node_t{4, 0, 0, 0, 1, 1, 0},
		       pga_topo_node_t{5, 0, 0, 2, 1, 0, 0}, pga_topo_node_t{6, 0, 0, 0, 2, 1, 0}};
		G.cons = {"ACGT", "ACGTACGTA", "TTTT"}; G.names = {"a", "b", "c"}; G.point();
		pga_gfa_params_t prm = ALL; prm.max_len = 4;
		Out E; uint32_t terr[TP_ERRS]; bool refused;
		if (!emulated(G, 2, prm, {13, 1000}, E, terr, refused) || refused) return 1;
		const char *want = "H\tVN:Z:1.0\n# blocks\nS\t5\t*\tRC:i:12\tLN:i:4\nS\t7\t*\tRC:i:8\tLN:i:4\n# edges\nL\t5\t+\t5\t+\t*\tRC:i:1\nL\t5\t+\t7\t-\t*\tRC:i:2\nL\t5\t-\t7\t+\t*\tRC:i:1\n"
		                   "# paths\nP\ta\t5+,7-\t*\tTP:Z:circular\nP\tb\t5-\t*\tTP:Z:circular\nP\tc\t7+,5-\t*\n";
		if (E.text != want) { fprintf(stderr, "gfa_emu: the hand-made graph gives\n%s", E.text.c_str()); return 1; }
		if (!run_case(G, 1, prm, {9})) return 1;
	}
	// ---- decimal widths at every edge
	{
		gf_u64 p = 1;
		for (uint32_t w = 1; w <= 20; ++w, p *= 10) {
			if (gf_width(p) != w || (w > 1 && gf_width(p - 1) != w - 1)) { fprintf(stderr, "gfa_emu: the width of 10^%u is off\n", w - 1); return 1; }
			char buf[24]; GfOut O{buf, 0, 24, 0}; gf_dec(O, p + p / 3);
			if (std::string(buf, O.at) != std::to_string(p + p / 3)) { fprintf(stderr, "gfa_emu: a number is misprinted\n"); return 1; }
		}
		if (gf_width(0) != 1 || gf_width(~0ULL) != 20) return 1;
	}
	// ---- what is refused: on the host, and by the kernels before an index is derived
	g_case = -2;
	Case H;
	auto fits = [](const Case &Y) { size_t i = 1; while (i < Y.N.size() && Y.N[i].block != Y.N[0].block) ++i; bool dead = false; for (auto &b : Y.B) dead = dead || !b.alive; return dead && i < Y.N.size() && Y.B[Y.N[0].block].cons_len > 0 && Y.P[0].n_nodes > 0; };
	do H = generate(10, 3, 40, 0); while (!fits(H));
	pga_gfa_params_t SEQ = ALL; SEQ.include_sequences = 1;
	auto host = [&](const Case &X, const pga_gfa_params_t *prm, uint32_t flags = 0, bool null_cons = false) {
		TpTables T;
		gf_validate((int64_t)X.B.size(), X.B.data(), (int64_t)X.P.size(), X.P.data(), (int64_t)X.N.size(), X.N.data(), null_cons ? nullptr : X.cons_p.data(), prm, flags, T);
	};
	host(H, &SEQ, PGA_GFA_STEPS);
	bool ok = true;
	size_t dead = 0; while (H.B[dead].alive) ++dead;
	Case X = H; X.N[0].member = X.B[X.N[0].block].depth;               ok = ok && refused_by_host([&] { host(X, &ALL); });
	X = H; X.N[0].block = (uint32_t)X.B.size();                        ok = ok && refused_by_host([&] { host(X, &ALL); });
	X = H; X.N[0].block = (uint32_t)dead;                              ok = ok && refused_by_host([&] { host(X, &ALL); });
	X = H; X.P[1].node_off += 1;                                       ok = ok && refused_by_host([&] { host(X, &ALL); });
	X = H; X.P[2].path_id = X.P[0].path_id;                            ok = ok && refused_by_host([&] { host(X, &ALL); });
	{ X = H; size_t a = 0; while (!X.B[a].alive) ++a; size_t b = a + 1; while (!X.B[b].alive) ++b; X.B[b].block_id = X.B[a].block_id; ok = ok && refused_by_host([&] { host(X, &ALL); }); }
	ok = ok && refused_by_host([&] { host(H, nullptr); }, "null parameters");
	ok = ok && refused_by_host([&] { host(H, &ALL, 2); }, "unknown flag");
	ok = ok && refused_by_host([&] { host(H, &SEQ, 0, true); }, "without consensus letters");
	{ pga_gfa_params_t B = ALL; B.min_len = 5; B.max_len = 4; ok = ok && refused_by_host([&] { host(H, &B); }, "minimum_length above maximum_length"); }
	{ pga_gfa_params_t B = ALL; B.min_depth = 5; B.max_depth = 4; ok = ok && refused_by_host([&] { host(H, &B); }, "minimum_depth above maximum_depth"); }
	if (!ok) { fprintf(stderr, "gfa_emu: malformed input was accepted by the host\n"); return 1; }
	auto device = [&](const Case &Y, int which) {
		Out E; uint32_t terr[TP_ERRS]; bool refused;
		if (!emulated(Y, 2, ALL, {512}, E, terr, refused)) return false;
		return refused && terr[which] != TP_NONE && E.text.empty();
	};
	{ X = H; size_t i = 1; while (X.N[i].block != X.N[0].block) ++i; X.N[i].member = X.N[0].member; ok = ok && device(X, TP_E_SLOT); }
	{ X = H; X.B[X.N[0].block].depth += 1; ok = ok && device(X, TP_E_DEPTH); }
	if (!ok) { fprintf(stderr, "gfa_emu: malformed input passed the kernels' checks\n"); return 1; }
	// behind the first wait: a NULL consensus or name of something emitted, NULL names; the same of something filtered is not read
	auto late = [&](const Case &Y, const pga_gfa_params_t &prm, const char *what) {
		Out E; uint32_t terr[TP_ERRS]; bool refused;
		return refused_by_host([&] { emulated(Y, 1, prm, {512}, E, terr, refused); }, what);
	};
	{ X = H; X.cons_p[X.N[0].block] = nullptr; ok = ok && late(X, SEQ, "null consensus of an emitted block"); }
	{ X = H; X.names_p[0] = nullptr; ok = ok && late(X, ALL, "null name of an emitted path (path 0)"); }
	{ X = H; pga_gfa_params_t F = SEQ; F.min_len = X.B[X.N[0].block].cons_len + 1u; X.cons_p[X.N[0].block] = nullptr; X.names_p[0] = nullptr; X.name_len[0] = 0; ok = ok && !late(X, F, ""); }   // (filtered, or empty: not read)
	{
		TpTables T; GfTables Gt;
		const uint32_t used1[1] = {0}, dup1[1] = {0}; const gf_u64 ps[2] = {0, 1};
		const pga_topo_block_t b1{1, 1, 1, 1, 0}; const pga_topo_path_t p1{0, 0, 1, 0};
		ok = ok && refused_by_host([&] { gf_tables(1, &b1, 1, &p1, nullptr, nullptr, nullptr, ALL, used1, dup1, ps, 1, 0, Gt); }, "null names with a path to emit");
		const char *nm[1] = {"x"}; const uint32_t nl[1] = {1};
		ok = ok && refused_by_host([&] { GfTables G2; gf_tables(1, &b1, 1, &p1, nullptr, nm, nl, ALL, used1, dup1, ps, 1ULL << 60, 0, G2); }, "a file of 2^63 bytes or more");   // 2^60 steps of 22 bytes
	}
	if (!ok) { fprintf(stderr, "gfa_emu: a refusal behind the first wait is off\n"); return 1; }
	// ---- the lookup at its edges
	const gf_u64 offs[6] = {0, 2, 2, 2, 5, 5};
	if (ts_last_le(offs, 0, 5, 0) != 0 || ts_last_le(offs, 0, 5, 1) != 0 || ts_last_le(offs, 0, 5, 2) != 3 || ts_last_le(offs, 0, 5, 4) != 3 || ts_last_le(offs, 3, 4, 4) != 3) { fprintf(stderr, "gfa_emu: a lookup is off\n"); return 1; }
	printf("gfa_emu OK (%zu items cut by a tile edge, %zu nodes filtered, %zu graphs of more than two tiles)\n", n_cut, n_dropped, n_big);
	return 0;
}
