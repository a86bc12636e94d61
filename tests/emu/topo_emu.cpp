// pga_topo_idx.h without a device: validation and the tables, then every kernel of the header under dev/emu/hip_emu.h -- the radix sort and
// the two scans of pga_topo.hip replaced by std::sort and plain loops -- with every buffer allocated at exactly the size the kernels may touch
// (under the address sanitizer an access one entry out is an error), against a direct scalar construction of one round of
// remove_transitive_edges (circularize.rs:11-76, merge_blocks.rs:33-89 and :196-234): maps and loops over every path, once per merged edge.
// Build and run (host only):  g++ -std=c++17 -g -O1 -DPGA_EMU -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined
//                             tests/emu/topo_emu.cpp -o topo_emu && ./topo_emu
#include <cstdio>
#include <array>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <set>
#include <string>
#include "../../dev/emu/hip_emu.h"
#include "../../pangraph_amd/csrc/pga_topo_idx.h"
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
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "topo_emu: %s:%d: %s (graph %d)\n", __FILE__, __LINE__, #c, g_graph); return false; } } while (0)
static int g_graph = -1;

struct Graph { std::vector<pga_topo_block_t> B; std::vector<pga_topo_path_t> P; std::vector<pga_topo_node_t> N; };
struct Out {
	std::vector<pga_topo_edge_t> trans, counts; std::vector<pga_topo_round_t> round; std::vector<uint32_t> partner;
	std::vector<pga_topo_node_t> fresh; std::vector<uint64_t> old_left, old_right; Graph after;
};

// ---------------------------------------------------------------- graphs: super-blocks cut into pieces, laid on paths in both directions
static Graph generate(uint32_t max_paths, uint32_t max_occ, bool filler)
{
	Graph G;
	struct Piece { uint32_t blk; int rev; };
	const uint32_t n_super = 2 + rnd(6);
	std::vector<std::vector<Piece>> supers(n_super);
	std::set<uint64_t> ids;
	const uint32_t lens[6] = {0, 5, 8, 8, 13, 40};
	for (auto &S : supers) {
		const uint32_t n = 1 + rnd(4);
		for (uint32_t k = 0; k < n; ++k) {
			if (rnd(5) == 0) G.B.push_back(pga_topo_block_t{0, 7, 3, 0, 0});            // a dead entry: skipped
			S.push_back(Piece{(uint32_t)G.B.size(), (int)rnd(2)});
			G.B.push_back(pga_topo_block_t{0, lens[rnd(6)], 0, 1, 0});
		}
	}
	while (ids.size() < G.B.size()) ids.insert(1 + rnd(100000));
	{ auto it = ids.begin(); for (auto &b : G.B) b.block_id = *it++; }                  // ascending with the index
	const uint32_t n_paths = 1 + rnd(max_paths);
	uint64_t nid = 1000;
	for (uint32_t p = 0; p < n_paths; ++p) {
		pga_topo_path_t P{10 + 3 * (uint64_t)p, G.N.size(), 0, (int32_t)rnd(2)};
		uint64_t at = 17 * p;
		const uint32_t n_occ = rnd(max_occ + 1);
		for (uint32_t o = 0; o < n_occ; ++o) {
			std::vector<Piece> S = supers[filler && rnd(4) ? 0 : rnd(n_super)];
			if (rnd(5) < 2) { std::reverse(S.begin(), S.end()); for (auto &x : S) x.rev ^= 1; }
			for (const Piece &x : S) {
				const uint32_t len = G.B[x.blk].cons_len;
				G.N.push_back(pga_topo_node_t{++nid, at, at + len, x.blk, G.B[x.blk].depth++, x.rev, 0});
				at += len + 1;
			}
		}
		P.n_nodes = (uint32_t)(G.N.size() - P.node_off);
		G.P.push_back(P);
	}
	// the member slots of every block in a random order
	std::vector<std::vector<uint32_t>> perm(G.B.size());
	for (size_t b = 0; b < G.B.size(); ++b) if (G.B[b].alive) { perm[b].resize(G.B[b].depth); for (uint32_t k = 0; k < G.B[b].depth; ++k) perm[b][k] = k; std::shuffle(perm[b].begin(), perm[b].end(), rng); }
	for (auto &n : G.N) n.member = perm[n.block][n.member];
	return G;
}

// ---------------------------------------------------------------- the direct construction
typedef std::array<uint32_t, 4> Edge;                                   // b1, s1, b2, s2
static Edge invert(const Edge &e) { return Edge{e[2], e[3] ^ 1u, e[0], e[1] ^ 1u}; }
static Edge conventional(const Edge &e) { return (e[0] < e[2] || (e[0] == e[2] && e[1] == 0)) ? e : invert(e); }
static uint64_t hash_words(std::initializer_list<uint64_t> w)
{
	std::vector<uint8_t> b;
	for (uint64_t x : w) for (int i = 0; i < 8; ++i) b.push_back((uint8_t)(x >> (8 * i)));
	return xxh64_bytes(b.data(), b.size(), 0);
}
static Out direct(const Graph &G, bool want_counts)
{
	Out D;
	std::map<std::array<uint32_t, 4>, uint32_t> count;                  // (b1, b2, s1, s2): the output order
	for (const auto &P : G.P) {
		const uint32_t n = P.n_nodes;
		for (uint32_t i = 0; i < (P.circular ? n : (n ? n - 1 : 0)); ++i) {
			const auto &x = G.N[P.node_off + i], &y = G.N[P.node_off + (i + 1) % n];
			const Edge c = conventional(Edge{x.block, (uint32_t)x.reverse, y.block, (uint32_t)y.reverse});
			++count[{c[0], c[2], c[1], c[3]}];
		}
	}
	for (const auto &kv : count) {
		const pga_topo_edge_t E{kv.first[0], kv.first[1], (int32_t)kv.first[2], (int32_t)kv.first[3], kv.second, 0};
		if (want_counts) D.counts.push_back(E);
		if (E.b1 != E.b2 && G.B[E.b1].depth == E.count && G.B[E.b2].depth == E.count) D.trans.push_back(E);
	}
	std::set<uint32_t> used;
	std::vector<int64_t> fate(G.N.size(), -1);                          // -1 kept, -2 dropped, else the new node
	for (size_t t = 0; t < D.trans.size(); ++t) {
		const pga_topo_edge_t &E = D.trans[t];
		if (used.count(E.b1) || used.count(E.b2)) continue;
		used.insert(E.b1); used.insert(E.b2);
		const auto &B1 = G.B[E.b1], &B2 = G.B[E.b2];
		Edge e{E.b1, (uint32_t)E.s1, E.b2, (uint32_t)E.s2};
		if (!(B1.cons_len > B2.cons_len || (B1.cons_len == B2.cons_len && B1.block_id < B2.block_id))) e = invert(e);
		const uint32_t a = e[0], b = e[2], rc = e[1] != e[3];
		pga_topo_round_t R{};
		R.anchor = a; R.other = b; R.anchor_rev = (int32_t)e[1]; R.other_rev = (int32_t)e[3]; R.transitive = (uint32_t)t;
		R.merge = e[1] == 0 ? pga_merge_edge_t{a, b, 0, (int32_t)rc} : pga_merge_edge_t{b, a, (int32_t)rc, 0};
		R.partner_off = D.partner.size();
		const size_t po = D.partner.size(), depth = G.B[a].depth;
		D.partner.resize(po + depth, TP_NONE); D.fresh.resize(po + depth); D.old_left.resize(po + depth); D.old_right.resize(po + depth);
		for (const auto &P : G.P) {
			const uint32_t n = P.n_nodes;
			for (uint32_t i = 0; i < (P.circular ? n : (n ? n - 1 : 0)); ++i) {
				const size_t ix = P.node_off + i, iy = P.node_off + (i + 1) % n;
				const auto &x = G.N[ix], &y = G.N[iy];
				const Edge here{x.block, (uint32_t)x.reverse, y.block, (uint32_t)y.reverse};
				if (here != e && here != invert(e)) continue;
				const bool x_anchor = x.block == a;
				const auto &A = x_anchor ? x : y, &L = x.block == R.merge.left ? x : y, &Rn = x.block == R.merge.left ? y : x;
				const size_t at = po + L.member;
				D.partner[at] = Rn.member;
				D.fresh[at] = pga_topo_node_t{hash_words({G.B[a].block_id, P.path_id, (uint64_t)A.reverse, x.pos0, y.pos1}), x.pos0, y.pos1, a, L.member, A.reverse, 0};
				D.old_left[at] = L.node_id; D.old_right[at] = Rn.node_id;
				fate[x_anchor ? ix : iy] = (int64_t)at; fate[x_anchor ? iy : ix] = -2;
			}
		}
		D.round.push_back(R);
	}
	if (D.round.empty()) return D;
	D.after.B = G.B;
	for (auto &b : D.after.B) if (!b.alive) { b.depth = 0; b.cons_len = 0; }
	for (const auto &R : D.round) { D.after.B[R.anchor].cons_len += G.B[R.other].cons_len; D.after.B[R.other] = pga_topo_block_t{G.B[R.other].block_id, 0, 0, 0, 0}; }
	for (const auto &P : G.P) {
		pga_topo_path_t Q{P.path_id, D.after.N.size(), 0, P.circular};
		for (uint64_t i = P.node_off; i < P.node_off + P.n_nodes; ++i) if (fate[i] != -2) D.after.N.push_back(fate[i] == -1 ? G.N[i] : D.fresh[fate[i]]);
		Q.n_nodes = (uint32_t)(D.after.N.size() - Q.node_off);
		D.after.P.push_back(Q);
	}
	return D;
}

// ---------------------------------------------------------------- the kernels, the sort and the scans between them as plain loops
static void scan(const uint32_t *in, uint32_t *out, size_t n) { uint32_t run = 0; for (size_t i = 0; i < n; ++i) { out[i] = run; run += in[i]; } }

static bool emulated(const Graph &G, uint32_t flags, unsigned grid, Out &O, uint32_t err[TP_ERRS])
{
	TpTables T;
	tp_validate((int64_t)G.B.size(), G.B.data(), (int64_t)G.P.size(), G.P.data(), (int64_t)G.N.size(), G.N.data(), 0, nullptr, flags, T);
	const uint64_t nn = G.N.size(), np = G.P.size(), nb = G.B.size();
	if (!nn || !np) return true;
	Exact<pga_topo_node_t> nodes(nn); Exact<pga_topo_path_t> paths(np);
	std::copy(G.N.begin(), G.N.end(), nodes.get()); std::copy(G.P.begin(), G.P.end(), paths.get());
	Exact<uint32_t> depth(nb), first(nb + 1), path_of(nn), slot_cnt(T.n_slots), blk_cnt(nb), e(TP_ERRS);
	std::copy(T.depth.begin(), T.depth.end(), depth.get()); std::copy(T.slot_first.begin(), T.slot_first.end(), first.get());
	e[0] = e[1] = TP_NONE;
	Exact<tp_u64> key(nn), skey(nn);
	Exact<uint32_t> head(nn + 1), hoff(nn + 1), rstart(nn + 1), keep(nn + 1), koff(nn + 1);
	TpDev V;
	memset(&V, 0, sizeof(V));
	V.n_nodes = nn; V.n_paths = np; V.n_blocks = nb; V.n_slots = T.n_slots;
	V.nodes = nodes.get(); V.paths = paths.get(); V.depth = depth.get(); V.slot_first = first.get(); V.path_of = path_of.get(); V.key = key.get();
	V.slot_cnt = slot_cnt.get(); V.blk_cnt = blk_cnt.get(); V.err = e.get();
	V.skey = skey.get(); V.head = head.get(); V.head_off = hoff.get(); V.run_start = rstart.get(); V.keep = keep.get(); V.keep_off = koff.get();
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_keys(V); });
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_check(V); });
	err[0] = e[0]; err[1] = e[1];
	if (e[0] != TP_NONE || e[1] != TP_NONE) return true;
	std::copy(key.get(), key.get() + nn, skey.get());
	std::sort(skey.get(), skey.get() + nn);
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_heads(V); });
	scan(head.get(), hoff.get(), nn + 1);
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_runs(V); });
	const uint32_t n_runs = hoff[nn];
	Exact<pga_topo_edge_t> counts((flags & PGA_TOPO_COUNTS) ? n_runs : 0);
	V.o_counts = counts.get();
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_keep(V); });
	scan(keep.get(), koff.get(), nn + 1);
	const uint32_t n_trans = koff[nn];
	Exact<pga_topo_edge_t> trans(n_trans);
	V.o_trans = trans.get();
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_compact(V); });
	O.trans.assign(trans.get(), trans.get() + n_trans); O.counts.assign(counts.get(), counts.get() + counts.n);
	TpRound R;
	tp_choose((int64_t)nb, G.B.data(), O.trans.data(), n_trans, 0, nullptr, R);
	O.round = R.round;
	if (R.round.empty()) return true;
	const uint64_t n_partner = R.n_partner, n_round = R.round.size();
	const uint32_t n_tiles = (uint32_t)((nn + TP_TILE - 1) / TP_TILE);
	Exact<uint32_t> choice(nb), partner(n_partner), cnt(nn + 1), repl(nn), tsum(n_tiles), toff(n_tiles + 1), poff(nn + 1);
	Exact<TpPick> pick(n_round); Exact<pga_topo_node_t> fresh(n_partner), onodes(nn - n_partner); Exact<uint64_t> left(n_partner), right(n_partner);
	Exact<pga_topo_path_t> opaths(np);
	std::copy(R.choice.begin(), R.choice.end(), choice.get()); std::copy(R.pick.begin(), R.pick.end(), pick.get());
	std::fill(partner.get(), partner.get() + n_partner, TP_NONE);
	V.choice = choice.get(); V.pick = pick.get(); V.o_partner = partner.get(); V.o_new = fresh.get(); V.o_left = left.get(); V.o_right = right.get();
	V.cnt = cnt.get(); V.repl = repl.get(); V.n_tiles = n_tiles; V.tile_sum = tsum.get(); V.tile_off = toff.get(); V.pos_off = poff.get();
	V.o_nodes = onodes.get(); V.o_paths = opaths.get();
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_pair(V); });
	emu_launch(dim3(std::min<unsigned>(grid, n_tiles)), dim3(TP_THREADS), [&] { k_topo_tile_sums(V); });
	emu_launch(dim3(1), dim3(TP_THREADS), [&] { k_topo_tile_scan(V); });
	CHECK(toff[n_tiles] == nn - n_partner);
	emu_launch(dim3(std::min<unsigned>(grid, n_tiles)), dim3(TP_THREADS), [&] { k_topo_splice(V); });
	emu_launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_paths(V); });
	O.partner.assign(partner.get(), partner.get() + n_partner); O.fresh.assign(fresh.get(), fresh.get() + n_partner);
	O.old_left.assign(left.get(), left.get() + n_partner); O.old_right.assign(right.get(), right.get() + n_partner);
	O.after.N.assign(onodes.get(), onodes.get() + onodes.n); O.after.P.assign(opaths.get(), opaths.get() + np);
	O.after.B.resize(nb);
	tp_blocks_after((int64_t)nb, G.B.data(), R, O.after.B.data());
	return true;
}

template <class T> static bool same(const std::vector<T> &a, const std::vector<T> &b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }

static bool run_graph(const Graph &G, unsigned grid)
{
	Out E, D = direct(G, true);
	uint32_t err[TP_ERRS];
	if (!emulated(G, PGA_TOPO_COUNTS, grid, E, err)) return false;
	if (G.N.empty()) return true;
	CHECK(err[0] == TP_NONE && err[1] == TP_NONE);
	CHECK(same(E.counts, D.counts)); CHECK(same(E.trans, D.trans)); CHECK(same(E.round, D.round)); CHECK(same(E.partner, D.partner));
	CHECK(same(E.fresh, D.fresh)); CHECK(same(E.old_left, D.old_left)); CHECK(same(E.old_right, D.old_right));
	CHECK(same(E.after.B, D.after.B)); CHECK(same(E.after.P, D.after.P)); CHECK(same(E.after.N, D.after.N));
	for (uint32_t q : D.partner) CHECK(q != TP_NONE);
	return true;
}

template <class F> static bool refused(F f) { try { f(); } catch (std::runtime_error &) { return true; } return false; }

int main()
{
	size_t n_rounds = 0, n_big = 0;
	for (g_graph = 0; g_graph < 18; ++g_graph) {
		const bool big = g_graph % 6 == 5;                                  // more than one tile of the splice, more than one workgroup
		const Graph G = generate(big ? 60 : 5, big ? 60 : 6, big);
		if (!run_graph(G, big ? 3 : 1 + rnd(3))) return 1;
		n_big += G.N.size() > (size_t)TP_TILE;
		n_rounds += !direct(G, false).round.empty();
	}
	if (n_rounds < 10 || n_big < 2) { fprintf(stderr, "topo_emu: the generator lost its cases (%zu rounds, %zu big graphs)\n", n_rounds, n_big); return 1; }
	// the hash against the general XXH64
	for (int i = 0; i < 50; ++i) {
		const uint64_t w[5] = {((uint64_t)rng() << 32) | rng(), rng(), (uint64_t)rnd(2), ((uint64_t)rng() << 20) | rng(), rng()};
		if (tp_node_id(w[0], w[1], w[2], w[3], w[4]) != hash_words({w[0], w[1], w[2], w[3], w[4]})) { fprintf(stderr, "topo_emu: tp_node_id differs from XXH64\n"); return 1; }
	}
	// what the device refuses: a slot named twice (and so another by none), found before any list is built
	g_graph = -2;
	{
		Graph G;
		do G = generate(4, 6, false); while (G.N.size() < 4);
		size_t i = 1;
		while (i < G.N.size() && !(G.N[i].block == G.N[0].block)) ++i;
		Out E; uint32_t err[TP_ERRS];
		if (i < G.N.size()) {
			G.N[i].member = G.N[0].member;
			if (!emulated(G, 0, 2, E, err) || err[TP_E_SLOT] == TP_NONE || err[TP_E_DEPTH] != TP_NONE) { fprintf(stderr, "topo_emu: a slot named twice was not found\n"); return 1; }
		}
		// and what the host refuses
		Graph H = generate(4, 6, false);
		while (H.N.size() < 3 || H.P.size() < 2) H = generate(4, 6, false);
		auto check = [&](Graph X) { TpTables T; tp_validate((int64_t)X.B.size(), X.B.data(), (int64_t)X.P.size(), X.P.data(), (int64_t)X.N.size(), X.N.data(), 0, nullptr, 0, T); };
		check(H);
		Graph X = H; X.N[0].block = (uint32_t)X.B.size();
		bool ok = refused([&] { check(X); });
		X = H; X.N[1].member = X.B[X.N[1].block].depth;
		ok = ok && refused([&] { check(X); });
		X = H; X.P[1].node_off += 1;
		ok = ok && refused([&] { check(X); });
		X = H; X.P[1].path_id = X.P[0].path_id;
		ok = ok && refused([&] { check(X); });
		X = H; X.B[X.N[0].block].alive = 0;
		ok = ok && refused([&] { check(X); });
		X = H; X.N.pop_back();
		ok = ok && refused([&] { check(X); });
		if (!ok) { fprintf(stderr, "topo_emu: malformed input was accepted\n"); return 1; }
	}
	printf("topo_emu OK (%zu graphs with a round, %zu of more than one tile)\n", n_rounds, n_big);
	return 0;
}
