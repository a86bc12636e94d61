// pga_join_idx.h without a device: validation and the tables, then every kernel of the header (and the copies of pga_assemble_idx.h it
// drives) under dev/emu/hip_emu.h, with every buffer allocated at exactly the size the kernels may touch (under the address sanitizer an
// access one entry out is an error), against a direct scalar construction: the alive blocks of all parts sorted by id, block after block,
// slot after slot, every list appended from where the member has it; the paths sorted by id, their nodes behind each other.
// Every file named on the command line is a named case of tests/join_gen.py (join_gen.dump: the parts of the call and host_join's
// expectation); it goes through the same kernels and is held against both the scalar construction and that expectation.
// The random instances are made here: 1 to 6 parts, some of them empty, flat graphs with dead entries, ids of the parts interleaved.  The
// three sorts are std::stable_sort where the device uses rocPRIM.
// Build and run (host only):  g++ -std=c++17 -g -O1 -DPGA_EMU -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined
//                             tests/emu/join_emu.cpp -o join_emu && ./join_emu [case files]
#include <cstdio>
#include <cstring>
#include <memory>
#include <numeric>
#include <random>
#include <set>
#include <string>
#include "../../dev/emu/hip_emu.h"
#include "../../pangraph_amd/csrc/pga_join_idx.h"

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
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "join_emu: %s:%d: %s (case %d)\n", __FILE__, __LINE__, #c, g_case); return false; } } while (0)
static int g_case = -1;
static const char CONS[] = "ACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCA";

struct Lists { std::vector<pga_sub_t> S; std::vector<pga_del_t> D; std::vector<pga_ins_t> I; };
struct Part {
	std::vector<pga_topo_block_t> GB; std::vector<pga_topo_path_t> GP; std::vector<pga_topo_node_t> GN;
	std::vector<pga_rc_block_t> RB; std::vector<pga_rc_member_t> M; Lists L; std::string seq; std::vector<pga_detach_member_t> who;
	pga_join_part_t view() const
	{
		return pga_join_part_t{(int64_t)GB.size(), GB.data(), (int64_t)GP.size(), GP.data(), (int64_t)GN.size(), GN.data(), RB.data(), M.data(), L.S.data(), L.D.data(), L.I.data(),
		                       seq.data(), seq.size(), who.data()};
	}
};
typedef std::vector<Part> Case;
struct Out {
	std::vector<pga_topo_block_t> GB; std::vector<pga_topo_path_t> GP; std::vector<pga_topo_node_t> GN;
	std::vector<pga_rc_member_t> M; Lists L; std::string seq;
	std::vector<pga_detach_member_t> who; std::vector<int32_t> part; std::vector<long long> origin; std::vector<uint32_t> bmap, pmap;
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

// part k of n: every id is x * n + k, so the parts never share one; ids of the parts interleave
static Part generate(uint32_t k, uint32_t n, uint32_t n_blocks, uint32_t max_depth, uint32_t long_list)
{
	Part G;
	static const char pool[] = "ACGTACGTTGCA";
	G.seq.assign(200 + rnd(300), 'A');
	for (char &c : G.seq) c = pool[rnd(12)];
	std::set<uint64_t> id_set;
	while (id_set.size() < n_blocks) id_set.insert(rnd(8) == 0 ? (uint64_t)rnd(4) * n + k : rnd(8) == 0 ? (~0ULL / n - rnd(4) - 1) * n + k : (((uint64_t)rng() << 32 | rng()) >> (rnd(3) ? 8 : 30)) / n * n + k);
	std::vector<uint64_t> ids(id_set.begin(), id_set.end());
	uint64_t nid = 1000;
	std::vector<std::pair<uint32_t, uint32_t>> slots;
	for (uint32_t b = 0; b < n_blocks; ++b) {
		const bool dead = rnd(7) == 0;
		const uint32_t d = dead ? 0 : rnd(max_depth + 1);
		G.GB.push_back(pga_topo_block_t{ids[b], dead ? 0u : 40 + rnd(60), d, dead ? 0 : 1, 0});
		G.RB.push_back(pga_rc_block_t{CONS + rnd(8), G.GB[b].cons_len, d});
		for (uint32_t m = 0; m < d; ++m) {
			G.M.push_back(add_lists(G.L, (uint32_t)G.seq.size(), long_list && G.M.size() % 7 == 3 ? long_list : 0));
			nid += 1 + rnd(5);
			G.who.push_back(pga_detach_member_t{nid * n + k, (int32_t)rnd(2), 0});
			slots.push_back({b, m});
		}
	}
	std::vector<uint32_t> first(n_blocks + 1, 0);
	for (uint32_t b = 0; b < n_blocks; ++b) first[b + 1] = first[b] + G.GB[b].depth;
	std::shuffle(slots.begin(), slots.end(), rng);
	uint64_t pid = rnd(5);
	for (size_t i = 0; i < slots.size() || G.GP.empty();) {
		const uint32_t cnt = (uint32_t)std::min<size_t>(rnd(6), slots.size() - i);
		pid += 1 + rnd(3);
		G.GP.push_back(pga_topo_path_t{pid * n + k, i, cnt, (int32_t)rnd(2)});
		for (uint32_t j = 0; j < cnt; ++j, ++i) {
			const pga_detach_member_t &W = G.who[first[slots[i].first] + slots[i].second];
			G.GN.push_back(pga_topo_node_t{W.node_id, rnd(1000), rnd(1000), slots[i].first, slots[i].second, W.reverse, 0});
		}
	}
	return G;
}
static Case generate_case(uint32_t n, uint32_t n_blocks, uint32_t max_depth, uint32_t long_list, bool with_empty)
{
	Case X;
	for (uint32_t k = 0; k < n; ++k) X.push_back(with_empty && rnd(3) == 0 ? Part() : generate(k, n, 1 + rnd(n_blocks), max_depth, long_list));
	return X;
}

// the scalar construction
static Out direct(const Case &X)
{
	Out D;
	struct Key { uint64_t id; uint32_t part, idx; };
	std::vector<Key> blocks, paths;
	std::vector<std::vector<uint64_t>> first(X.size()), off[3];
	std::vector<uint64_t> b_off(1, 0), p_off(1, 0);
	for (int q = 0; q < 3; ++q) off[q].resize(X.size());
	for (uint32_t k = 0; k < X.size(); ++k) {
		const Part &G = X[k];
		first[k].assign(G.GB.size() + 1, 0);
		for (size_t b = 0; b < G.GB.size(); ++b) { first[k][b + 1] = first[k][b] + G.GB[b].depth; if (G.GB[b].alive) blocks.push_back(Key{G.GB[b].block_id, k, (uint32_t)b}); }
		for (size_t p = 0; p < G.GP.size(); ++p) paths.push_back(Key{G.GP[p].path_id, k, (uint32_t)p});
		for (int q = 0; q < 3; ++q) off[q][k].assign(G.M.size() + 1, 0);
		for (size_t a = 0; a < G.M.size(); ++a) { off[0][k][a + 1] = off[0][k][a] + G.M[a].n_subs; off[1][k][a + 1] = off[1][k][a] + G.M[a].n_dels; off[2][k][a + 1] = off[2][k][a] + G.M[a].n_inss; }
		b_off.push_back(b_off.back() + G.GB.size()); p_off.push_back(p_off.back() + G.GP.size());
	}
	auto by_id = [](const Key &x, const Key &y) { return x.id < y.id; };
	std::stable_sort(blocks.begin(), blocks.end(), by_id); std::stable_sort(paths.begin(), paths.end(), by_id);
	D.bmap.assign(b_off.back(), TP_NONE); D.pmap.assign(p_off.back(), TP_NONE);
	for (uint32_t i = 0; i < blocks.size(); ++i) {
		const Part &G = X[blocks[i].part];
		const pga_topo_block_t &B = G.GB[blocks[i].idx];
		D.GB.push_back(pga_topo_block_t{B.block_id, B.cons_len, B.depth, 1, 0});
		D.bmap[b_off[blocks[i].part] + blocks[i].idx] = i;
		for (uint32_t s = 0; s < B.depth; ++s) {
			const uint64_t a = first[blocks[i].part][blocks[i].idx] + s;
			const pga_rc_member_t &M = G.M[a];
			D.M.push_back(M); D.who.push_back(pga_detach_member_t{G.who[a].node_id, G.who[a].reverse ? 1 : 0, 0}); D.part.push_back((int32_t)blocks[i].part); D.origin.push_back((long long)a);
			const uint64_t s0 = off[0][blocks[i].part][a], d0 = off[1][blocks[i].part][a], i0 = off[2][blocks[i].part][a];
			D.L.S.insert(D.L.S.end(), G.L.S.begin() + s0, G.L.S.begin() + s0 + M.n_subs); D.L.D.insert(D.L.D.end(), G.L.D.begin() + d0, G.L.D.begin() + d0 + M.n_dels);
			for (uint64_t j = i0; j < i0 + M.n_inss; ++j) { D.L.I.push_back(pga_ins_t{G.L.I[j].pos, G.L.I[j].len, D.seq.size()}); D.seq.append(G.seq, G.L.I[j].seq_off, G.L.I[j].len); }
		}
	}
	for (uint32_t i = 0; i < paths.size(); ++i) {
		const Part &G = X[paths[i].part];
		const pga_topo_path_t &P = G.GP[paths[i].idx];
		D.pmap[p_off[paths[i].part] + paths[i].idx] = i;
		D.GP.push_back(pga_topo_path_t{P.path_id, D.GN.size(), P.n_nodes, P.circular});
		for (uint64_t j = P.node_off; j < P.node_off + P.n_nodes; ++j) { pga_topo_node_t N = G.GN[j]; N.block = D.bmap[b_off[paths[i].part] + N.block]; N.pad = 0; D.GN.push_back(N); }
	}
	return D;
}

// ---------------------------------------------------------------- the kernels under the emulation
struct ScanBufs {
	Exact<jn_u64> tile_sum, tile_off, off; RmScan S;
	ScanBufs(uint64_t n, uint32_t n_q) : tile_sum((size_t)n_q * ((n + JN_TILE - 1) / JN_TILE)), tile_off((size_t)n_q * ((n + JN_TILE - 1) / JN_TILE + 1)), off((size_t)n_q * (n + 1)),
		S{n, (uint32_t)((n + JN_TILE - 1) / JN_TILE), n_q, tile_sum.get(), tile_off.get(), off.get()} {}
};
template <class Val> static void scan(const RmScan &S, const Val &val, unsigned grid)
{
	if (S.n_tiles) emu_launch(dim3(std::min<unsigned>(grid, S.n_tiles)), dim3(JN_THREADS), [&] { k_ts_sums<jn_u64, Val>(S, val); });
	emu_launch(dim3(1), dim3(JN_THREADS), [&] { k_ts_scan<jn_u64>(S); });
	if (S.n_tiles) emu_launch(dim3(std::min<unsigned>(grid, S.n_tiles)), dim3(JN_THREADS), [&] { k_ts_offsets<jn_u64, Val>(S, val); });
}
static void validate(const Case &X, uint32_t flags, JnTables &J)
{
	std::vector<pga_join_part_t> parts;
	for (const Part &G : X) parts.push_back(G.view());
	jn_validate((int32_t)parts.size(), parts.data(), flags, J);
}
template <class T, class F> static void place(Exact<T> &dst, const Case &X, const std::vector<jn_u64> &off, F field)
{
	for (size_t k = 0; k < X.size(); ++k) { const auto &v = field(X[k]); std::copy(v.begin(), v.begin() + (off[k + 1] - off[k]), dst.get() + off[k]); }
}
template <class K> static void sort_pairs(const K *kin, K *kout, const uint32_t *vin, uint32_t *vout, size_t n)
{
	std::vector<std::pair<K, uint32_t>> s;
	for (size_t i = 0; i < n; ++i) s.push_back({kin[i], vin ? vin[i] : 0u});
	std::stable_sort(s.begin(), s.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
	for (size_t i = 0; i < n; ++i) { kout[i] = s[i].first; if (vout) vout[i] = s[i].second; }
}

struct Errs { jn_u64 jn[JN_ERRS]; uint32_t hit[JN_ERRS]; as_u64 as[AS_ERRS]; };
// returns false on a CHECK; `refused` says whether the device checks stopped the call (nothing behind them has run then)
static bool emulated(const Case &X, unsigned grid, Out &O, Errs &E, bool &refused)
{
	JnTables J;
	validate(X, 0, J);
	const uint64_t P = X.size(), nb = J.blk_off[P], np = J.path_off[P], nn = J.node_off[P], nm = J.mem_off[P], na = J.alive_id.size();
	const uint64_t ns = J.list_off[0][P], nd = J.list_off[1][P], ni = J.ins_off[P], nl = J.let_off[P];
	refused = false;
	Exact<pga_topo_block_t> blocks(nb), oblocks(na); Exact<pga_topo_path_t> paths(np), opaths(np); Exact<pga_topo_node_t> nodes(nn), onodes(nn);
	Exact<pga_rc_member_t> members(nm), omembers(nm); Exact<pga_detach_member_t> who(nm), owho(nm);
	Exact<pga_sub_t> subs(ns); Exact<pga_del_t> dels(nd); Exact<pga_ins_t> inss(ni); Exact<char> letters(nl);
	Exact<jn_u64> blk_off(J.blk_off), path_off(J.path_off), node_off(J.node_off), mem_off(J.mem_off), ins_off(J.ins_off), let_off(J.let_off);
	Exact<jn_u64> aid(J.alive_id), sbid(na), pid(np), spid(np), nid(nn), snid(nn), err((size_t)JN_ERRS), aerr((size_t)AS_ERRS);
	Exact<uint32_t> first(J.first_member), ablock(J.alive_block), sblock(na), pidx(np), spath(np), osrc(na), bmap(nb), pmap(np), cnt(nm), hit((size_t)JN_ERRS);
	Exact<int32_t> opart(nm); Exact<long long> origin(nm); Exact<AsDesc> desc(nm);
	place(blocks, X, J.blk_off, [](const Part &G) -> const std::vector<pga_topo_block_t>& { return G.GB; }); place(paths, X, J.path_off, [](const Part &G) -> const std::vector<pga_topo_path_t>& { return G.GP; });
	place(nodes, X, J.node_off, [](const Part &G) -> const std::vector<pga_topo_node_t>& { return G.GN; }); place(members, X, J.mem_off, [](const Part &G) -> const std::vector<pga_rc_member_t>& { return G.M; });
	place(who, X, J.mem_off, [](const Part &G) -> const std::vector<pga_detach_member_t>& { return G.who; }); place(subs, X, J.list_off[0], [](const Part &G) -> const std::vector<pga_sub_t>& { return G.L.S; });
	place(dels, X, J.list_off[1], [](const Part &G) -> const std::vector<pga_del_t>& { return G.L.D; }); place(inss, X, J.ins_off, [](const Part &G) -> const std::vector<pga_ins_t>& { return G.L.I; });
	place(letters, X, J.let_off, [](const Part &G) -> const std::string& { return G.seq; });
	err.fill(0xff); aerr.fill(0xff); bmap.fill(0xff); pmap.fill(0xff);
	ScanBufs b_before(nm, 3), b_blocks(na, 1), b_paths(np, 1), b_out(nm, 3);
	JnDev V;
	memset(&V, 0, sizeof(V));
	V.n_parts = P; V.n_blocks = nb; V.n_paths = np; V.n_nodes = nn; V.n_members = nm; V.n_alive = na; V.n_inss = ni;
	V.blk_off = blk_off.get(); V.path_off = path_off.get(); V.node_off = node_off.get(); V.mem_off = mem_off.get(); V.ins_off = ins_off.get(); V.let_off = let_off.get();
	V.blocks = blocks.get(); V.paths = paths.get(); V.nodes = nodes.get(); V.first_member = first.get(); V.who = who.get(); V.inss = inss.get();
	V.path_id = pid.get(); V.node_id = nid.get(); V.path_idx = pidx.get();
	V.s_block_id = sbid.get(); V.s_block = sblock.get(); V.s_path_id = spid.get(); V.s_path = spath.get(); V.s_node_id = snid.get();
	V.o_blocks = oblocks.get(); V.o_src = osrc.get(); V.o_paths = opaths.get(); V.o_nodes = onodes.get(); V.block_map = bmap.get(); V.path_map = pmap.get();
	V.o_who = owho.get(); V.o_part = opart.get(); V.slot_cnt = cnt.get(); V.err = err.get(); V.hit = hit.get();
	V.A.n_out_members = nm; V.A.ins_seq_len = nl; V.A.p_ins_seq_len = 0;
	V.A.members = members.get(); V.A.subs = subs.get(); V.A.dels = dels.get(); V.A.inss = inss.get(); V.A.letters = letters.get();
	V.A.desc = desc.get(); V.A.o_members = omembers.get(); V.A.origin = origin.get(); V.A.err = aerr.get();
	V.scan[JN_SCAN_BEFORE] = b_before.S; V.scan[JN_SCAN_BLOCKS] = b_blocks.S; V.scan[JN_SCAN_PATHS] = b_paths.S; V.A.scan[AS_SCAN_OUT] = b_out.S;
	emu_launch(dim3(grid), dim3(JN_THREADS), [&] { k_join_keys(V); });
	emu_launch(dim3(grid), dim3(JN_THREADS), [&] { k_join_ins(V); });
	scan(V.scan[JN_SCAN_BEFORE], AsBeforeValue{V.A}, grid);
	sort_pairs(aid.get(), sbid.get(), ablock.get(), sblock.get(), na); sort_pairs(pid.get(), spid.get(), pidx.get(), spath.get(), np);
	sort_pairs<jn_u64>(nid.get(), snid.get(), nullptr, nullptr, nn);
	emu_launch(dim3(grid), dim3(JN_THREADS), [&] { k_join_rank(V); });
	scan(V.scan[JN_SCAN_BLOCKS], JnDepthValue{V}, grid);
	scan(V.scan[JN_SCAN_PATHS], JnPathValue{V}, grid);
	emu_launch(dim3(grid), dim3(JN_THREADS), [&] { k_join_desc(V); });
	emu_launch(dim3(grid), dim3(JN_THREADS), [&] { k_join_nodes(V); });
	emu_launch(dim3(grid), dim3(JN_THREADS), [&] { k_join_check(V); });
	scan(V.A.scan[AS_SCAN_OUT], AsOutValue{V.A}, grid);
	auto read_errs = [&]() {
		std::copy(err.get(), err.get() + JN_ERRS, E.jn); std::copy(hit.get(), hit.get() + JN_ERRS, E.hit); std::copy(aerr.get(), aerr.get() + AS_ERRS, E.as);
		for (uint32_t x : E.hit) if (x) return true;                          // (hit[], not err[]: an id may itself be all-ones)
		for (as_u64 x : E.as) if (x != AS_NONE) return true;
		return false;
	};
	if (read_errs()) { refused = true; return true; }
	CHECK(b_blocks.off[na] == nm && b_paths.off[np] == nn);
	CHECK(b_out.off[0 * (nm + 1) + nm] == ns && b_out.off[1 * (nm + 1) + nm] == nd && b_out.off[2 * (nm + 1) + nm] == ni);
	Exact<pga_sub_t> osubs(ns); Exact<pga_del_t> odels(nd); Exact<pga_ins_t> oinss(ni);
	V.A.o_subs = osubs.get(); V.A.o_dels = odels.get(); V.A.o_inss = oinss.get();
	if (ns) emu_launch(dim3(grid), dim3(AS_THREADS), [&] { k_assemble_copy<RM_LIST_SUB>(V.A); });
	if (nd) emu_launch(dim3(grid), dim3(AS_THREADS), [&] { k_assemble_copy<RM_LIST_DEL>(V.A); });
	if (ni) emu_launch(dim3(grid), dim3(AS_THREADS), [&] { k_assemble_copy<RM_LIST_INS>(V.A); });
	ScanBufs b_let(ni, 1);
	V.A.scan[AS_SCAN_LETTERS] = b_let.S;
	scan(V.A.scan[AS_SCAN_LETTERS], AsLetterValue{V.A}, grid);
	if (read_errs()) { refused = true; return true; }
	const uint64_t nl_out = b_let.off[ni];
	Exact<char> oseq(nl_out);
	V.A.o_ins_seq = oseq.get();
	if (nl_out) emu_launch(dim3(grid), dim3(AS_THREADS), [&] { k_assemble_letters(V.A); });
	if (ni) emu_launch(dim3(grid), dim3(AS_THREADS), [&] { k_assemble_seq_off(V.A); });
	O.GB.assign(oblocks.get(), oblocks.get() + na); O.GP.assign(opaths.get(), opaths.get() + np); O.GN.assign(onodes.get(), onodes.get() + nn);
	O.M.assign(omembers.get(), omembers.get() + nm); O.L.S.assign(osubs.get(), osubs.get() + ns); O.L.D.assign(odels.get(), odels.get() + nd); O.L.I.assign(oinss.get(), oinss.get() + ni);
	O.who.assign(owho.get(), owho.get() + nm); O.part.assign(opart.get(), opart.get() + nm); O.origin.assign(origin.get(), origin.get() + nm);
	O.bmap.assign(bmap.get(), bmap.get() + nb); O.pmap.assign(pmap.get(), pmap.get() + np);
	if (nl_out) O.seq.assign(oseq.get(), nl_out);
	return true;
}

template <class T> static bool same(const std::vector<T> &a, const std::vector<T> &b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }
static bool equal(const Out &E, const Out &D, bool with_who)
{
	CHECK(same(E.GB, D.GB)); CHECK(same(E.GP, D.GP)); CHECK(same(E.GN, D.GN)); CHECK(same(E.M, D.M)); CHECK(same(E.L.S, D.L.S)); CHECK(same(E.L.D, D.L.D)); CHECK(same(E.L.I, D.L.I));
	CHECK(E.seq == D.seq); CHECK(same(E.part, D.part)); CHECK(same(E.origin, D.origin)); CHECK(same(E.bmap, D.bmap)); CHECK(same(E.pmap, D.pmap));
	if (with_who) CHECK(same(E.who, D.who));
	return true;
}
static bool run_case(const Case &X, unsigned grid)
{
	Out E, D = direct(X);
	Errs err; bool refused;
	if (!emulated(X, grid, E, err, refused)) return false;
	CHECK(!refused);
	if (!equal(E, D, true)) return false;
	for (size_t i = 1; i < E.GB.size(); ++i) CHECK(E.GB[i - 1].block_id < E.GB[i].block_id);
	for (size_t i = 1; i < E.GP.size(); ++i) CHECK(E.GP[i - 1].path_id < E.GP[i].path_id);
	return true;
}

// ---------------------------------------------------------------- a named case of tests/join_gen.py from its file (join_gen.dump)
struct Reader {
	std::string buf; size_t at = 0; bool ok = true;
	uint64_t word() { uint64_t n = 0; if (at + 8 > buf.size()) { ok = false; return 0; } memcpy(&n, buf.data() + at, 8); at += 8; return n; }
	template <class T> std::vector<T> take()
	{
		std::vector<T> v;
		const uint64_t n = word();
		if (!ok || n % sizeof(T) || at + n > buf.size()) { ok = false; return v; }
		v.resize(n / sizeof(T));
		if (n) memcpy(v.data(), buf.data() + at, n);
		at += n;
		return v;
	}
	std::string text() { const std::vector<char> v = take<char>(); return std::string(v.begin(), v.end()); }
	std::vector<pga_rc_block_t> blocks() { std::vector<pga_rc_block_t> B; const std::vector<uint32_t> v = take<uint32_t>(); for (size_t i = 0; i + 1 < v.size(); i += 2) B.push_back(pga_rc_block_t{CONS, v[i], v[i + 1]}); return B; }
};
static bool load(const char *file, Case &X, Out &E)
{
	Reader R;
	FILE *f = fopen(file, "rb");
	if (!f) return false;
	char tmp[1 << 16]; size_t n;
	while ((n = fread(tmp, 1, sizeof(tmp), f)) > 0) R.buf.append(tmp, n);
	fclose(f);
	const uint64_t n_parts = R.word();
	if (!R.ok || n_parts > 100000) return false;
	X.resize(n_parts);
	for (Part &G : X) {
		G.GB = R.take<pga_topo_block_t>(); G.GP = R.take<pga_topo_path_t>(); G.GN = R.take<pga_topo_node_t>(); G.RB = R.blocks(); G.M = R.take<pga_rc_member_t>();
		G.L.S = R.take<pga_sub_t>(); G.L.D = R.take<pga_del_t>(); G.L.I = R.take<pga_ins_t>(); G.seq = R.text(); G.who = R.take<pga_detach_member_t>();
	}
	E.GB = R.take<pga_topo_block_t>(); E.GP = R.take<pga_topo_path_t>(); E.GN = R.take<pga_topo_node_t>(); E.M = R.take<pga_rc_member_t>(); E.L.S = R.take<pga_sub_t>(); E.L.D = R.take<pga_del_t>();
	E.L.I = R.take<pga_ins_t>(); E.seq = R.text(); E.part = R.take<int32_t>(); E.origin = R.take<long long>(); E.bmap = R.take<uint32_t>(); E.pmap = R.take<uint32_t>();
	return R.ok && R.at == R.buf.size();
}
// the kernels on a named case, against the scalar construction AND against what the Python side expects (host_join)
static bool run_file(const char *file)
{
	Case X; Out W;
	if (!load(file, X, W)) { fprintf(stderr, "join_emu: cannot read %s\n", file); return false; }
	Out E, D = direct(X);
	Errs err; bool refused;
	if (!emulated(X, 2, E, err, refused)) return false;
	CHECK(!refused);
	return equal(E, D, true) && equal(E, W, false);
}

template <class F> static bool refused_by_host(F f) { try { f(); } catch (std::runtime_error &) { return true; } return false; }

int main(int argc, char **argv)
{
	for (int a = 1; a < argc; ++a) { g_case = 1000 + a; if (!run_file(argv[a])) { fprintf(stderr, "join_emu: %s\n", argv[a]); return 1; } }
	size_t n_big = 0, n_long = 0, n_empty = 0, n_dead = 0, n_parts = 0;
	for (g_case = 0; g_case < 12; ++g_case) {
		const int kind = g_case;                          // 3: more than one tile of members; 4: lists of several tiles; 5: one part; 6: many small parts
		const Case X = kind == 3 ? generate_case(3, 1200, 4, 0, false) : kind == 4 ? generate_case(2, 8, 4, 2 * JN_TILE + 5, false) : kind == 5 ? generate_case(1, 12, 4, 0, false)
		               : kind == 6 ? generate_case(40, 2, 2, 0, true) : generate_case(1 + rnd(6), 12, 5, 0, true);
		if (!run_case(X, 1 + rnd(3))) return 1;
		const Out D = direct(X);
		n_big += D.M.size() > (size_t)JN_TILE; n_long += D.L.S.size() > (size_t)2 * JN_TILE; n_parts += X.size();
		for (const Part &G : X) { n_empty += G.GB.empty(); for (const auto &B : G.GB) n_dead += !B.alive; }
	}
	if (n_big < 1 || n_long < 1 || n_empty < 3 || n_dead < 3) { fprintf(stderr, "join_emu: the generator lost its cases (%zu big, %zu long lists, %zu empty parts, %zu dead entries)\n", n_big, n_long, n_empty, n_dead); return 1; }
	// ---- what is refused: on the host, and by the kernels before an index is derived
	g_case = -2;
	Case H;
	auto fits = [](const Case &Y) {
		for (const Part &G : Y) {
			bool letters = false;
			for (const auto &I : G.L.I) letters = letters || (I.len && I.seq_off + I.len > 3);
			size_t alive = 0;
			for (const auto &B : G.GB) alive += B.alive != 0;
			if (!letters || G.GN.size() < 3 || G.GP.size() < 2 || alive < 2) return false;
		}
		return Y[1].seq.size() > 50;
	};
	do H = generate_case(3, 10, 4, 0, false); while (!fits(H));
	auto host = [&](const Case &X, uint32_t flags) { JnTables J; validate(X, flags, J); };
	host(H, 0); host(H, 1);
	bool ok = true;
	auto alive_at = [](const Part &G, int which) { size_t b = 0; for (;; ++b) if (G.GB[b].alive && which-- == 0) return b; };
	Case X = H;                                                        ok = ok && refused_by_host([&] { host(X, 2); });
	X.clear();                                                         ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; std::swap(X[1].GB[alive_at(X[1], 0)].block_id, X[1].GB[alive_at(X[1], 1)].block_id);   ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; std::swap(X[2].GP[0].path_id, X[2].GP[1].path_id);          ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X[1].GN[0].block = (uint32_t)X[1].GB.size();                ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X[1].GB[X[1].GN[0].block].alive = 0;                        ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X[0].GN[0].member = X[0].GB[X[0].GN[0].block].depth;        ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X[2].GP[1].node_off += 1;                                   ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X[1].RB[alive_at(X[1], 0)].n_members += 1;                  ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X[1].RB[alive_at(X[1], 0)].cons_len += 1;                   ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X[1].M[0].n_subs = 0xffffffffu; { std::vector<pga_join_part_t> parts; for (const Part &G : X) parts.push_back(G.view()); parts[1].subs = nullptr; parts[1].members = nullptr;
	         ok = ok && refused_by_host([&] { JnTables J; jn_validate(3, parts.data(), 0, J); }); }
	if (!ok) { fprintf(stderr, "join_emu: malformed input was accepted by the host\n"); return 1; }
	auto device = [&](const Case &Y, int which, jn_u64 what) {
		Out E; Errs err; bool refused;
		if (!emulated(Y, 1, E, err, refused)) return false;
		return refused && err.hit[which] && err.jn[which] == what && E.M.empty() && E.L.S.empty();
	};
	{ X = H; const uint64_t id = X[0].GB[alive_at(X[0], 1)].block_id; X[2].GB[alive_at(X[2], 0)].block_id = 0; X[0].GB[alive_at(X[0], 0)].block_id = 0; (void)id; ok = ok && device(X, JN_E_BLOCK, 0); }
	{ X = H; const uint64_t id = std::max(X[1].GP.back().path_id, X[2].GP.back().path_id) + 1; X[1].GP.back().path_id = id; X[2].GP.back().path_id = id; ok = ok && device(X, JN_E_PATH, id); }
	{ X = H; X[2].GN[1].node_id = X[0].GN[2].node_id; ok = ok && device(X, JN_E_NODE, X[0].GN[2].node_id); }
	{ X = H; X[1].GN[1].node_id = X[1].GN[0].node_id; ok = ok && device(X, JN_E_NODE, X[1].GN[0].node_id); }
	{ X = H;                                                           // (the id all-ones in two parts: err[] alone would read as "none")
	  for (int k = 1; k < 3; ++k) { pga_topo_block_t &B = X[k].GB.back(); B.block_id = ~0ULL; if (!B.alive) { B.alive = 1; B.cons_len = X[k].RB.back().cons_len = 5; } }
	  ok = ok && device(X, JN_E_BLOCK, ~0ULL); }
	{ X = H; size_t i = 1; while (i < X[1].GN.size() && X[1].GN[i].block != X[1].GN[0].block) ++i;
	  if (i < X[1].GN.size()) { const uint32_t lo = std::min(X[1].GN[0].member, X[1].GN[i].member); const bool first_takes = X[1].GN[0].member > X[1].GN[i].member;
	    (first_takes ? X[1].GN[0] : X[1].GN[i]).member = lo; uint64_t slot = 0; for (uint32_t b = 0; b < X[1].GN[0].block; ++b) slot += X[1].GB[b].depth;
	    JnTables J; validate(H, 0, J); ok = ok && device(X, JN_E_SLOT, (J.mem_off[1] + slot + lo) << 1 | 1u); } }
	{ X = H; X[1].seq.resize(3); Out E; Errs err; bool refused; ok = ok && emulated(X, 1, E, err, refused) && refused && err.hit[JN_E_SEQ] && E.M.empty(); }
	{ X = H; size_t j = 0; while (!X[0].L.I[j].len) ++j; X[0].L.I[j].seq_off = X[0].seq.size() - X[0].L.I[j].len + 1;                  // (inside the concatenated letters, beyond its own part's)
	  JnTables J; validate(H, 0, J); ok = ok && device(X, JN_E_SEQ, J.ins_off[0] + j); }
	{ X = H; size_t j = 0; while (!X[2].L.I[j].len) ++j; X[2].L.I[j].seq_off = ~0ULL - 2; JnTables J; validate(H, 0, J); ok = ok && device(X, JN_E_SEQ, J.ins_off[2] + j); }   // (seq_off + len wraps)
	if (!ok) { fprintf(stderr, "join_emu: malformed input passed the kernels' checks\n"); return 1; }
	printf("join_emu OK (%d named cases, %zu random parts, %zu graphs of more than one tile, %zu with long lists, %zu empty parts, %zu dead entries)\n", argc - 1, n_parts, n_big, n_long, n_empty, n_dead);
	return 0;
}
