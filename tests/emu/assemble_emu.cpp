// pga_assemble_idx.h without a device: validation and the tables, then every kernel of the header under dev/emu/hip_emu.h, with every buffer
// allocated at exactly the size the kernels may touch (under the address sanitizer an access one entry out is an error), against a direct
// scalar construction: block after block of the graph after, slot after slot, every list appended from where the slot's member has it.
// The instances are made here: blocks with members, some of them cut into intervals, intervals paired into promises, slices that keep some
// members, a block table after in id order with the member slots in a random order (what the node ids would give).
// Build and run (host only):  g++ -std=c++17 -g -O1 -DPGA_EMU -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined
//                             tests/emu/assemble_emu.cpp -o assemble_emu && ./assemble_emu
#include <cstdio>
#include <cstring>
#include <memory>
#include <numeric>
#include <random>
#include <set>
#include <string>
#include "../../dev/emu/hip_emu.h"
#include "../../pangraph_amd/csrc/pga_assemble_idx.h"

using namespace pga;

template <class T> struct Exact {                                       // n entries, not one more
	std::unique_ptr<T[]> p; size_t n;
	explicit Exact(size_t n_) : p(n_ ? new T[n_]() : nullptr), n(n_) {}
	template <class V> explicit Exact(const V &v) : Exact(v.size()) { std::copy(v.begin(), v.end(), p.get()); }
	T *get() { return p.get(); }
	T &operator[](size_t i) { return p[i]; }
};

static std::mt19937 rng(20261020);
static uint32_t rnd(uint32_t n) { return n ? (uint32_t)(rng() % n) : 0u; }
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "assemble_emu: %s:%d: %s (case %d)\n", __FILE__, __LINE__, #c, g_case); return false; } } while (0)
static int g_case = -1;
static const char CONS[] = "ACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCAACGTTGCA";

struct Lists { std::vector<pga_sub_t> S; std::vector<pga_del_t> D; std::vector<pga_ins_t> I; };
struct Case {
	std::vector<pga_rc_block_t> RB; std::vector<pga_rc_member_t> M; Lists B; std::string seq, p_seq;
	std::vector<pga_apply_cut_t> cut; std::vector<pga_plan_interval_t> iv; std::vector<pga_plan_promise_t> pr;
	std::vector<pga_slice_res_t> sl; std::vector<pga_slice_member_t> sm; Lists SL;
	std::vector<pga_mapvar_res_t> res; Lists P;
	std::vector<pga_topo_block_t> ab; std::vector<pga_topo_node_t> an; std::vector<pga_apply_block_t> ae; std::vector<uint64_t> msrc; std::vector<uint32_t> bmap;
	pga_slice_out_t slice() const { return pga_slice_out_t{(pga_slice_res_t*)sl.data(), (pga_slice_member_t*)sm.data(), nullptr, nullptr, (pga_sub_t*)SL.S.data(), (pga_del_t*)SL.D.data(), (pga_ins_t*)SL.I.data()}; }
	pga_apply_out_t applied() const
	{
		pga_apply_out_t a;
		memset(&a, 0, sizeof(a));
		a.n_new_nodes = (int64_t)sm.size(); a.n_new_blocks = (int64_t)ae.size(); a.n_blocks = (int64_t)ab.size(); a.n_nodes = (int64_t)an.size();
		a.new_blocks = (pga_apply_block_t*)ae.data(); a.member_src = (uint64_t*)msrc.data(); a.block_map = (uint32_t*)bmap.data(); a.nodes = (pga_topo_node_t*)an.data(); a.blocks = (pga_topo_block_t*)ab.data();
		return a;
	}
};
struct Out {
	std::vector<pga_rc_block_t> B; std::vector<pga_rc_member_t> M; Lists L; std::string seq;
	std::vector<pga_detach_member_t> who; std::vector<long long> origin;
};

static const uint32_t LENGTHS[] = {0, 0, 0, 1, 2, 63, 64, 65, 130};
// the lists of one member appended to L; the letters of an insertion lie anywhere in a buffer of seq_len letters
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

static Case generate(uint32_t n_blocks, uint32_t max_depth, uint32_t cut_one_in, uint32_t long_list)
{
	Case G;
	static const char pool[] = "ACGTACGTTGCA";
	G.seq.assign(5000 + rnd(100), 'A'); G.p_seq.assign(150 + rnd(100), 'A');
	for (char &c : G.seq) c = pool[rnd(12)];
	for (char &c : G.p_seq) c = pool[rnd(12)];
	std::set<uint64_t> id_set;
	while (id_set.size() < 4 * (size_t)n_blocks + 8) id_set.insert(((uint64_t)rng() << 32 | rng()) | (rnd(3) ? 0 : 1ULL << 63));
	std::vector<uint64_t> ids(id_set.begin(), id_set.end());
	std::shuffle(ids.begin(), ids.end(), rng);
	size_t next_id = 0;
	std::vector<uint64_t> before_id(n_blocks);
	std::vector<uint64_t> first(n_blocks + 1, 0);
	for (uint32_t b = 0; b < n_blocks; ++b) {
		const bool dead = rnd(7) == 0;
		const uint32_t n = dead ? 0 : rnd(max_depth + 1);
		G.RB.push_back(pga_rc_block_t{CONS + rnd(8), 40 + rnd(60), n});
		before_id[b] = ids[next_id++];
		first[b + 1] = first[b] + n;
		for (uint32_t m = 0; m < n; ++m) G.M.push_back(add_lists(G.B, (uint32_t)G.seq.size(), long_list && G.M.size() % 7 == 3 ? long_list : 0));
	}
	// ---- the cut: some blocks, 1 .. 3 intervals each; pairs of intervals become promises
	std::vector<int> is_cut(n_blocks, 0);
	for (uint32_t b = 0; b < n_blocks; ++b) if (rnd(cut_one_in) == 0) {
		is_cut[b] = 1;
		const uint32_t n_iv = 1 + rnd(3), step = G.RB[b].cons_len / n_iv;
		G.cut.push_back(pga_apply_cut_t{b, n_iv, G.iv.size()});
		for (uint32_t j = 0; j < n_iv; ++j) G.iv.push_back(pga_plan_interval_t{ids[next_id++], -1, j * step + (j ? rnd(3) : 0), (j + 1) * step, 0, 0, 0, 0, 0, 0});
	}
	std::vector<uint32_t> order(G.iv.size());
	std::iota(order.begin(), order.end(), 0u);
	std::shuffle(order.begin(), order.end(), rng);
	const size_t n_pr = order.size() / 3;
	for (size_t p = 0; p < n_pr; ++p) {
		const uint32_t a = order[2 * p], q = order[2 * p + 1];
		G.iv[a].aligned = G.iv[q].aligned = 1; G.iv[a].is_anchor = 1; G.iv[q].new_block_id = G.iv[a].new_block_id;
		G.pr.push_back(pga_plan_promise_t{G.iv[a].new_block_id, (int64_t)p, a, q, 0, 0, 0, 0, 0});
	}
	std::sort(G.pr.begin(), G.pr.end(), [](const pga_plan_promise_t &x, const pga_plan_promise_t &y) { return x.new_block_id < y.new_block_id; });
	// ---- the slices: every interval keeps some members of its block
	for (const pga_apply_cut_t &C : G.cut) for (uint32_t j = 0; j < C.n_intervals; ++j) {
		pga_slice_res_t R{G.sm.size(), 0, 0};
		for (uint32_t m = 0; m < G.RB[C.block].n_members; ++m) {
			if (rnd(4) == 0) { ++R.n_dropped; continue; }
			pga_slice_member_t X;
			memset(&X, 0, sizeof(X));
			X.member = m; X.sub_off = G.SL.S.size(); X.del_off = G.SL.D.size(); X.ins_off = G.SL.I.size();
			X.counts = add_lists(G.SL, (uint32_t)G.seq.size(), 0);
			G.sm.push_back(X); ++R.n_kept;
		}
		G.sl.push_back(R);
	}
	for (const pga_plan_promise_t &P : G.pr) for (uint32_t j = 0; j < G.sl[P.append_interval].n_kept; ++j) {
		pga_mapvar_res_t R;
		memset(&R, 0, sizeof(R));
		R.sub_off = G.P.S.size(); R.del_off = G.P.D.size(); R.ins_off = G.P.I.size();
		const pga_rc_member_t X = add_lists(G.P, (uint32_t)G.p_seq.size(), long_list && G.res.size() % 5 == 1 ? long_list : 0);
		R.n_subs = X.n_subs; R.n_dels = X.n_dels; R.n_inss = X.n_inss;
		G.res.push_back(R);
	}
	// ---- the graph after: survivors and new blocks by ascending id; the member slots of a new block in a random order
	struct After { uint64_t id; int kind; uint32_t old, ia, ib; };
	std::vector<After> after;
	for (uint32_t b = 0; b < n_blocks; ++b) if (!is_cut[b] && (G.RB[b].n_members || rnd(2))) after.push_back(After{before_id[b], -1, b, 0, 0});
	for (uint32_t s = 0; s < G.iv.size(); ++s) if (!G.iv[s].aligned) after.push_back(After{G.iv[s].new_block_id, 0, 0, s, 0});
	for (const pga_plan_promise_t &P : G.pr) after.push_back(After{P.new_block_id, 1, 0, (uint32_t)P.anchor_interval, (uint32_t)P.append_interval});
	std::sort(after.begin(), after.end(), [](const After &x, const After &y) { return x.id < y.id; });
	G.bmap.assign(n_blocks, TP_NONE);
	uint64_t nid = 1000;
	for (uint32_t i = 0; i < after.size(); ++i) {
		const After &X = after[i];
		uint32_t depth;
		if (X.kind < 0) { G.bmap[X.old] = i; depth = G.RB[X.old].n_members; G.ab.push_back(pga_topo_block_t{X.id, G.RB[X.old].cons_len, depth, 1, 0}); }
		else {
			std::vector<uint64_t> ks;
			for (uint32_t j = 0; j < G.sl[X.ia].n_kept; ++j) ks.push_back(G.sl[X.ia].member_off + j);
			for (uint32_t j = 0; X.kind && j < G.sl[X.ib].n_kept; ++j) ks.push_back(G.sl[X.ib].member_off + j);
			std::shuffle(ks.begin(), ks.end(), rng);
			depth = (uint32_t)ks.size();
			G.ae.push_back(pga_apply_block_t{i, X.kind, X.ia, X.kind ? X.ib : 0, G.msrc.size()});
			G.msrc.insert(G.msrc.end(), ks.begin(), ks.end());
			G.ab.push_back(pga_topo_block_t{X.id, G.iv[X.ia].end - G.iv[X.ia].start, depth, 1, 0});
		}
		for (uint32_t s = 0; s < depth; ++s) { nid += 1 + rnd(5); G.an.push_back(pga_topo_node_t{nid, 0, 0, i, s, (int32_t)rnd(2), 0}); }
	}
	std::shuffle(G.an.begin(), G.an.end(), rng);
	if (!G.SL.I.empty()) { G.SL.I[0].len = 5000; G.SL.I[0].seq_off = G.seq.size() - 5000; }     // (a kept slice member's: always in the default output)
	return G;
}
// one more surviving block, behind all others, that brings the members after to exactly `target`
static bool pad_to(Case &G, uint64_t target)
{
	uint64_t cur = 0, top = 0;
	for (const auto &B : G.ab) { cur += B.depth; top = std::max<uint64_t>(top, B.block_id); }
	if (cur >= target || top == ~0ULL) return false;
	const uint32_t n = (uint32_t)(target - cur), i = (uint32_t)G.ab.size();
	G.RB.push_back(pga_rc_block_t{CONS, 50, n}); G.bmap.push_back(i); G.ab.push_back(pga_topo_block_t{top + 1, 50, n, 1, 0});
	for (uint32_t s = 0; s < n; ++s) { G.M.push_back(s % 5 ? pga_rc_member_t{0, 0, 0} : add_lists(G.B, (uint32_t)G.seq.size(), 0)); G.an.push_back(pga_topo_node_t{1ULL << 40 | s, 0, 0, i, s, (int32_t)(s & 1), 0}); }
	return true;
}

// ---------------------------------------------------------------- the direct construction
static void append_lists(Out &D, const Lists &L, const std::string &seq, uint64_t s, uint64_t d, uint64_t x, pga_rc_member_t n)
{
	D.M.push_back(n);
	D.L.S.insert(D.L.S.end(), L.S.begin() + s, L.S.begin() + s + n.n_subs); D.L.D.insert(D.L.D.end(), L.D.begin() + d, L.D.begin() + d + n.n_dels);
	for (uint64_t k = x; k < x + n.n_inss; ++k) { pga_ins_t I = L.I[k]; I.seq_off = D.seq.size(); D.seq += seq.substr(L.I[k].seq_off, I.len); D.L.I.push_back(I); }
}
static Out direct(const Case &G, uint32_t flags)
{
	Out D;
	std::vector<uint64_t> first(G.RB.size() + 1, 0), off[3];
	for (size_t b = 0; b < G.RB.size(); ++b) first[b + 1] = first[b] + G.RB[b].n_members;
	for (auto &o : off) o.assign(G.M.size() + 1, 0);
	for (size_t m = 0; m < G.M.size(); ++m) { off[0][m + 1] = off[0][m] + G.M[m].n_subs; off[1][m + 1] = off[1][m] + G.M[m].n_dels; off[2][m + 1] = off[2][m] + G.M[m].n_inss; }
	std::vector<uint64_t> first_res(G.pr.size() + 1, 0);
	for (size_t p = 0; p < G.pr.size(); ++p) first_res[p + 1] = first_res[p] + G.sl[G.pr[p].append_interval].n_kept;
	std::vector<int> kind(G.ab.size(), -1); std::vector<size_t> entry(G.ab.size(), 0);
	for (size_t b = 0; b < G.bmap.size(); ++b) if (G.bmap[b] != TP_NONE) entry[G.bmap[b]] = b;
	for (size_t e = 0; e < G.ae.size(); ++e) { kind[G.ae[e].block] = G.ae[e].kind; entry[G.ae[e].block] = e; }
	std::vector<std::vector<const pga_topo_node_t*>> slot(G.ab.size());
	for (size_t i = 0; i < G.ab.size(); ++i) slot[i].resize(G.ab[i].depth);
	for (const auto &n : G.an) slot[n.block][n.member] = &n;
	for (size_t i = 0; i < G.ab.size(); ++i) {
		if ((flags & PGA_ASSEMBLE_MERGED_ONLY) && kind[i] != 1) continue;
		if (kind[i] < 0) {
			const size_t b = entry[i];
			D.B.push_back(G.RB[b]);
			for (uint64_t m = first[b]; m < first[b + 1]; ++m) { append_lists(D, G.B, G.seq, off[0][m], off[1][m], off[2][m], G.M[m]); D.origin.push_back((long long)m); }
		} else {
			const pga_apply_block_t &E = G.ae[entry[i]];
			const pga_plan_interval_t &I = G.iv[E.interval_a];
			size_t c = 0; while (!(G.cut[c].first_interval <= E.interval_a && E.interval_a < G.cut[c].first_interval + G.cut[c].n_intervals)) ++c;
			D.B.push_back(pga_rc_block_t{G.RB[G.cut[c].block].consensus + I.start, I.end - I.start, G.ab[i].depth});
			for (uint32_t s = 0; s < G.ab[i].depth; ++s) {
				const uint64_t k = G.msrc[E.member_off + s];
				const pga_slice_res_t &Q = G.sl[E.interval_b];
				if (E.kind && k >= Q.member_off && k < Q.member_off + Q.n_kept) {
					size_t p = 0; while (G.pr[p].append_interval != E.interval_b) ++p;
					const pga_mapvar_res_t &R = G.res[first_res[p] + (k - Q.member_off)];
					append_lists(D, G.P, G.p_seq, R.sub_off, R.del_off, R.ins_off, pga_rc_member_t{R.n_subs, R.n_dels, R.n_inss});
				} else append_lists(D, G.SL, G.seq, G.sm[k].sub_off, G.sm[k].del_off, G.sm[k].ins_off, G.sm[k].counts);
				D.origin.push_back(-(1LL + (long long)k));
			}
		}
		for (uint32_t s = 0; s < G.ab[i].depth; ++s) D.who.push_back(pga_detach_member_t{slot[i][s]->node_id, slot[i][s]->reverse ? 1 : 0, 0});
	}
	return D;
}

// ---------------------------------------------------------------- the kernels in the order of pga_assemble.hip
struct ScanBufs {
	Exact<as_u64> tile_sum, tile_off, off; RmScan S;
	ScanBufs(uint64_t n, uint32_t n_q) : tile_sum((size_t)n_q * ((n + AS_TILE - 1) / AS_TILE)), tile_off((size_t)n_q * ((n + AS_TILE - 1) / AS_TILE + 1)), off((size_t)n_q * (n + 1)),
		S{n, (uint32_t)((n + AS_TILE - 1) / AS_TILE), n_q, tile_sum.get(), tile_off.get(), off.get()} {}
};
template <class Val> static void scan(const RmScan &S, const Val &val, unsigned grid)
{
	if (S.n_tiles) emu_launch(dim3(std::min<unsigned>(grid, S.n_tiles)), dim3(AS_THREADS), [&] { k_ts_sums<as_u64, Val>(S, val); });
	emu_launch(dim3(1), dim3(AS_THREADS), [&] { k_ts_scan<as_u64>(S); });
	if (S.n_tiles) emu_launch(dim3(std::min<unsigned>(grid, S.n_tiles)), dim3(AS_THREADS), [&] { k_ts_offsets<as_u64, Val>(S, val); });
}
static void validate(const Case &G, uint32_t flags, AsTables &A, bool with_cut = true)
{
	const pga_slice_out_t sl = G.slice();
	const pga_apply_out_t ap = G.applied();
	as_validate((int64_t)G.RB.size(), G.RB.data(), G.M.data(), G.B.S.data(), G.B.D.data(), G.B.I.data(), with_cut ? (int64_t)G.cut.size() : 0, G.cut.data(), G.iv.data(), (int64_t)G.pr.size(), G.pr.data(), &sl,
	            G.res.data(), G.P.S.data(), G.P.D.data(), G.P.I.data(), &ap, flags, A);
}

// returns false on a CHECK; `refused` says whether the device checks stopped the call (nothing behind them has run then)
static bool emulated(const Case &G, unsigned grid, uint32_t flags, uint64_t seq_len, uint64_t p_seq_len, Out &O, as_u64 err[AS_ERRS], bool &refused)
{
	AsTables A;
	validate(G, flags, A);
	const uint64_t nbo = A.blocks.size(), nmo = A.n_out_members, nmb = A.n_before_members, nk = A.n_slice_members, nn = G.an.size();
	refused = false;
	CHECK(nmb == G.M.size() && nk == G.sm.size() && A.n_res == G.res.size());
	CHECK((flags & PGA_ASSEMBLE_MERGED_ONLY) ? A.before_tot[0] == 0 && A.before_tot[2] == 0 : A.before_tot[0] == G.B.S.size() && A.before_tot[2] == G.B.I.size());
	CHECK(A.slice_tot[0] == G.SL.S.size() && A.slice_tot[1] == G.SL.D.size() && A.slice_tot[2] == G.SL.I.size() && A.p_tot[0] == G.P.S.size() && A.p_tot[1] == G.P.D.size() && A.p_tot[2] == G.P.I.size());
	Exact<AsBlock> blocks(A.blocks); Exact<as_u64> blk_first(A.blk_first), afirst(A.after_first), e((size_t)AS_ERRS); Exact<uint32_t> adepth(A.after_depth), used(nk), slotcnt(nmo);
	Exact<pga_rc_member_t> members(G.M), omembers(nmo); Exact<pga_sub_t> subs(G.B.S), ssubs(G.SL.S), psubs(G.P.S); Exact<pga_del_t> dels(G.B.D), sdels(G.SL.D), pdels(G.P.D);
	Exact<pga_ins_t> inss(G.B.I), sinss(G.SL.I), pinss(G.P.I); Exact<pga_slice_res_t> slices(G.sl); Exact<pga_slice_member_t> smembers(G.sm); Exact<pga_mapvar_res_t> res(G.res);
	Exact<uint64_t> msrc(G.msrc); Exact<char> letters(seq_len + p_seq_len); Exact<pga_topo_node_t> nodes(G.an);
	Exact<AsDesc> desc(nmo); Exact<long long> origin(nmo); Exact<pga_detach_member_t> who(nmo);
	std::copy(G.seq.begin(), G.seq.begin() + seq_len, letters.get()); std::copy(G.p_seq.begin(), G.p_seq.begin() + p_seq_len, letters.get() + seq_len);
	std::fill(e.get(), e.get() + AS_ERRS, AS_NONE);
	ScanBufs b_before(nmb, 3), b_out(nmo, 3);
	AsDev V;
	memset(&V, 0, sizeof(V));
	V.n_out_blocks = nbo; V.n_out_members = nmo; V.n_before_members = nmb; V.n_nodes = nn; V.n_after_blocks = A.n_after_blocks; V.ins_seq_len = seq_len; V.p_ins_seq_len = p_seq_len;
	for (int q = 0; q < 3; ++q) { V.slice_tot[q] = A.slice_tot[q]; V.p_tot[q] = A.p_tot[q]; }
	V.blocks = blocks.get(); V.blk_first = blk_first.get(); V.members = members.get(); V.subs = subs.get(); V.dels = dels.get(); V.inss = inss.get();
	V.slices = slices.get(); V.s_members = smembers.get(); V.s_subs = ssubs.get(); V.s_dels = sdels.get(); V.s_inss = sinss.get();
	V.res = res.get(); V.p_subs = psubs.get(); V.p_dels = pdels.get(); V.p_inss = pinss.get(); V.letters = letters.get(); V.member_src = msrc.get(); V.used = used.get();
	V.desc = desc.get(); V.o_members = omembers.get(); V.origin = origin.get();
	V.nodes = nodes.get(); V.after_first = afirst.get(); V.after_depth = adepth.get(); V.who = who.get(); V.slot_cnt = slotcnt.get(); V.err = e.get();
	V.scan[AS_SCAN_BEFORE] = b_before.S; V.scan[AS_SCAN_OUT] = b_out.S;
	scan(V.scan[AS_SCAN_BEFORE], AsBeforeValue{V}, grid);
	emu_launch(dim3(grid), dim3(AS_THREADS), [&] { k_assemble_desc(V); });
	emu_launch(dim3(grid), dim3(AS_THREADS), [&] { k_assemble_who(V); });
	emu_launch(dim3(grid), dim3(AS_THREADS), [&] { k_assemble_who_check(V); });
	scan(V.scan[AS_SCAN_OUT], AsOutValue{V}, grid);
	std::copy(e.get(), e.get() + AS_ERRS, err);
	for (int i = 0; i < AS_ERRS; ++i) if (err[i] != AS_NONE) { refused = true; return true; }
	const uint64_t ns_out = b_out.off[0 * (nmo + 1) + nmo], nd_out = b_out.off[1 * (nmo + 1) + nmo], ni_out = b_out.off[2 * (nmo + 1) + nmo];
	Exact<pga_sub_t> osubs(ns_out); Exact<pga_del_t> odels(nd_out); Exact<pga_ins_t> oinss(ni_out);
	V.o_subs = osubs.get(); V.o_dels = odels.get(); V.o_inss = oinss.get();
	if (ns_out) emu_launch(dim3(grid), dim3(AS_THREADS), [&] { k_assemble_copy<RM_LIST_SUB>(V); });
	if (nd_out) emu_launch(dim3(grid), dim3(AS_THREADS), [&] { k_assemble_copy<RM_LIST_DEL>(V); });
	if (ni_out) emu_launch(dim3(grid), dim3(AS_THREADS), [&] { k_assemble_copy<RM_LIST_INS>(V); });
	ScanBufs b_let(ni_out, 1);
	V.scan[AS_SCAN_LETTERS] = b_let.S;
	scan(V.scan[AS_SCAN_LETTERS], AsLetterValue{V}, grid);
	std::copy(e.get(), e.get() + AS_ERRS, err);
	for (int i = 0; i < AS_ERRS; ++i) if (err[i] != AS_NONE) { refused = true; return true; }
	const uint64_t nl_out = b_let.off[ni_out];
	Exact<char> oseq(nl_out);
	V.o_ins_seq = oseq.get();
	if (nl_out) emu_launch(dim3(grid), dim3(AS_THREADS), [&] { k_assemble_letters(V); });
	if (ni_out) emu_launch(dim3(grid), dim3(AS_THREADS), [&] { k_assemble_seq_off(V); });
	O.B = A.o_blocks; O.M.assign(omembers.get(), omembers.get() + nmo); O.L.S.assign(osubs.get(), osubs.get() + ns_out); O.L.D.assign(odels.get(), odels.get() + nd_out);
	O.L.I.assign(oinss.get(), oinss.get() + ni_out); O.who.assign(who.get(), who.get() + nmo); O.origin.assign(origin.get(), origin.get() + nmo);
	if (nl_out) O.seq.assign(oseq.get(), nl_out);
	return true;
}

template <class T> static bool same(const std::vector<T> &a, const std::vector<T> &b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0); }
static bool same_blocks(const std::vector<pga_rc_block_t> &a, const std::vector<pga_rc_block_t> &b)
{
	if (a.size() != b.size()) return false;
	for (size_t i = 0; i < a.size(); ++i) if (a[i].consensus != b[i].consensus || a[i].cons_len != b[i].cons_len || a[i].n_members != b[i].n_members) return false;
	return true;
}

static bool run_case(const Case &G, unsigned grid, uint32_t flags)
{
	Out E, D = direct(G, flags);
	as_u64 err[AS_ERRS]; bool refused;
	if (!emulated(G, grid, flags, G.seq.size(), G.p_seq.size(), E, err, refused)) return false;
	CHECK(!refused);
	CHECK(same_blocks(E.B, D.B)); CHECK(same(E.M, D.M)); CHECK(same(E.L.S, D.L.S)); CHECK(same(E.L.D, D.L.D)); CHECK(same(E.L.I, D.L.I));
	CHECK(E.seq == D.seq); CHECK(same(E.who, D.who)); CHECK(same(E.origin, D.origin));
	return true;
}

template <class F> static bool refused_by_host(F f) { try { f(); } catch (std::runtime_error &) { return true; } return false; }

int main()
{
	size_t n_big = 0, n_merged = 0, n_append = 0, n_long = 0, n_empty = 0;
	for (g_case = 0; g_case < 7; ++g_case) {
		const int kind = g_case;                          // 3: more than one tile of members; 4: lists of several tiles; 5: nearly everything cut
		Case G;
		do G = kind == 3 ? generate(600, 4, 3, 0) : kind == 4 ? generate(8, 4, 2, 2 * AS_TILE + 5) : kind == 5 ? generate(30, 3, 1, 0) : generate(6 + rnd(10), 4, 2, 0);
		while (G.cut.empty());                            // (the empty cut has no graph after: it is held on the tables below)
		if (!run_case(G, 1 + rnd(3), 0) || !run_case(G, 2, PGA_ASSEMBLE_MERGED_ONLY)) return 1;
		const Out D = direct(G, 0);
		n_big += D.M.size() > (size_t)AS_TILE; n_long += D.L.S.size() > (size_t)2 * AS_TILE; n_merged += G.pr.size();
		for (const auto &P : G.pr) n_append += G.sl[P.append_interval].n_kept;
		for (const auto &B : G.ab) n_empty += B.depth == 0;
	}
	if (n_big < 1 || n_merged < 20 || n_append < 20 || n_long < 1 || n_empty < 3) {
		fprintf(stderr, "assemble_emu: the generator lost its cases (%zu big, %zu merged blocks, %zu append members, %zu long lists, %zu empty blocks)\n", n_big, n_merged, n_append, n_long, n_empty);
		return 1;
	}
	// ---- exactly 1023 / 1024 / 1025 members after: the last tile of the member scans full, one short, one over
	for (uint64_t target : {(uint64_t)AS_TILE - 1, (uint64_t)AS_TILE, (uint64_t)AS_TILE + 1}) {
		g_case = 100 + (int)target;
		Case G;
		do G = generate(20, 4, 2, 0); while (G.cut.empty() || !pad_to(G, target));
		if (direct(G, 0).M.size() != target || !run_case(G, 2, 0) || !run_case(G, 3, PGA_ASSEMBLE_MERGED_ONLY)) return 1;
	}
	// ---- no cut: the input copied with compacted letters, no who; merged-only: nothing
	g_case = -1;
	{
		Case G = generate(12, 4, 2, 0);
		AsTables A;
		validate(G, 0, A, false);
		if (!A.identity || A.blocks.size() != G.RB.size() || A.n_out_members != G.M.size()) { fprintf(stderr, "assemble_emu: the empty cut is not the identity\n"); return 1; }
		AsTables M;
		validate(G, PGA_ASSEMBLE_MERGED_ONLY, M, false);
		if (!M.blocks.empty() || M.n_out_members) { fprintf(stderr, "assemble_emu: the empty cut has merged blocks\n"); return 1; }
	}
	// ---- what is refused: on the host, and by the kernels before an index is derived
	g_case = -2;
	Case H;
	auto fits = [](const Case &Y) {                       // a promise whose append slice keeps a member with an insertion that has letters; a survivor with members; two cuts
		bool ok = false, surv = false;
		std::vector<uint64_t> first_res(Y.pr.size() + 1, 0);
		for (size_t p = 0; p < Y.pr.size(); ++p) {
			first_res[p + 1] = first_res[p] + Y.sl[Y.pr[p].append_interval].n_kept;
			for (uint64_t r = first_res[p]; r < first_res[p + 1]; ++r) for (uint64_t k = Y.res[r].ins_off; k < Y.res[r].ins_off + Y.res[r].n_inss; ++k) ok = ok || Y.P.I[k].len;
		}
		for (size_t b = 0; b < Y.RB.size(); ++b) surv = surv || (Y.bmap[b] != TP_NONE && Y.RB[b].n_members);
		return ok && surv && Y.res.size() >= 2 && Y.sl[Y.pr[0].anchor_interval].member_off + 1 < Y.sm.size() && Y.cut.size() >= 2 && Y.pr.size() >= 2 && Y.msrc.size() >= 4 && !Y.SL.I.empty() && Y.sl[Y.pr[0].anchor_interval].n_kept && Y.sl[Y.pr[0].append_interval].n_kept;
	};
	do H = generate(14, 4, 2, 0); while (!fits(H));
	auto host = [&](const Case &X, uint32_t flags) { AsTables A; validate(X, flags, A); };
	host(H, 0); host(H, 1);
	bool ok = true;
	size_t surv = 0; while (H.bmap[surv] == TP_NONE || !H.RB[surv].n_members) ++surv;
	Case X = H;                                                        ok = ok && refused_by_host([&] { host(X, 2); });
	X = H; X.cut[0].block = (uint32_t)X.RB.size();                     ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.cut[1].block = X.cut[0].block;                            ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.cut[1].first_interval += 1;                               ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.cut[0].n_intervals = 0;                                   ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.iv[0].start = X.iv[0].end;                                ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.iv[X.cut[0].n_intervals - 1].end = 1000;                  ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.sl[1].member_off += 1;                                    ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.bmap[surv] = TP_NONE;                                     ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.bmap[X.cut[0].block] = 0;                                 ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.bmap[surv] = X.ae[0].block;                               ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.RB[surv].n_members += 1; X.M.push_back(pga_rc_member_t{0, 0, 0});   ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.ab.pop_back();                                            ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.ab.push_back(pga_topo_block_t{1, 1, 0, 1, 0});            ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.ae[1].member_off += 1;                                    ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.ab[X.ae[0].block].depth += 1;                             ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.ae[0].kind = 2;                                           ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.pr[0].append_interval = X.pr[1].append_interval;          ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; std::swap(X.pr[0].anchor_interval, X.pr[1].anchor_interval);  ok = ok && refused_by_host([&] { host(X, 0); });
	X = H; X.pr.pop_back();                                            ok = ok && refused_by_host([&] { host(X, 0); });
	if (!ok) { fprintf(stderr, "assemble_emu: malformed input was accepted by the host\n"); return 1; }
	auto device = [&](const Case &Y, uint64_t seq_len, uint64_t p_seq_len, int which) {
		Out E; as_u64 err[AS_ERRS]; bool refused;
		if (!emulated(Y, 2, 0, seq_len, p_seq_len, E, err, refused)) return false;
		return refused && err[which] != AS_NONE && E.M.empty() && E.L.S.empty();
	};
	size_t merged = 0; while (H.ae[merged].kind != 1 || H.ae[merged].interval_a != H.pr[0].anchor_interval) ++merged;
	const uint64_t mo = H.ae[merged].member_off;
	for (size_t e = 0; e < H.ae.size(); ++e) if (e != merged && H.ab[H.ae[e].block].depth) {                                         // a member of another block
		X = H; X.msrc[mo] = H.msrc[H.ae[e].member_off]; ok = ok && device(X, X.seq.size(), X.p_seq.size(), AS_E_SRC_RANGE);
		break;
	}
	{ X = H; X.msrc[mo] = ~0ULL; ok = ok && device(X, X.seq.size(), X.p_seq.size(), AS_E_SRC_RANGE); }
	{ X = H; X.msrc[mo] = X.msrc[mo + 1]; ok = ok && device(X, X.seq.size(), X.p_seq.size(), AS_E_SRC_TWICE); }
	{ X = H; X.res[0].status = 3; ok = ok && device(X, X.seq.size(), X.p_seq.size(), AS_E_STATUS); }
	{ X = H; X.res[0].sub_off = ~0ULL - 1; X.res[0].n_subs = 5; ok = ok && device(X, X.seq.size(), X.p_seq.size(), AS_E_LIST_RANGE); }
	{ X = H; X.sm[H.sl[H.pr[0].anchor_interval].member_off].ins_off = X.SL.I.size() + 1; ok = ok && device(X, X.seq.size(), X.p_seq.size(), AS_E_LIST_RANGE); }
	ok = ok && device(H, H.seq.size(), 0, AS_E_SEQ_RANGE);
	ok = ok && device(H, 3, H.p_seq.size(), AS_E_SEQ_RANGE);
	{ X = H; for (auto &I : X.P.I) I.seq_off = ~0ULL - 2; ok = ok && device(X, X.seq.size(), X.p_seq.size(), AS_E_SEQ_RANGE); }        // (seq_off + len wraps)
	{ X = H; X.an[1].block = X.an[0].block; X.an[1].member = X.an[0].member; ok = ok && device(X, X.seq.size(), X.p_seq.size(), AS_E_SLOT_TWICE); }
	{ X = H; X.an.pop_back(); ok = ok && device(X, X.seq.size(), X.p_seq.size(), AS_E_SLOT_EMPTY); }
	{ X = H; X.an[0].member = X.ab[X.an[0].block].depth; ok = ok && device(X, X.seq.size(), X.p_seq.size(), AS_E_SLOT_RANGE); }
	{ X = H; X.an[0].block = (uint32_t)X.ab.size(); ok = ok && device(X, X.seq.size(), X.p_seq.size(), AS_E_SLOT_RANGE); }
	if (!ok) { fprintf(stderr, "assemble_emu: malformed input passed the kernels' checks\n"); return 1; }
	// ---- the message of a failed result names the promise and the member
	{
		X = H; AsTables A; validate(X, 0, A);
		as_u64 err[AS_ERRS]; std::fill(err, err + AS_ERRS, AS_NONE);
		uint64_t m = 0; while (A.blocks[ts_last_le(A.blk_first.data(), 0, A.blocks.size(), m)].kind != AS_K_MERGED) ++m;
		err[AS_E_STATUS] = m;
		const AsBlock &B = A.blocks[ts_last_le(A.blk_first.data(), 0, A.blocks.size(), m)];
		std::string msg;
		try { as_report(err, A, X.sl[B.ib].member_off + 0, X.sl.data()); } catch (std::runtime_error &e2) { msg = e2.what(); }
		if (msg.find("promise " + std::to_string(B.promise) + ", member 0") == std::string::npos) { fprintf(stderr, "assemble_emu: the message is off: %s\n", msg.c_str()); return 1; }
	}
	printf("assemble_emu OK (%zu graphs of more than one tile, %zu merged blocks, %zu append members, %zu with long lists, %zu empty blocks)\n", n_big, n_merged, n_append, n_long, n_empty);
	return 0;
}
