// pga_reweave_idx.h without a device: the host tables of rw_build_tables, then every kernel of the header under dev/emu/hip_emu.h -- the
// rocPRIM sorts and scans of pga_reweave.hip replaced by std::stable_sort and plain loops -- with every buffer allocated at exactly the size
// the kernels may touch (under the address sanitizer an access one entry out is an error), against a direct scalar construction of
// reweave's front half (reweave.rs:132-340, pangraph_interval.rs:98-255, cigar.rs:26-96): lists and loops, add_flanking_indel literally.
// Build and run (host only):  g++ -std=c++17 -g -O1 -DPGA_EMU -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined
//                             tests/emu/reweave_emu.cpp -o reweave_emu && ./reweave_emu
#include <cstdio>
#include <array>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <string>
#include "../../dev/emu/hip_emu.h"
#include "../../pangraph_amd/csrc/pga_reweave_idx.h"
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

struct Level {
	std::vector<int64_t> group_off{0};
	std::vector<std::string> cons; std::vector<pga_plan_block_t> blocks;
	std::vector<pga_match_t> matches; std::vector<uint32_t> cigars;
	uint32_t thr;
};

// ---------------------------------------------------------------- the direct construction
typedef std::pair<uint32_t, uint32_t> Op;                               // (kind, len)
struct Iv { uint32_t start, end; bool aligned; uint64_t id; bool is_anchor, reverse; int64_t match; uint32_t el, er; bool has_el, has_er; std::vector<Op> cigar; };
static bool is_m(uint32_t k) { return k == 0 || k == 7 || k == 8; }
static std::vector<Op> add_flanking_indel(const std::vector<Op> &cg, uint32_t kind, uint32_t add, bool leading)
{
	int replace = -1;
	if (leading) { for (size_t i = 0; i < cg.size(); ++i) { if (is_m(cg[i].first)) break; if (cg[i].first == kind) replace = (int)i; } }
	else { for (size_t i = cg.size(); i-- > 0;) { if (is_m(cg[i].first)) break; if (cg[i].first == kind) replace = (int)i; } }
	std::vector<Op> out = cg;
	if (replace >= 0) out[replace].second += add;
	else out.insert(leading ? out.begin() : out.end(), Op(kind, add));
	return out;
}
static uint64_t hash_words(std::initializer_list<uint64_t> w)
{
	std::vector<uint8_t> b;
	for (uint64_t x : w) for (int i = 0; i < 8; ++i) b.push_back((uint8_t)(x >> (8 * i)));
	return xxh64_bytes(b.data(), b.size(), 0);
}
struct Direct {
	std::vector<pga_plan_match_t> matches;
	struct Blk { uint32_t block; int status; int64_t fail; std::vector<Iv> iv; size_t before; };
	std::vector<Blk> blocks;
	struct Prom { uint64_t id; int64_t match; uint32_t a_blk, q_blk, a_s, a_e, q_s, q_e; bool reverse; std::vector<Op> cigar; };
	std::vector<Prom> promises;
	uint64_t n_failed = 0;
};
static Direct direct(const Level &L)
{
	Direct D;
	const size_t nm = L.matches.size();
	D.matches.resize(nm);
	for (size_t m = 0; m < nm; ++m) {
		const pga_match_t &A = L.matches[m];
		const int64_t b0 = L.group_off[A.group];
		const pga_plan_block_t &R = L.blocks[b0 + A.ref], &Q = L.blocks[b0 + A.qry];
		pga_plan_match_t O{};
		O.new_block_id = hash_words({Q.block_id, (uint64_t)A.qry_start, (uint64_t)A.qry_end, R.block_id, (uint64_t)A.ref_start, (uint64_t)A.ref_end});
		if (R.depth != Q.depth) { O.anchor = R.depth > Q.depth ? 0 : 1; O.route = 0; }
		else {
			uint32_t rn = 0, qn = 0;
			for (int32_t i = A.ref_start; i < A.ref_end; ++i) rn += R.consensus[i] == 'N';
			for (int32_t i = A.qry_start; i < A.qry_end; ++i) qn += Q.consensus[i] == 'N';
			O.anchor = rn <= qn ? 0 : 1; O.route = 2; O.ref_n = rn; O.qry_n = qn;
		}
		D.matches[m] = O;
	}
	for (size_t g = 0; g + 1 < L.group_off.size(); ++g) {
		std::map<uint64_t, uint32_t> by_id;                              // BTreeMap order
		for (int64_t b = L.group_off[g]; b < L.group_off[g + 1]; ++b) by_id[L.blocks[b].block_id] = (uint32_t)b;
		struct Half { uint64_t id; uint32_t blk, s, e; bool anchor, reverse; std::vector<Op> cigar; uint32_t el, er; bool hel, her; int64_t match; };
		std::vector<Half> halves;
		for (auto &kv : by_id) {
			const uint32_t b = kv.second;
			std::vector<Iv> hits;
			for (size_t m = 0; m < nm; ++m) {
				const pga_match_t &A = L.matches[m];
				if ((size_t)A.group != g) continue;
				const int64_t b0 = L.group_off[g];
				std::vector<Op> cg;
				for (uint32_t i = 0; i < A.n_cigar; ++i) cg.push_back(Op(L.cigars[A.cigar_off + i] & 15u, L.cigars[A.cigar_off + i] >> 4));
				if ((uint32_t)(b0 + A.ref) == b) {
					Iv h{(uint32_t)A.ref_start, (uint32_t)A.ref_end, true, D.matches[m].new_block_id, D.matches[m].anchor == 0, A.reverse != 0, (int64_t)m, 0, 0, false, false, {}};
					if (h.is_anchor) h.cigar = cg;
					hits.push_back(h);
				}
				if ((uint32_t)(b0 + A.qry) == b) {
					Iv h{(uint32_t)A.qry_start, (uint32_t)A.qry_end, true, D.matches[m].new_block_id, D.matches[m].anchor == 1, A.reverse != 0, (int64_t)m, 0, 0, false, false, {}};
					if (h.is_anchor) {
						if (A.reverse) std::reverse(cg.begin(), cg.end());
						for (Op &o : cg) o.first = o.first == 1 ? 2 : o.first == 2 ? 1 : o.first;
						h.cigar = cg;
					}
					hits.push_back(h);
				}
			}
			if (hits.empty()) continue;
			// create_intervals
			std::stable_sort(hits.begin(), hits.end(), [](const Iv &x, const Iv &y) { return x.start < y.start; });
			std::vector<Iv> iv; uint32_t cursor = 0;
			const uint32_t len = L.blocks[b].cons_len;
			for (const Iv &h : hits) {
				if (h.start > cursor) iv.push_back(Iv{cursor, h.start, false, hash_words({L.blocks[b].block_id, cursor, h.start}), false, false, -1, 0, 0, false, false, {}});
				iv.push_back(h); cursor = h.end;
			}
			if (cursor < len) iv.push_back(Iv{cursor, len, false, hash_words({L.blocks[b].block_id, cursor, len}), false, false, -1, 0, 0, false, false, {}});
			// refine_intervals
			Direct::Blk B{b, 0, -1, {}, iv.size()};
			std::vector<std::pair<size_t, size_t>> mergers;
			for (size_t n = 0; n < iv.size() && !B.status; ++n) {
				const uint32_t l = iv[n].end - iv[n].start;
				if (l >= L.thr) continue;
				const uint32_t left = n > 0 ? iv[n - 1].end - iv[n - 1].start : 0, right = n + 1 < iv.size() ? iv[n + 1].end - iv[n + 1].start : 0;
				if (iv[n].aligned) B.status = 1;
				else if (n > 0 && !iv[n - 1].aligned) B.status = 2;
				else if (n > 0 && left < L.thr) B.status = 3;
				else if (n + 1 < iv.size() && !iv[n + 1].aligned) B.status = 4;
				else if (n + 1 < iv.size() && right < L.thr) B.status = 5;
				if (B.status) { B.fail = (int64_t)n; break; }
				mergers.push_back(left >= right ? std::make_pair(n, n - 1) : std::make_pair(n, n + 1));
			}
			if (B.status) { ++D.n_failed; D.blocks.push_back(B); continue; }
			for (size_t k = mergers.size(); k-- > 0;) {
				const size_t from = mergers[k].first, to = mergers[k].second;
				const uint32_t l = iv[from].end - iv[from].start;
				if (from < to) { iv[to].start = iv[from].start; iv[to].el += l; iv[to].has_el = true; }
				else { iv[to].end = iv[from].end; iv[to].er += l; iv[to].has_er = true; }
				iv.erase(iv.begin() + from);
			}
			for (const Iv &x : iv) if (x.aligned) halves.push_back(Half{x.id, b, x.start, x.end, x.is_anchor, x.reverse, x.cigar, x.el, x.er, x.has_el, x.has_er, x.match});
			B.iv = iv;
			D.blocks.push_back(B);
		}
		// group_promises
		std::stable_sort(halves.begin(), halves.end(), [](const Half &x, const Half &y) { return x.id < y.id; });
		for (size_t k = 0; k + 1 < halves.size(); k += 2) {
			const Half &A = halves[k].anchor ? halves[k] : halves[k + 1], &Q = halves[k].anchor ? halves[k + 1] : halves[k];
			if (halves[k].id != halves[k + 1].id || A.anchor == Q.anchor) continue;      // (a block of the group failed: the lists are not compared)
			std::vector<Op> cg = A.cigar;
			if (A.hel) cg = add_flanking_indel(cg, 2, A.el, true);
			if (A.her) cg = add_flanking_indel(cg, 2, A.er, false);
			if (Q.hel) cg = add_flanking_indel(cg, 1, Q.el, !A.reverse);
			if (Q.her) cg = add_flanking_indel(cg, 1, Q.er, A.reverse);
			D.promises.push_back(Direct::Prom{A.id, A.match, A.blk, Q.blk, A.s, A.e, Q.s, Q.e, A.reverse, cg});
		}
	}
	return D;
}

// ---------------------------------------------------------------- the kernels
static uint64_t n_levels, n_match_total, n_fail_levels, n_route[3], n_flank_ops, n_codes[6];
#define FAIL(...) do { printf("round %d: ", round); printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

static int run(const Level &L, int round, bool resident)
{
	RwTables T;
	// the bit plane: every block at an odd base offset of one store, 16 bases per word, a pad word behind
	std::vector<RwResident> res; std::vector<uint16_t> plane;
	if (resident) {
		uint64_t at = 3;
		std::vector<uint64_t> pos;
		for (const pga_plan_block_t &b : L.blocks) { pos.push_back(at); at += b.cons_len; }
		plane.assign((size_t)((at + 15) / 16), 0);
		for (size_t i = 0; i < L.blocks.size(); ++i) for (uint32_t k = 0; k < L.blocks[i].cons_len; ++k) {
			const char c = L.blocks[i].consensus[k], u = (char)(c & 0xdf);
			if (c < 0x40 || !(u == 'A' || u == 'C' || u == 'G' || u == 'T' || u == 'U')) plane[(size_t)((pos[i] + k) >> 4)] |= (uint16_t)(1u << ((pos[i] + k) & 15));
		}
		for (size_t i = 0; i < L.blocks.size(); ++i) res.push_back(RwResident{plane.data(), pos[i]});
	}
	rw_build_tables((int32_t)L.group_off.size() - 1, L.group_off.data(), L.blocks.data(), (int64_t)L.matches.size(), L.matches.data(), L.cigars.data(), L.cigars.size(),
	                resident ? res.data() : nullptr, T);
	const uint64_t nm = L.matches.size(), nh = 2 * nm, n_hb = T.hb_block.size();
	if (nm == 0) return 0;
	const uint64_t cap_iv = 2 * nh + n_hb, cap_cig = T.cigar_in + 4 * nm;
	Exact<uint32_t> ncnt(nh), hval(nh), hs(nh), pval(nm), pgrp(nm), pm(nm), cnt_b(nh + 1), cnt_a(nh + 1), herr(nh + 1), off_b(nh + 1), off_a(nh + 1), err(4), o_cig(cap_cig);
	Exact<rw_u64> hkey(nh), pkey(nm), iv_of(nh), b_first(n_hb), b_firstb(n_hb), b_end(n_hb), b_err(n_hb), n_out(nm + 1), c_off(nm + 1), counters(RW_COUNTERS);
	Exact<pga_plan_match_t> o_match(nm); Exact<RwExt> ext(nh); Exact<pga_plan_block_res_t> o_blk(n_hb); Exact<pga_plan_interval_t> o_iv(cap_iv);
	Exact<pga_slice_interval_t> o_siv(cap_iv); Exact<RwPlan> plan(nm); Exact<pga_plan_promise_t> o_prom(nm);
	RwDev V;
	V.n_matches = nm; V.n_hits = nh; V.n_hb = n_hb; V.cap_iv = cap_iv; V.cap_cig = cap_cig; V.thr_len = L.thr; V.pad = 0;
	V.blk = T.blk.data(); V.mt = T.mt.data(); V.cig = L.cigars.data(); V.ncnt = ncnt.get(); V.o_match = o_match.get();
	V.hkey = hkey.get(); V.hval = hval.get(); V.pkey = pkey.get(); V.pval = pval.get(); V.pgrp = pgrp.get(); V.hs = hs.get();
	V.cnt_b = cnt_b.get(); V.cnt_a = cnt_a.get(); V.herr = herr.get(); V.off_b = off_b.get(); V.off_a = off_a.get(); V.ext = ext.get(); V.iv_of = iv_of.get();
	V.b_first = b_first.get(); V.b_firstb = b_firstb.get(); V.b_end = b_end.get(); V.b_err = b_err.get(); V.o_blk = o_blk.get(); V.o_iv = o_iv.get(); V.o_siv = o_siv.get();
	V.pm = pm.get(); V.plan = plan.get(); V.n_out = n_out.get(); V.c_off = c_off.get(); V.o_prom = o_prom.get(); V.o_cig = o_cig.get();
	V.counters = counters.get(); V.err = err.get();
	const unsigned grid = 1 + rnd(3);                                       // (fewer threads than records: the grid-stride loops are walked)
	std::vector<uint8_t> stage; std::vector<RwJob> jobs;
	auto stage_letters = [&](const std::vector<uint32_t> &which) {
		jobs.clear(); uint64_t bytes = 0;
		for (uint32_t m : which) for (uint32_t s = 0; s < 2; ++s) { const RwMatch &M = T.mt[m]; jobs.push_back(RwJob{bytes, 2 * m + s, M.end[s] - M.start[s]}); bytes += ((uint64_t)(M.end[s] - M.start[s]) + 15) & ~15ULL; }
		stage.assign((size_t)bytes, 0);
		for (const RwJob &J : jobs) { const RwMatch &M = T.mt[J.side >> 1]; memcpy(stage.data() + J.off, L.blocks[M.blk[J.side & 1]].consensus + M.start[J.side & 1], J.len); }
		for (uint32_t m : which) T.mt[m].letters = 1;
	};
	if (!resident && !T.eq.empty()) stage_letters(T.eq);
	for (int pass = 0; pass < 2; ++pass) {
		for (int i = 0; i < RW_COUNTERS; ++i) counters[i] = 0;
		for (int i = 0; i < 4; ++i) err[i] = 0;
		for (uint64_t b = 0; b < n_hb; ++b) b_err[b] = ~0ULL;
		if (pass == 0 && resident && !T.eq.empty()) {
			std::vector<uint32_t> sides;
			for (uint32_t m : T.eq) { sides.push_back(2 * m); sides.push_back(2 * m + 1); }
			emu_launch(dim3(grid), dim3(RW_THREADS), [&] { k_rw_mask(V, sides.data(), sides.size()); });
		}
		if (!jobs.empty()) {
			std::vector<RwV4> st16(stage.size() / 16);                          // (exactly the staged bytes, 16-aligned)
			memcpy(st16.data(), stage.data(), stage.size());
			emu_launch(dim3(grid), dim3(RW_THREADS), [&] { k_rw_letters(V, jobs.data(), jobs.size(), st16.data()); });
		}
		emu_launch(dim3(grid), dim3(RW_THREADS), [&] { k_rw_match(V); });
		{   // (stands in for the radix sorts)
			std::vector<uint32_t> o(nh); for (uint64_t i = 0; i < nh; ++i) o[i] = (uint32_t)i;
			std::stable_sort(o.begin(), o.end(), [&](uint32_t x, uint32_t y) { return hkey[x] < hkey[y]; });
			for (uint64_t i = 0; i < nh; ++i) hs[i] = hval[o[i]];
			std::vector<uint32_t> q(nm); for (uint64_t i = 0; i < nm; ++i) q[i] = (uint32_t)i;
			std::stable_sort(q.begin(), q.end(), [&](uint32_t x, uint32_t y) { return pkey[x] < pkey[y]; });
			std::vector<uint32_t> by_id(nm); for (uint64_t i = 0; i < nm; ++i) by_id[i] = pval[q[i]];
			emu_launch(dim3(grid), dim3(RW_THREADS), [&] { k_rw_groups(V, by_id.data()); });
			for (uint64_t i = 0; i < nm; ++i) q[i] = (uint32_t)i;
			std::stable_sort(q.begin(), q.end(), [&](uint32_t x, uint32_t y) { return pgrp[x] < pgrp[y]; });
			for (uint64_t i = 0; i < nm; ++i) pm[i] = by_id[q[i]];
		}
		emu_launch(dim3(grid), dim3(RW_THREADS), [&] { k_rw_hits(V); });
		{ uint32_t a = 0, b = 0; for (uint64_t h = 0; h <= nh; ++h) { off_b[h] = b; off_a[h] = a; b += cnt_b[h]; a += cnt_a[h]; } }
		emu_launch(dim3(grid), dim3(RW_THREADS), [&] { k_rw_intervals(V); });
		emu_launch(dim3(grid), dim3(RW_THREADS), [&] { k_rw_blocks(V); });
		emu_launch(dim3(grid), dim3(RW_THREADS), [&] { k_rw_cigar_plan(V); });
		{ rw_u64 c = 0; for (uint64_t p = 0; p <= nm; ++p) { c_off[p] = c; c += n_out[p]; } }
		emu_launch(dim3(grid), dim3(RW_THREADS), [&] { k_rw_cigar_write(V); });
		if (counters[RW_C_UNDECIDED] == 0) break;
		if (pass == 1) FAIL("undecided after the letters pass");
		std::vector<uint32_t> need;
		for (uint32_t m : T.eq) if (ncnt[2 * (size_t)m] | ncnt[2 * (size_t)m + 1]) need.push_back(m);
		if (need.size() != counters[RW_C_UNDECIDED]) FAIL("the matches that need letters");
		stage_letters(need);
	}
	if (err[0]) FAIL("device error %u", err[0]);
	// ---- against the direct construction ----
	const Direct D = direct(L);
	for (uint64_t m = 0; m < nm; ++m) {
		const pga_plan_match_t &a = o_match[m], &b = D.matches[m];
		const bool by_mask = a.route == 1;
		if (a.new_block_id != b.new_block_id || a.anchor != b.anchor || (a.route == 0) != (b.route == 0) || (by_mask ? (a.ref_n || a.qry_n || b.ref_n || b.qry_n || !resident) : (a.ref_n != b.ref_n || a.qry_n != b.qry_n)))
			FAIL("match %llu: id %llx / %llx anchor %d / %d route %d / %d n %u %u / %u %u", (unsigned long long)m, (unsigned long long)a.new_block_id, (unsigned long long)b.new_block_id, a.anchor, b.anchor, a.route, b.route, a.ref_n, a.qry_n, b.ref_n, b.qry_n);
		++n_route[a.route];
	}
	if (D.blocks.size() != n_hb || counters[RW_C_FAILED] != D.n_failed) FAIL("blocks with a hit %llu / %zu, failed %llu / %llu", (unsigned long long)n_hb, D.blocks.size(), counters[RW_C_FAILED], (unsigned long long)D.n_failed);
	size_t before = 0, at = 0;
	for (uint64_t b = 0; b < n_hb; ++b) {
		const Direct::Blk &B = D.blocks[b]; const pga_plan_block_res_t &O = o_blk[b];
		before += B.before;
		if (T.hb_block[b] != B.block || O.status != B.status || O.fail_interval != B.fail) FAIL("block %llu: block %u / %u status %d / %d fail %lld / %lld", (unsigned long long)b, T.hb_block[b], B.block, O.status, B.status, (long long)O.fail_interval, (long long)B.fail);
		++n_codes[B.status];
		if (D.n_failed) continue;
		if (O.first_interval != at || O.n_intervals != B.iv.size()) FAIL("block %llu: intervals %llu + %u, direct %zu + %zu", (unsigned long long)b, (unsigned long long)O.first_interval, O.n_intervals, at, B.iv.size());
		for (const Iv &x : B.iv) {
			const pga_plan_interval_t &I = o_iv[at]; const pga_slice_interval_t &S = o_siv[at];
			if (I.start != x.start || I.end != x.end || I.aligned != (int)x.aligned || I.new_block_id != x.id || I.is_anchor != (int)x.is_anchor || I.reverse != (int)x.reverse || I.match != x.match ||
			    I.extend_left != x.el || I.extend_right != x.er || S.start != x.start || S.end != x.end || S.flip != (int)(x.aligned && !x.is_anchor && x.reverse))
				FAIL("interval %zu of block %llu", at, (unsigned long long)b);
			++at;
		}
	}
	if (off_b[nh] != before) FAIL("intervals before refinement %u / %zu", off_b[nh], before);
	if (D.n_failed) { ++n_fail_levels; ++n_levels; n_match_total += nm; return 0; }
	if (off_a[nh] != at || D.promises.size() != nm) FAIL("totals");
	rw_u64 cig_at = 0;
	for (uint64_t p = 0; p < nm; ++p) {
		const Direct::Prom &P = D.promises[p]; const pga_plan_promise_t &O = o_prom[p];
		if (O.new_block_id != P.id || O.match != P.match || O.anchor_block != P.a_blk || O.append_block != P.q_blk || O.reverse != (int)P.reverse || O.cigar_off != cig_at || O.n_cigar != P.cigar.size())
			FAIL("promise %llu: id %llx / %llx match %lld / %lld n_cigar %u / %zu", (unsigned long long)p, (unsigned long long)O.new_block_id, (unsigned long long)P.id, (long long)O.match, (long long)P.match, O.n_cigar, P.cigar.size());
		const pga_plan_interval_t &A = o_iv[O.anchor_interval], &Q = o_iv[O.append_interval];
		if (A.start != P.a_s || A.end != P.a_e || Q.start != P.q_s || Q.end != P.q_e || !A.is_anchor || Q.is_anchor || A.match != P.match || Q.match != P.match) FAIL("promise %llu: its intervals", (unsigned long long)p);
		for (size_t k = 0; k < P.cigar.size(); ++k) if (o_cig[cig_at + k] != (P.cigar[k].second << 4 | P.cigar[k].first)) FAIL("promise %llu: operation %zu is %u%c, direct %u%c", (unsigned long long)p, k, o_cig[cig_at + k] >> 4, "MIDNSHP=XB"[o_cig[cig_at + k] & 15], P.cigar[k].second, "MIDNSHP=XB"[P.cigar[k].first]);
		n_flank_ops += P.cigar.size() - L.matches[P.match].n_cigar;
		cig_at += P.cigar.size();
	}
	if (c_off[nm] != cig_at) FAIL("CIGAR total");
	++n_levels; n_match_total += nm;
	return 0;
}

// ---------------------------------------------------------------- levels
static std::string letters(uint32_t n, const char *alphabet) { std::string s; const uint32_t k = (uint32_t)strlen(alphabet); for (uint32_t i = 0; i < n; ++i) s.push_back(alphabet[rnd(k)]); return s; }
// blocks as lists of pieces: gap lengths and hit lengths; the hits of a key are paired
struct Piece { bool hit; uint32_t len; int key; };
static void add_group(Level &L, const std::vector<std::vector<Piece>> &lay, const std::vector<uint32_t> &depth, const char *alphabet, int cigar_len /* -1: random */)
{
	const int g = (int)L.group_off.size() - 1; const int64_t b0 = L.group_off.back();
	std::map<int, std::vector<std::array<uint32_t, 3>>> seen;
	for (size_t b = 0; b < lay.size(); ++b) {
		uint32_t at = 0;
		for (const Piece &p : lay[b]) { if (p.hit) seen[p.key].push_back({(uint32_t)b, at, at + p.len}); at += p.len; }
		L.cons.push_back(letters(at, alphabet));
	}
	L.group_off.push_back(b0 + (int64_t)lay.size());
	for (size_t b = 0; b < lay.size(); ++b) L.blocks.push_back(pga_plan_block_t{(uint64_t)rng() << 20 ^ (1000 - b), nullptr, 0, depth[b]});
	for (auto &kv : seen) {
		const auto &o = kv.second;
		const bool swap = rnd(2);
		const auto &r = swap ? o[1] : o[0], &q = swap ? o[0] : o[1];
		pga_match_t M; memset(&M, 0, sizeof(M));
		M.group = g; M.ref = (int32_t)r[0]; M.ref_start = (int32_t)r[1]; M.ref_end = (int32_t)r[2]; M.qry = (int32_t)q[0]; M.qry_start = (int32_t)q[1]; M.qry_end = (int32_t)q[2];
		M.reverse = (int32_t)rnd(2); M.cigar_off = L.cigars.size();
		static const uint32_t lens[] = {0, 1, 2, 5, 9, 63, 64, 65, 130};
		const uint32_t n = cigar_len >= 0 ? (uint32_t)cigar_len : lens[rnd(9)];
		const bool no_m = rnd(6) == 0;
		for (uint32_t i = 0; i < n; ++i) { const uint32_t kinds[] = {0, 1, 2, 7, 8, 1, 2}; L.cigars.push_back((1 + rnd(40)) << 4 | (no_m ? 1 + rnd(2) : kinds[rnd(i < 3 || i + 3 >= n ? 7 : 5)])); }
		M.n_cigar = n;
		L.matches.push_back(M);
	}
}
static void finish(Level &L) { for (size_t i = 0; i < L.blocks.size(); ++i) { L.blocks[i].consensus = L.cons[i].data(); L.blocks[i].cons_len = (uint32_t)L.cons[i].size(); } }

static Level random_level(bool may_fail)
{
	static const uint32_t thrs[] = {0, 1, 20, 20, 20, 33};
	static const char *const alphabets[] = {"ACGT", "ACGTN", "ACGTNRYn-"};
	Level L; L.thr = thrs[rnd(6)];
	const uint32_t thr = L.thr;
	const char *alphabet = alphabets[rnd(3)];
	for (uint32_t g = 1 + rnd(5); g-- > 0;) {
		const uint32_t nb = 2 + rnd(7);
		std::vector<std::vector<int>> slots(nb);
		const uint32_t nk = rnd(5) == 0 ? 0 : 1 + rnd(rnd(4) == 0 ? 70 : 3 * nb);
		for (uint32_t k = 0; k < nk; ++k) { const uint32_t a = rnd(nb), b = (a + 1 + rnd(nb - 1)) % nb; slots[a].push_back((int)k); slots[b].push_back((int)k); }
		std::vector<std::vector<Piece>> lay(nb); std::vector<uint32_t> depth(nb);
		for (uint32_t b = 0; b < nb; ++b) {
			std::shuffle(slots[b].begin(), slots[b].end(), rng);
			const uint32_t gaps[] = {0, 0, 1, thr ? thr - 1 : 0, thr, thr + 1, 3 * thr + 2};
			for (int k : slots[b]) {
				lay[b].push_back(Piece{false, gaps[rnd(7)], -1});
				lay[b].push_back(Piece{true, may_fail && rnd(12) == 0 && thr > 1 ? 1 + rnd(thr - 1) : std::max(1u, thr) + rnd(40), k});
			}
			lay[b].push_back(Piece{false, gaps[rnd(7)], -1});
			depth[b] = 1 + rnd(3);
		}
		add_group(L, lay, depth, alphabet, -1);
	}
	finish(L);
	return L;
}
// the shapes named in the issue: 1, 2, 63, 64, 65 hits on a block; all four flanks on CIGARs of 1 .. 3001 operations
static Level edge_level()
{
	Level L; L.thr = 20;
	std::vector<std::vector<Piece>> lay; int key = 0;
	for (uint32_t n : {1u, 2u, 63u, 64u, 65u}) {
		std::vector<Piece> big;
		static const uint32_t gaps[] = {0, 20, 19, 23, 1};
		for (uint32_t t = 0; t < n; ++t) { big.push_back(Piece{false, gaps[(t + n) % 5], -1}); big.push_back(Piece{true, 20 + t % 11, key + (int)t}); }
		lay.push_back(big);
		for (uint32_t t = 0; t < n; ++t) lay.push_back({Piece{false, t % 3, -1}, Piece{true, 20 + t % 13, key + (int)t}, Piece{false, (t % 4) * 6, -1}});
		key += (int)n;
	}
	add_group(L, lay, std::vector<uint32_t>(lay.size(), 1), "ACGT", -1);
	for (int n : {1, 63, 64, 65, 3001}) for (uint32_t d = 0; d < 3; ++d)
		add_group(L, {{Piece{false, 19, -1}, Piece{true, 25, 0}, Piece{false, 3, -1}}, {Piece{false, 2, -1}, Piece{true, 22, 0}, Piece{false, 1, -1}}}, {1u + (d == 0), 1u + (d == 1)}, "ACGTN", n);
	finish(L);
	return L;
}

int main()
{
	// XXH64 of 24 and 48 bytes against the byte-stream implementation
	for (int t = 0; t < 200; ++t) {
		uint64_t w[6]; uint8_t b[48];
		for (int i = 0; i < 6; ++i) { w[i] = t < 2 ? (uint64_t)t * ~0ULL : ((uint64_t)rng() << 32 | rng()); for (int k = 0; k < 8; ++k) b[8 * i + k] = (uint8_t)(w[i] >> (8 * k)); }
		if (xxh64_words(w, 3) != xxh64_bytes(b, 24, 0) || xxh64_words(w, 6) != xxh64_bytes(b, 48, 0)) { printf("XXH64 of words\n"); return 1; }
	}
	for (uint32_t x : {0u, 0x4Eu, 0x4E4E4E4Eu, 0x4E004E4Fu, 0x4D4E4F4Eu, 0xCE4E6E4Eu, 0x4E4E4E4Du}) {
		uint32_t want = 0; for (int k = 0; k < 4; ++k) want += ((x >> (8 * k)) & 255u) == 'N';
		if (rw_count_n(x) != want) { printf("rw_count_n(%08x)\n", x); return 1; }
	}
	{ const Level E = edge_level(); if (run(E, -1, false) || run(E, -2, true)) return 1; }
	if (n_fail_levels) { printf("the edge level fails\n"); return 1; }
	for (int round = 0; round < 18; ++round) { const Level L = random_level(round % 3 == 2); if (run(L, round, round % 2 == 0)) return 1; }
	if (n_levels < 15 || n_match_total < 800 || n_fail_levels < 2 || n_fail_levels > 10 || !n_route[0] || !n_route[1] || !n_route[2] || n_flank_ops < 50 || !n_codes[1] || !n_codes[5]) {
		printf("the generator is too tame: %llu levels (%llu fail), %llu matches, routes %llu %llu %llu, %llu flank operations, codes 1: %llu 5: %llu\n", (unsigned long long)n_levels, (unsigned long long)n_fail_levels,
		       (unsigned long long)n_match_total, (unsigned long long)n_route[0], (unsigned long long)n_route[1], (unsigned long long)n_route[2], (unsigned long long)n_flank_ops, (unsigned long long)n_codes[1], (unsigned long long)n_codes[5]);
		return 1;
	}
	if (n_codes[2] || n_codes[3] || n_codes[4]) { printf("a status that create_intervals cannot lead to\n"); return 1; }
	printf("reweave_emu OK: %llu levels (%llu with a failing block), %llu matches, routes %llu / %llu / %llu, %llu inserted flank operations, statuses 1: %llu 5: %llu\n", (unsigned long long)n_levels,
	       (unsigned long long)n_fail_levels, (unsigned long long)n_match_total, (unsigned long long)n_route[0], (unsigned long long)n_route[1], (unsigned long long)n_route[2], (unsigned long long)n_flank_ops,
	       (unsigned long long)n_codes[1], (unsigned long long)n_codes[5]);
	return 0;
}
