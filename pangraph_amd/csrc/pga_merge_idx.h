// pga_merge_idx.h -- the index arithmetic of pga_merge.hip (merge_blocks.rs:92-148 concatenate_alignments over PangraphBlock::reverse_complement,
// pangraph_block.rs:63-75, and Edit::{reverse_complement, shift, concat}, edits.rs:257-304): the host tables and the list kernels.  None of
// them uses a wave intrinsic, so all of this compiles under hipcc and, with dev/emu/hip_emu.h included first, under g++ -std=c++17 -DPGA_EMU
// (tests/emu/merge_emu.cpp runs it against a direct scalar construction).  The one-wave scan of pga_merge.hip (wave_incl_u64 of pga_wave.h) is not in here.
//
// An OUTPUT MEMBER is (edge, k): the k-th member of the edge's left block joined with member partner[k] of its right block.  Each of its
// two SIDES is one input member read through its block's orientation:
//   position maps   sub: pos -> len-pos-1   del: pos -> len-pos-len_d   ins: pos -> len-pos       (*_rc; otherwise the identity)
//   primed order    forward: list order.  *_rc: stably sorted by mapped position -- the reversed list when the mapped positions are strictly
//                   decreasing (the usual case: a bit per list says otherwise), else every entry's exact stable rank, an O(n) scan per entry
//   concat          subs, dels: left' then right' + L_left.  inss: left' first; a right' insertion joins the FIRST accumulated insertion at
//                   its position, else it is pushed.  Positions of the two sides meet only at the boundary (left' at L_left, right' at 0):
//                   first_l is the first left' insertion at L_left (the lowest source index among them, in both orientations), and every
//                   right' insertion at 0 joins it.  Right' insertions that share a position among themselves join their LEADER, the one of
//                   lowest source index (the sort is stable).  Lists where that can happen (bit set) take the O(n)-per-entry path.
//   letters         one row per output member: its output insertions in order, each its own letters followed by those that joined it.  A
//                   source insertion with letters is one RowRun (reverse-complemented by k_rows when its side is *_rc); its place in the row
//                   is a prefix sum of lengths in output order, which the host's per-member running sums (`cum`, source order) give directly
//                   on the usual path: forward cum[t], reversed cum[n] - cum[t + 1].
#pragma once
#include "../../include/pga_align.h"
#include "pga_rows.h"
#include <algorithm>

namespace pga {

typedef unsigned long long mg_u64;
constexpr uint32_t MG_NONE = 0xffffffffu;
constexpr int MG_THREADS = 256, MG_WAVES = MG_THREADS / 64;
enum { MG_SUB = 0, MG_DEL = 1, MG_INS = 2 };
// per output member: bit (side, kind) = the list does not take the usual path (see above)
constexpr uint32_t mg_bit(int side, int kind) { return 1u << (side * 3 + kind); }
constexpr uint32_t MG_SLOW_INS = mg_bit(0, MG_INS) | mg_bit(1, MG_INS);

// one side of an output member: the lists of its input member, its block's consensus length and orientation, what is added to positions
struct MgSide { uint64_t sub_off, del_off, ins_off, cum_off; uint32_t n_sub, n_del, n_ins, len, rc, shift; };
// an output member: first output substitution / deletion (host sums), first scratch entry of its right insertions, first run and first
// letter of its row of inserted letters (row_off: in out->ins_seq, a multiple of 16)
struct MgMem { MgSide s[2]; uint64_t o_sub, o_del, lead_off, run_off, row_off; uint32_t edge, pad; };
struct MgDev {
	const MgMem *mem; uint64_t n_mem;
	const pga_sub_t *subs; const pga_del_t *dels; const pga_ins_t *inss;
	const mg_u64 *cum;        // per input member n_ins + 1 entries: runs << 32 | letters of the insertions before entry t
	uint32_t *flags;          // per output member: mg_bit()s
	uint32_t *first_l;        // per output member: source index of the first left' insertion at L_left, or MG_NONE
	uint32_t *b_cnt;          // per output member: right' insertions at 0 ...
	mg_u64 *b_sum;            // ... and their runs << 32 | letters
	uint32_t *n_ins;          // per output member: output insertions
	uint32_t *lead;           // per right insertion of a slow member: its leader
	uint32_t *edge_bad;       // per edge: a substitution letter the complement table rejects
	const mg_u64 *ins_off;    // per output member: first output insertion (exclusive sums of n_ins; entry n_mem: the total)
};

__host__ __device__ inline uint32_t mg_sub_pos(uint32_t pos, uint32_t len, uint32_t rc) { return rc ? len - pos - 1u : pos; }
__host__ __device__ inline uint32_t mg_del_pos(uint32_t pos, uint32_t dlen, uint32_t len, uint32_t rc) { return rc ? len - pos - dlen : pos; }
__host__ __device__ inline uint32_t mg_ins_pos(uint32_t pos, uint32_t len, uint32_t rc) { return rc ? len - pos : pos; }
__host__ __device__ inline mg_u64 mg_pack(uint32_t len) { return len ? (1ULL << 32 | (mg_u64)len) : 0ULL; }
// whether source entry u stands before source entry t (u != t) in the primed list; ku, kt: their mapped positions
__host__ __device__ inline bool mg_before(uint32_t rc, uint32_t ku, uint32_t kt, uint32_t u, uint32_t t) { return rc ? (ku < kt || (ku == kt && u < t)) : u < t; }

template <int KIND> __device__ __forceinline__ uint32_t mg_count(const MgSide &S) { return KIND == MG_SUB ? S.n_sub : KIND == MG_DEL ? S.n_del : S.n_ins; }
// mapped position of source entry t (without the shift)
template <int KIND> __device__ __forceinline__ uint32_t mg_key(const MgDev &V, const MgSide &S, uint32_t t)
{
	if (KIND == MG_SUB) return mg_sub_pos(V.subs[S.sub_off + t].pos, S.len, S.rc);
	if (KIND == MG_DEL) { const pga_del_t d = V.dels[S.del_off + t]; return mg_del_pos(d.pos, d.len, S.len, S.rc); }
	return mg_ins_pos(V.inss[S.ins_off + t].pos, S.len, S.rc);
}
// index of source entry t in the primed list
template <int KIND> __device__ __forceinline__ uint32_t mg_dst(const MgDev &V, const MgSide &S, uint32_t t, bool slow)
{
	const uint32_t n = mg_count<KIND>(S);
	if (!S.rc) return t;
	if (!slow) return n - 1u - t;
	const uint32_t kt = mg_key<KIND>(V, S, t);
	uint32_t r = 0;
	for (uint32_t u = 0; u < n; ++u) if (u != t && mg_before(1u, mg_key<KIND>(V, S, u), kt, u, t)) ++r;
	return r;
}
// the bit of a list: *_rc: mapped positions not strictly decreasing; forward right insertions: positions not strictly increasing
template <int KIND> __device__ __forceinline__ void mg_list_bit(const MgDev &V, const MgSide &S, int side, uint64_t o, uint32_t lane)
{
	const uint32_t n = mg_count<KIND>(S);
	if (!S.rc && !(KIND == MG_INS && side == 1)) return;
	for (uint32_t t = lane; t + 1 < n; t += 64) {
		const uint32_t a = mg_key<KIND>(V, S, t), b = mg_key<KIND>(V, S, t + 1);
		if (S.rc ? a <= b : a >= b) atomicOr(&V.flags[o], mg_bit(side, KIND));
	}
}

// pass 1, one wave per output member, lanes over entries: the list bits, first_l, and what the right' insertions at 0 hold
__global__ __launch_bounds__(MG_THREADS) void k_merge_lists(MgDev V)
{
	const uint32_t lane = threadIdx.x & 63u;
	for (uint64_t o = (uint64_t)blockIdx.x * MG_WAVES + (threadIdx.x >> 6); o < V.n_mem; o += (uint64_t)gridDim.x * MG_WAVES) {
		const MgMem M = V.mem[o];
		for (int side = 0; side < 2; ++side) {
			mg_list_bit<MG_SUB>(V, M.s[side], side, o, lane);
			mg_list_bit<MG_DEL>(V, M.s[side], side, o, lane);
			mg_list_bit<MG_INS>(V, M.s[side], side, o, lane);
		}
		for (uint32_t t = lane; t < M.s[0].n_ins; t += 64) if (mg_key<MG_INS>(V, M.s[0], t) == M.s[0].len) atomicMin(&V.first_l[o], t);
		for (uint32_t t = lane; t < M.s[1].n_ins; t += 64) if (mg_key<MG_INS>(V, M.s[1], t) == 0u) {
			atomicAdd(&V.b_cnt[o], 1u);
			const mg_u64 p = mg_pack(V.inss[M.s[1].ins_off + t].len);
			if (p) atomicAdd(&V.b_sum[o], p);
		}
	}
}

// pass 2, one wave per output member: the number of output insertions; on the slow path every right insertion's leader
__global__ __launch_bounds__(MG_THREADS) void k_merge_count(MgDev V)
{
	const uint32_t lane = threadIdx.x & 63u;
	for (uint64_t o = (uint64_t)blockIdx.x * MG_WAVES + (threadIdx.x >> 6); o < V.n_mem; o += (uint64_t)gridDim.x * MG_WAVES) {
		const MgMem M = V.mem[o];
		const MgSide &R = M.s[1];
		const bool has_l = V.first_l[o] != MG_NONE;
		if (!(V.flags[o] & MG_SLOW_INS)) {                                       // (no two right' insertions share a position: at most one at 0)
			if (lane == 0) V.n_ins[o] = M.s[0].n_ins + R.n_ins - ((has_l && V.b_cnt[o]) ? 1u : 0u);
			continue;
		}
		if (lane == 0) atomicAdd(&V.n_ins[o], M.s[0].n_ins);
		for (uint32_t t = lane; t < R.n_ins; t += 64) {
			const uint32_t pt = V.inss[R.ins_off + t].pos;
			uint32_t l = t;
			for (uint32_t u = 0; u < t; ++u) if (V.inss[R.ins_off + u].pos == pt) { l = u; break; }
			V.lead[M.lead_off + t] = l;
			if (l == t && !(has_l && mg_ins_pos(pt, R.len, R.rc) == 0u)) atomicAdd(&V.n_ins[o], 1u);
		}
	}
}

// index in the primed list and runs << 32 | letters before source insertion t of side S (without what joins first_l)
__device__ __forceinline__ void mg_ins_before(const MgDev &V, const MgSide &S, uint32_t t, bool slow, uint32_t &idx, mg_u64 &sum)
{
	const mg_u64 *cum = V.cum + S.cum_off;
	if (!slow) {
		if (!S.rc) { idx = t; sum = cum[t]; }
		else { idx = S.n_ins - 1u - t; sum = cum[S.n_ins] - cum[t + 1]; }
		return;
	}
	const uint32_t kt = mg_key<MG_INS>(V, S, t);
	idx = 0; sum = 0;
	for (uint32_t u = 0; u < S.n_ins; ++u) if (u != t && mg_before(S.rc, mg_key<MG_INS>(V, S, u), kt, u, t)) { ++idx; sum += mg_pack(V.inss[S.ins_off + u].len); }
}

template <int KIND, class Put> __device__ __forceinline__ void mg_write_list(const MgDev &V, const MgMem &M, uint64_t o, uint32_t lane, Put put)
{
	for (int side = 0; side < 2; ++side) {
		const MgSide &S = M.s[side];
		const bool slow = (V.flags[o] & mg_bit(side, KIND)) != 0u;
		const uint32_t n = mg_count<KIND>(S), first = side ? mg_count<KIND>(M.s[0]) : 0u;
		for (uint32_t t = lane; t < n; t += 64) put(S, t, first + mg_dst<KIND>(V, S, t, slow));
	}
}

// pass 3 (behind the scan of n_ins), one wave per output member, lanes over SOURCE entries: every entry computes its own place
__global__ __launch_bounds__(MG_THREADS) void k_merge_write(MgDev V, pga_sub_t *o_subs, pga_del_t *o_dels, pga_ins_t *o_inss, RowRun *runs)
{
	const uint32_t lane = threadIdx.x & 63u;
	for (uint64_t o = (uint64_t)blockIdx.x * MG_WAVES + (threadIdx.x >> 6); o < V.n_mem; o += (uint64_t)gridDim.x * MG_WAVES) {
		const MgMem M = V.mem[o];
		mg_write_list<MG_SUB>(V, M, o, lane, [&](const MgSide &S, uint32_t t, uint32_t at) {
			const pga_sub_t x = V.subs[S.sub_off + t];
			uint32_t alt = x.alt;
			if (S.rc) { const uint32_t c = d_comp.t[alt & 255u]; if (c) alt = c; else atomicOr(&V.edge_bad[M.edge], 1u); }
			o_subs[M.o_sub + at] = pga_sub_t{mg_sub_pos(x.pos, S.len, S.rc) + S.shift, alt};
		});
		mg_write_list<MG_DEL>(V, M, o, lane, [&](const MgSide &S, uint32_t t, uint32_t at) {
			const pga_del_t x = V.dels[S.del_off + t];
			o_dels[M.o_del + at] = pga_del_t{mg_del_pos(x.pos, x.len, S.len, S.rc) + S.shift, x.len};
		});
		// ---- insertions ----
		const MgSide &L = M.s[0], &R = M.s[1];
		const uint32_t fl = V.flags[o], f = V.first_l[o];
		const bool slow = (fl & MG_SLOW_INS) != 0u, has_l = f != MG_NONE;
		const mg_u64 B = has_l ? V.b_sum[o] : 0ULL;                              // what joins first_l
		const uint32_t b_cnt = has_l ? V.b_cnt[o] : 0u;
		const mg_u64 at0 = V.ins_off[o], l_tot = V.cum[L.cum_off + L.n_ins];
		const uint32_t kind_l = 1u | (L.rc ? ROW_REV : 0u), kind_r = 1u | (R.rc ? ROW_REV : 0u);
		const uint32_t kf = has_l ? L.len : 0u;                                  // (the mapped position of first_l)
		for (uint32_t t = lane; t < L.n_ins; t += 64) {
			const pga_ins_t x = V.inss[L.ins_off + t];
			const uint32_t kt = mg_ins_pos(x.pos, L.len, L.rc);
			uint32_t idx; mg_u64 sum;
			mg_ins_before(V, L, t, slow, idx, sum);
			if (has_l && t != f && mg_before(L.rc, kf, kt, f, t)) sum += B;
			const uint32_t off = (uint32_t)sum;
			o_inss[at0 + idx] = pga_ins_t{kt, x.len + (t == f ? (uint32_t)B : 0u), M.row_off + off};
			if (x.len) runs[M.run_off + (sum >> 32)] = RowRun{off, kind_l, x.seq_off};
		}
		for (uint32_t t = lane; t < R.n_ins; t += 64) {
			const pga_ins_t x = V.inss[R.ins_off + t];
			const uint32_t kt = mg_ins_pos(x.pos, R.len, R.rc);
			if (has_l && kt == 0u) {                                              // joins first_l: behind its letters and the earlier ones at 0
				uint32_t idx; mg_u64 sum;
				mg_ins_before(V, L, f, slow, idx, sum);
				sum += mg_pack(V.inss[L.ins_off + f].len);
				if (b_cnt > 1u) for (uint32_t u = 0; u < t; ++u) { const pga_ins_t y = V.inss[R.ins_off + u]; if (mg_ins_pos(y.pos, R.len, R.rc) == 0u) sum += mg_pack(y.len); }
				if (x.len) runs[M.run_off + (sum >> 32)] = RowRun{(uint32_t)sum, kind_r, x.seq_off};
				continue;
			}
			uint32_t idx, glen = x.len; mg_u64 sum; bool leader = true;
			if (!slow) {
				mg_ins_before(V, R, t, false, idx, sum);                            // (a right' insertion at 0 is right'[0]: its letters are in `sum`)
				idx -= b_cnt ? 1u : 0u;
				sum += l_tot;
			} else {
				const uint32_t lt = V.lead[M.lead_off + t];
				leader = lt == t;
				idx = 0; sum = l_tot + B; glen = 0;
				for (uint32_t u = 0; u < R.n_ins; ++u) {
					const pga_ins_t y = V.inss[R.ins_off + u];
					const uint32_t ku = mg_ins_pos(y.pos, R.len, R.rc);
					if (has_l && ku == 0u) continue;                                  // (joined first_l: counted in B)
					if (ku == kt) { glen += y.len; if (u < t) sum += mg_pack(y.len); continue; }
					const uint32_t lu = V.lead[M.lead_off + u];
					if (R.rc ? ku < kt : lu < lt) { sum += mg_pack(y.len); if (lu == u) ++idx; }
				}
			}
			const uint32_t off = (uint32_t)sum;
			if (leader) o_inss[at0 + L.n_ins + idx] = pga_ins_t{kt + R.shift, glen, M.row_off + off};
			if (x.len) runs[M.run_off + (sum >> 32)] = RowRun{off, kind_r, x.seq_off};
		}
	}
}

// ---------------------------------------------------------------- host side: validation of the edges and the tables
struct MgTables {
	std::vector<MgMem> mem; std::vector<mg_u64> cum;
	std::vector<RowJob> jobs; std::vector<uint32_t> job_edge;             // consensus rows first, then the rows of inserted letters
	std::vector<RowRun> cons_runs;                                        // the runs of the consensus rows; the others are built on the device behind them
	std::vector<char> cons; std::vector<uint64_t> cons_off, member_off;   // per edge: its consensus in out->cons, its first output member
	uint64_t cons_units = 0, units = 0, n_runs = 0, n_lead = 0, n_sub = 0, n_del = 0, ins_lo = UINT64_MAX, ins_hi = 0;
};

// G: row_graph_init (aligned: the lists are checked, nothing is prepared).  Throws std::runtime_error on what fails the call.
static void mg_build_tables(const RowGraph &G, int64_t n_edges, const pga_merge_edge_t *edges, const uint32_t *partner, MgTables &T)
{
	auto fail = [](const std::string &what) { throw std::runtime_error("pga_merge_blocks: " + what); };
	if (n_edges < 0 || (n_edges && !edges)) fail("null argument");
	if (n_edges >= (1LL << 32)) fail("more than 2^32 edges");
	const uint64_t n_mem_in = G.n_mem;
	// running sums of every input member's insertion lengths, source order
	T.cum.assign((size_t)(G.ins_off[n_mem_in] + n_mem_in), 0);
	for (uint64_t m = 0; m < n_mem_in; ++m) {
		mg_u64 run = 0;
		const uint64_t c0 = G.ins_off[m] + m;
		T.cum[c0] = 0;
		for (uint64_t t = G.ins_off[m]; t < G.ins_off[m + 1]; ++t) {
			if (G.inss[t].len && !G.ins_seq) fail("null insertion letters with a non-zero length (member " + std::to_string(m) + ")");
			run += mg_pack(G.inss[t].len);
			if ((uint32_t)run > (1u << 30)) fail("more than 2^30 inserted letters in one member (member " + std::to_string(m) + ")");
			T.cum[c0 + (t - G.ins_off[m]) + 1] = run;
		}
	}
	std::unordered_map<uint32_t, uint64_t> cons_at;
	auto place_cons = [&](uint32_t b) {
		auto ins = cons_at.emplace(b, (uint64_t)T.cons.size());
		if (ins.second) T.cons.insert(T.cons.end(), G.blocks[b].consensus, G.blocks[b].consensus + G.blocks[b].cons_len);
		return ins.first->second;
	};
	T.cons_off.assign((size_t)n_edges, 0); T.member_off.assign((size_t)n_edges + 1, 0);
	uint64_t p0 = 0;
	std::vector<uint8_t> seen;
	std::vector<RowJob> ins_jobs; std::vector<uint32_t> ins_job_edge;
	uint64_t ins_units = 0;
	for (int64_t e = 0; e < n_edges; ++e) {
		const pga_merge_edge_t &E = edges[e];
		const std::string who = " (edge " + std::to_string(e) + ")";
		if (E.left >= (uint64_t)G.n_blocks || E.right >= (uint64_t)G.n_blocks) fail("edge names a block that does not exist" + who);
		const pga_rc_block_t &BL = G.blocks[E.left], &BR = G.blocks[E.right];
		if (BL.n_members != BR.n_members) fail("the two blocks differ in depth" + who);
		if ((uint64_t)BL.cons_len + BR.cons_len >= (1ULL << 30)) fail("merged consensus of 2^30 letters or more" + who);
		const uint32_t depth = BL.n_members;
		if (depth && !partner) fail("null partner list");
		seen.assign(depth, 0);
		for (uint32_t k = 0; k < depth; ++k) {
			const uint32_t q = partner[p0 + k];
			if (q >= depth || seen[q]) fail("partner is no permutation of the right block's members" + who);
			seen[q] = 1;
		}
		// the consensus row: left' then right'
		const uint32_t len = BL.cons_len + BR.cons_len;
		T.cons_off[e] = T.cons_units * ROW_LETTERS;
		if (len) {
			const uint64_t r0 = T.cons_runs.size();
			if (BL.cons_len) T.cons_runs.push_back(RowRun{0u, E.left_rc ? ROW_REV : 0u, place_cons(E.left)});
			if (BR.cons_len) T.cons_runs.push_back(RowRun{BL.cons_len, E.right_rc ? ROW_REV : 0u, place_cons(E.right)});
			T.jobs.push_back(RowJob{r0, T.cons_units, (uint32_t)(T.cons_runs.size() - r0), len, 0u, 0u});
			T.job_edge.push_back((uint32_t)e);
			T.cons_units += row_pad(len) / ROW_LETTERS;
		}
		for (uint32_t k = 0; k < depth; ++k) {
			const uint64_t ml = G.mem_first[E.left] + k, mr = G.mem_first[E.right] + partner[p0 + k];
			MgMem M;
			memset(&M, 0, sizeof(M));
			const uint64_t mm[2] = {ml, mr};
			for (int s = 0; s < 2; ++s) {
				const uint64_t m = mm[s];
				M.s[s] = MgSide{G.sub_off[m], G.del_off[m], G.ins_off[m], G.ins_off[m] + m, G.members[m].n_subs, G.members[m].n_dels, G.members[m].n_inss,
				                s ? BR.cons_len : BL.cons_len, (uint32_t)((s ? E.right_rc : E.left_rc) ? 1 : 0), s ? BL.cons_len : 0u};
				for (uint64_t t = G.ins_off[m]; t < G.ins_off[m + 1]; ++t) if (G.inss[t].len) { T.ins_lo = std::min<uint64_t>(T.ins_lo, G.inss[t].seq_off); T.ins_hi = std::max<uint64_t>(T.ins_hi, G.inss[t].seq_off + G.inss[t].len); }
			}
			if ((uint64_t)M.s[0].n_sub + M.s[1].n_sub >= (1ULL << 32) || (uint64_t)M.s[0].n_del + M.s[1].n_del >= (1ULL << 32) || (uint64_t)M.s[0].n_ins + M.s[1].n_ins >= (1ULL << 32))
				fail("more than 2^32 edits of one kind in one merged member" + who);
			const mg_u64 tot = T.cum[M.s[0].cum_off + M.s[0].n_ins] + T.cum[M.s[1].cum_off + M.s[1].n_ins];
			M.o_sub = T.n_sub; M.o_del = T.n_del; M.lead_off = T.n_lead; M.run_off = T.n_runs; M.row_off = ins_units * ROW_LETTERS; M.edge = (uint32_t)e;
			T.n_sub += (uint64_t)M.s[0].n_sub + M.s[1].n_sub; T.n_del += (uint64_t)M.s[0].n_del + M.s[1].n_del; T.n_lead += M.s[1].n_ins;
			if ((uint32_t)tot) {
				ins_jobs.push_back(RowJob{M.run_off, ins_units, (uint32_t)(tot >> 32), (uint32_t)tot, 0u, 0u});
				ins_job_edge.push_back((uint32_t)e);
				ins_units += row_pad((uint32_t)tot) / ROW_LETTERS;
				T.n_runs += tot >> 32;
			}
			T.mem.push_back(M);
		}
		p0 += depth;
		T.member_off[e + 1] = T.member_off[e] + depth;
	}
	// one unit space and one run array: the consensus rows, then the rows of inserted letters
	for (size_t j = 0; j < ins_jobs.size(); ++j) { RowJob J = ins_jobs[j]; J.run_off += T.cons_runs.size(); J.unit0 += T.cons_units; T.jobs.push_back(J); T.job_edge.push_back(ins_job_edge[j]); }
	for (MgMem &M : T.mem) M.run_off += T.cons_runs.size();
	T.n_runs += T.cons_runs.size();
	T.units = T.cons_units + ins_units;
	if (T.jobs.size() >= (1ULL << 31)) fail("more than 2^31 rows");
}

} // namespace pga
