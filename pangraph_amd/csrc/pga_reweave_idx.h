// pga_reweave_idx.h -- the list kernels and host tables of pga_reweave.hip (the front half of reweave: reweave.rs:132-340 over
// pangraph_interval.rs:98-255 and cigar.rs:26-96).  None of it uses a wave intrinsic, so all of this compiles under hipcc and, with
// dev/emu/hip_emu.h included first, under g++ -std=c++17 -DPGA_EMU (tests/emu/reweave_emu.cpp runs it against a direct scalar construction).
// The sorts and the scans between the kernels are rocPRIM's (pga_reweave.hip) and are not in here.
//
// A SIDE of match m is 2m + s, s = 0 the ref hit, s = 1 the qry hit (the values of pga_plan_match_t.anchor).  A HIT is a side; the sorted
// hit list hs[] holds sides by (rank of the block in the output order, start).  Every rule of create_intervals / refine_intervals looks one
// step left and right only, so a hit decides for itself, from the hit before and the hit behind it on the same block:
//   gap_l      the gap in front of it (it OWNS that gap; the last hit of a block also owns the trailing gap)
//   ext_l      gap_l when that gap is short and joins this hit (left_len < right_len), ext_r the gap behind it that joins this hit
//   before / after   the intervals it owns in the unrefined and in the refined list
// Two short gaps are never adjacent and a short gap's neighbours are aligned, so the merges of refine_intervals do not interact.
#pragma once
#ifndef PGA_EMU
#include "pga_common.h"
#endif
#include "../../include/pga_align.h"
#include "pga_xxh64.h"
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

namespace pga {

typedef unsigned long long rw_u64;
constexpr int RW_THREADS = 256, RW_WAVES = RW_THREADS / 64;
constexpr uint32_t RW_MAX_LEN = 1u << 28;                       // an operation length lives in 28 bits
enum { RW_ERR_OVERLAP = 1, RW_ERR_DUP_ID = 2, RW_ERR_OP_LEN = 3, RW_ERR_OP_KIND = 4 };
enum { RW_C_DEPTH = 0, RW_C_MASK = 1, RW_C_LETTERS = 2, RW_C_UNDECIDED = 3, RW_C_FAILED = 4, RW_COUNTERS = 5 };
constexpr uint32_t RW_OP_M = 0, RW_OP_I = 1, RW_OP_D = 2, RW_OP_EQ = 7, RW_OP_X = 8;

struct RwBlk { uint64_t block_id; const uint16_t *nmask; uint64_t nm_pos; uint32_t cons_len, depth, ord, hb; };   // ord: rank in the output order; hb: index among the blocks with a hit
struct RwMatch { uint64_t cigar_off; uint32_t blk[2], start[2], end[2]; uint32_t n_cigar, reverse, group, letters; };   // [0] ref, [1] qry; letters: ncnt holds letter counts
struct RwJob { uint64_t off; uint32_t side, len; };             // letters route: `len` letters of side `side` at stage[off ..), off a multiple of 16
struct alignas(16) RwV4 { uint32_t w[4]; };
struct RwExt { uint32_t left, right; };
struct RwPlan { uint32_t front[2], back[2], mod_idx[4], mod_add[4], nf, nb; };   // what update_cigar does to a promise's base CIGAR: operations in front and behind, lengthened base operations (idx ~0: none)

struct RwDev {
	uint64_t n_matches, n_hits, n_hb, cap_iv, cap_cig; uint32_t thr_len, pad;
	const RwBlk *blk; const RwMatch *mt; const uint32_t *cig;
	uint32_t *ncnt;                          // per side: set bits of the bit plane, or letters equal to 'N'
	pga_plan_match_t *o_match;
	rw_u64 *hkey; uint32_t *hval;            // per side: (ord << 32 | start, side), unsorted
	rw_u64 *pkey; uint32_t *pval, *pgrp;     // per match: (new_block_id, match); the group of the match at rank i of the id sort
	const uint32_t *hs;                      // sorted sides
	uint32_t *cnt_b, *cnt_a, *herr;          // per sorted hit (n_hits + 1 entries, the last 0): intervals owned before / after refinement; code | local index << 8
	const uint32_t *off_b, *off_a;           // their exclusive sums
	RwExt *ext;                              // per side
	rw_u64 *iv_of;                           // per side: its aligned interval in intervals[]
	rw_u64 *b_first, *b_firstb, *b_end, *b_err;   // per hit block: first refined / unrefined interval, end, min(global unrefined index << 8 | code)
	pga_plan_block_res_t *o_blk; pga_plan_interval_t *o_iv; pga_slice_interval_t *o_siv;
	const uint32_t *pm;                      // promises: matches by (group, new_block_id)
	RwPlan *plan; rw_u64 *n_out; const rw_u64 *c_off;   // per promise (n_out, c_off: n + 1 entries)
	pga_plan_promise_t *o_prom; uint32_t *o_cig;
	rw_u64 *counters; uint32_t *err;         // RW_COUNTERS sums; [0] code, [1..2] where
};

__device__ inline void rw_fail(const RwDev &V, uint32_t code, uint64_t where)
{
#ifdef PGA_EMU
	if (V.err[0] == 0u) { V.err[0] = code; V.err[1] = (uint32_t)(where & 0xffffffffu); V.err[2] = (uint32_t)(where >> 32); }
#else
	if (atomicCAS(&V.err[0], 0u, code) == 0u) { V.err[1] = (uint32_t)(where & 0xffffffffu); V.err[2] = (uint32_t)(where >> 32); }
#endif
}
__host__ __device__ inline uint32_t rw_popc(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return (uint32_t)__popc(x);
#else
	return (uint32_t)__builtin_popcount(x);
#endif
}

// ---------------------------------------------------------------- the ids: XXH64 (pga_xxh64.h) of six and of three words
__host__ __device__ inline uint64_t rw_match_id(uint64_t q_id, uint32_t qs, uint32_t qe, uint64_t r_id, uint32_t rs, uint32_t re)
{
	const uint64_t w[6] = {q_id, qs, qe, r_id, rs, re};
	return xxh64_words(w, 6);
}
__host__ __device__ inline uint64_t rw_gap_id(uint64_t block_id, uint32_t start, uint32_t end)
{
	const uint64_t w[3] = {block_id, start, end};
	return xxh64_words(w, 3);
}

// ---------------------------------------------------------------- the N counts, one wave per side
// the mask route: the set bits of the 16-bit words that hold bases [a, b) of the packed store, the two edge words masked.  The sum goes
// through the wave's LDS word; every wave of a workgroup takes the same number of turns, so the barriers are reached by all of them.
__global__ __launch_bounds__(RW_THREADS) void k_rw_mask(RwDev V, const uint32_t *sides, uint64_t n)
{
	__shared__ uint32_t s_sum[RW_WAVES];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (uint64_t j0 = (uint64_t)blockIdx.x * RW_WAVES; j0 < n; j0 += (uint64_t)gridDim.x * RW_WAVES) {
		const uint64_t j = j0 + wave;
		if (lane == 0) s_sum[wave] = 0;
		__syncthreads();
		uint32_t side = 0;
		if (j < n) {
			side = sides[j];
			const RwMatch &M = V.mt[side >> 1]; const RwBlk B = V.blk[M.blk[side & 1]];
			const uint64_t a = B.nm_pos + M.start[side & 1], b = B.nm_pos + M.end[side & 1];      // (a < b: checked by the host)
			const uint64_t w0 = a >> 4, w1 = (b - 1) >> 4;
			uint32_t part = 0;
			for (uint64_t w = w0 + lane; w <= w1; w += 64) {
				uint32_t x = B.nmask[w];
				if (w == w0) x &= 0xffffu << (uint32_t)(a & 15);
				if (w == w1) x &= 0xffffu >> (15u - (uint32_t)((b - 1) & 15));
				part += rw_popc(x & 0xffffu);
			}
			if (part) atomicAdd(&s_sum[wave], part);
		}
		__syncthreads();
		if (j < n && lane == 0) V.ncnt[side] = s_sum[wave];
	}
}
// bytes equal to 'N' among the 4 of a word: 0x80 where a byte of x is zero, exactly (no borrow between bytes)
__host__ __device__ inline uint32_t rw_count_n(uint32_t w)
{
	const uint32_t x = w ^ 0x4E4E4E4Eu;
	return rw_popc(~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu));
}
// the letters route: 16 letters per lane and turn from the staging buffer (every job starts at a multiple of 16 and the buffer is padded to
// one); the letters behind the job's last are cleared before they are compared
__global__ __launch_bounds__(RW_THREADS) void k_rw_letters(RwDev V, const RwJob *jobs, uint64_t n, const RwV4 *stage)
{
	__shared__ uint32_t s_sum[RW_WAVES];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (uint64_t j0 = (uint64_t)blockIdx.x * RW_WAVES; j0 < n; j0 += (uint64_t)gridDim.x * RW_WAVES) {
		const uint64_t j = j0 + wave;
		if (lane == 0) s_sum[wave] = 0;
		__syncthreads();
		RwJob J{0, 0, 0};
		if (j < n) {
			J = jobs[j];
			const RwV4 *src = stage + (J.off >> 4);
			const uint32_t n16 = (J.len + 15u) >> 4;
			uint32_t part = 0;
			for (uint32_t t = lane; t < n16; t += 64) {
				RwV4 v = src[t];
				const uint32_t have = J.len - t * 16u;               // letters of this turn that belong to the job (>= 1)
#pragma unroll
				for (uint32_t k = 0; k < 4; ++k) {
					const uint32_t lo = 4u * k, w = have <= lo ? 0u : have >= lo + 4u ? v.w[k] : v.w[k] & (0xffffffffu >> (8u * (lo + 4u - have)));
					part += rw_count_n(w);
				}
			}
			if (part) atomicAdd(&s_sum[wave], part);
		}
		__syncthreads();
		if (j < n && lane == 0) V.ncnt[J.side] = s_sum[wave];
	}
}

// ---------------------------------------------------------------- per match: anchor, route, id, the two hit keys, the promise key
__global__ __launch_bounds__(RW_THREADS) void k_rw_match(RwDev V)
{
	for (uint64_t m = (uint64_t)blockIdx.x * RW_THREADS + threadIdx.x; m < V.n_matches; m += (uint64_t)gridDim.x * RW_THREADS) {
		const RwMatch M = V.mt[m]; const RwBlk R = V.blk[M.blk[0]], Q = V.blk[M.blk[1]];
		pga_plan_match_t O;
		O.new_block_id = rw_match_id(Q.block_id, M.start[1], M.end[1], R.block_id, M.start[0], M.end[0]);
		O.ref_n = O.qry_n = 0;
		if (R.depth != Q.depth) { O.anchor = R.depth > Q.depth ? 0 : 1; O.route = 0; atomicAdd(&V.counters[RW_C_DEPTH], (rw_u64)1); }
		else {
			const uint32_t rn = V.ncnt[2 * m], qn = V.ncnt[2 * m + 1];
			if (M.letters) { O.ref_n = rn; O.qry_n = qn; O.anchor = rn <= qn ? 0 : 1; O.route = 2; atomicAdd(&V.counters[RW_C_LETTERS], (rw_u64)1); }
			else {
				O.anchor = 0; O.route = 1;
				if (rn | qn) atomicAdd(&V.counters[RW_C_UNDECIDED], (rw_u64)1);          // (the bit plane is an upper bound only: the host sends letters and asks again)
				else atomicAdd(&V.counters[RW_C_MASK], (rw_u64)1);
			}
		}
		V.o_match[m] = O;
		V.hkey[2 * m] = (rw_u64)R.ord << 32 | M.start[0]; V.hval[2 * m] = (uint32_t)(2 * m);
		V.hkey[2 * m + 1] = (rw_u64)Q.ord << 32 | M.start[1]; V.hval[2 * m + 1] = (uint32_t)(2 * m + 1);
		V.pkey[m] = O.new_block_id; V.pval[m] = (uint32_t)m;
	}
}
// the group of the match at every rank of the id sort (the key of the second, stable sort)
__global__ __launch_bounds__(RW_THREADS) void k_rw_groups(RwDev V, const uint32_t *by_id)
{
	for (uint64_t i = (uint64_t)blockIdx.x * RW_THREADS + threadIdx.x; i < V.n_matches; i += (uint64_t)gridDim.x * RW_THREADS) V.pgrp[i] = V.mt[by_id[i]].group;
}

// ---------------------------------------------------------------- per sorted hit: what it owns, its extensions, its first error
struct RwHit { uint32_t blk, start, end; };
__device__ inline RwHit rw_hit(const RwDev &V, uint32_t side) { const RwMatch &M = V.mt[side >> 1]; return RwHit{M.blk[side & 1], M.start[side & 1], M.end[side & 1]}; }
struct RwOwn { uint32_t gap_l, trail, ext_l, ext_r; bool keep_l, keep_t; };
__device__ inline RwOwn rw_own(const RwDev &V, uint64_t h, const RwHit &X, uint32_t &code, uint32_t &at)
{
	const uint32_t thr = V.thr_len, cons_len = V.blk[X.blk].cons_len, L = X.end - X.start;
	bool prev = false, next = false; RwHit P{0, 0, 0}, N{0, 0, 0};
	if (h > 0) { P = rw_hit(V, V.hs[h - 1]); prev = P.blk == X.blk; }
	if (h + 1 < V.n_hits) { N = rw_hit(V, V.hs[h + 1]); next = N.blk == X.blk; }
	if (prev && X.start < P.end) rw_fail(V, RW_ERR_OVERLAP, h);
	RwOwn O;
	const uint32_t cursor = prev ? P.end : 0u, left_len = prev ? P.end - P.start : 0u;
	O.gap_l = X.start > cursor ? X.start - cursor : 0u;
	O.trail = next ? 0u : cons_len - X.end;
	const bool short_l = O.gap_l > 0 && O.gap_l < thr, short_t = O.trail > 0 && O.trail < thr;
	O.ext_l = short_l && left_len < L ? O.gap_l : 0u;                            // (left_len >= right_len: it joins the hit before)
	O.ext_r = short_t ? O.trail : 0u;
	if (next) { const uint32_t ga = N.start > X.end ? N.start - X.end : 0u; if (ga > 0 && ga < thr && L >= N.end - N.start) O.ext_r = ga; }
	O.keep_l = O.gap_l > 0 && !short_l; O.keep_t = O.trail > 0 && !short_t;
	// check_interval_conditions, over the gap in front, the hit, the trailing gap: the first that fails
	code = 0; at = 0;
	if (short_l && prev && left_len < thr) code = 3;
	else if (short_l && L < thr) code = 5;
	else if (L < thr) { code = 1; at = O.gap_l > 0 ? 1u : 0u; }
	else if (short_t && L < thr) { code = 3; at = (O.gap_l > 0 ? 1u : 0u) + 1u; }    // (unreachable: the hit itself fails first; kept for the order of the reference)
	return O;
}
__global__ __launch_bounds__(RW_THREADS) void k_rw_hits(RwDev V)
{
	for (uint64_t h = (uint64_t)blockIdx.x * RW_THREADS + threadIdx.x; h <= V.n_hits; h += (uint64_t)gridDim.x * RW_THREADS) {
		if (h == V.n_hits) { V.cnt_b[h] = 0; V.cnt_a[h] = 0; V.herr[h] = 0; continue; }
		const uint32_t side = V.hs[h];
		const RwHit X = rw_hit(V, side);
		uint32_t code, at;
		const RwOwn O = rw_own(V, h, X, code, at);
		V.cnt_b[h] = (O.gap_l > 0 ? 1u : 0u) + 1u + (O.trail > 0 ? 1u : 0u);
		V.cnt_a[h] = (O.keep_l ? 1u : 0u) + 1u + (O.keep_t ? 1u : 0u);
		V.herr[h] = code | at << 8;
		V.ext[side] = RwExt{O.ext_l, O.ext_r};
	}
}
// behind the two scans: the refined intervals of every hit in their places, the block table's ends, the first error of every block
__global__ __launch_bounds__(RW_THREADS) void k_rw_intervals(RwDev V)
{
	for (uint64_t h = (uint64_t)blockIdx.x * RW_THREADS + threadIdx.x; h < V.n_hits; h += (uint64_t)gridDim.x * RW_THREADS) {
		const uint32_t side = V.hs[h];
		const uint64_t m = side >> 1;
		const RwHit X = rw_hit(V, side);
		const RwBlk B = V.blk[X.blk];
		uint32_t code, at;
		const RwOwn O = rw_own(V, h, X, code, at);
		const bool head = h == 0 || rw_hit(V, V.hs[h - 1]).blk != X.blk, tail = h + 1 == V.n_hits || rw_hit(V, V.hs[h + 1]).blk != X.blk;
		uint64_t k = V.off_a[h];
		if (head) { V.b_first[B.hb] = k; V.b_firstb[B.hb] = V.off_b[h]; }
		if (tail) V.b_end[B.hb] = k + V.cnt_a[h];
		if (code) atomicMin(&V.b_err[B.hb], ((rw_u64)V.off_b[h] + at) << 8 | code);
		const pga_plan_match_t Mt = V.o_match[m];
		const RwMatch &M = V.mt[m];
		if (O.keep_l && k < V.cap_iv) {
			const uint32_t s = X.start - O.gap_l;
			V.o_iv[k] = pga_plan_interval_t{rw_gap_id(B.block_id, s, X.start), -1, s, X.start, 0, 0, 0, 0u, 0u, 0u};
			V.o_siv[k] = pga_slice_interval_t{s, X.start, 0};
			++k;
		}
		if (k < V.cap_iv) {
			const int32_t is_anchor = Mt.anchor == (int32_t)(side & 1) ? 1 : 0, rev = M.reverse ? 1 : 0;
			V.o_iv[k] = pga_plan_interval_t{Mt.new_block_id, (int64_t)m, X.start - O.ext_l, X.end + O.ext_r, 1, is_anchor, rev, O.ext_l, O.ext_r, 0u};
			V.o_siv[k] = pga_slice_interval_t{X.start - O.ext_l, X.end + O.ext_r, !is_anchor && rev ? 1 : 0};
			V.iv_of[side] = k;
			++k;
		}
		if (O.keep_t && k < V.cap_iv) {
			V.o_iv[k] = pga_plan_interval_t{rw_gap_id(B.block_id, X.end, B.cons_len), -1, X.end, B.cons_len, 0, 0, 0, 0u, 0u, 0u};
			V.o_siv[k] = pga_slice_interval_t{X.end, B.cons_len, 0};
		}
	}
}
// per block with a hit: its record (`block` is the host's)
__global__ __launch_bounds__(RW_THREADS) void k_rw_blocks(RwDev V)
{
	for (uint64_t b = (uint64_t)blockIdx.x * RW_THREADS + threadIdx.x; b < V.n_hb; b += (uint64_t)gridDim.x * RW_THREADS) {
		const rw_u64 e = V.b_err[b];
		pga_plan_block_res_t O;
		O.first_interval = V.b_first[b]; O.n_intervals = (uint32_t)(V.b_end[b] - V.b_first[b]); O.block = 0; O.pad = 0;
		if (e == ~0ULL) { O.status = 0; O.fail_interval = -1; }
		else { O.status = (int32_t)(e & 0xffu); O.fail_interval = (int64_t)((e >> 8) - V.b_firstb[b]); atomicAdd(&V.counters[RW_C_FAILED], (rw_u64)1); }
		V.o_blk[b] = O;
	}
}

// ---------------------------------------------------------------- the promise CIGARs
__host__ __device__ inline bool rw_is_match(uint32_t op) { return op == RW_OP_M || op == RW_OP_EQ || op == RW_OP_X; }
// operation i of the anchor's CIGAR (extract_hits): the match's own for a ref-side anchor; for a qry-side one reversed when the match is
// reverse, then I <-> D
__host__ __device__ inline uint32_t rw_base_op(const uint32_t *cig, uint32_t n, uint32_t anchor, uint32_t reverse, uint32_t i)
{
	if (!anchor) return cig[i];
	const uint32_t w = cig[reverse ? n - 1u - i : i], op = w & 15u;
	return op == RW_OP_I ? (w & ~15u) | RW_OP_D : op == RW_OP_D ? (w & ~15u) | RW_OP_I : w;
}
// add_flanking_indel on the planned CIGAR  front[0 .. nf) ++ base (+ mods) ++ back[0 .. nb): the walk from one end meets the inserted
// operations of that end, then the base up to its first M, and only when the base has no M at all the inserted operations of the other end.
// The last operation of `kind` it meets is lengthened; otherwise one is inserted at the very end of that side.  `step` (0 .. 3, a literal at
// every call) is the slot of a lengthened base operation: no array of the plan is indexed by a run-time value.
// lead_last / trail_last: the base operation of `kind` a leading / trailing walk meets last, or -1.  Returns false when a length reaches 2^28.
__host__ __device__ inline bool rw_lengthen(uint32_t &w, uint32_t add) { if ((w >> 4) + add >= RW_MAX_LEN) return false; w += add << 4; return true; }
__host__ __device__ inline bool rw_add_flank(RwPlan &P, const uint32_t *cig, uint32_t n, uint32_t anchor, uint32_t reverse, bool has_m, int64_t lead_last, int64_t trail_last,
                                             uint32_t kind, uint32_t add, bool leading, int step)
{
	if (add == 0) return true;
	if (add >= RW_MAX_LEN) return false;
	const bool f0 = P.nf >= 1 && (P.front[0] & 15u) == kind, f1 = P.nf == 2 && (P.front[1] & 15u) == kind;
	const bool b0 = P.nb >= 1 && (P.back[0] & 15u) == kind, b1 = P.nb == 2 && (P.back[1] & 15u) == kind;
	const int64_t at = leading ? lead_last : trail_last;
	if (leading) {
		if (!has_m && b1) return rw_lengthen(P.back[1], add);
		if (!has_m && b0) return rw_lengthen(P.back[0], add);
		if (at < 0 && f1) return rw_lengthen(P.front[1], add);
		if (at < 0 && f0) return rw_lengthen(P.front[0], add);
	} else {
		if (!has_m && f0) return rw_lengthen(P.front[0], add);
		if (!has_m && f1) return rw_lengthen(P.front[1], add);
		if (at < 0 && b0) return rw_lengthen(P.back[0], add);
		if (at < 0 && b1) return rw_lengthen(P.back[1], add);
	}
	if (at >= 0) {
		uint32_t len = rw_base_op(cig, n, anchor, reverse, (uint32_t)at) >> 4;
#pragma unroll
		for (int k = 0; k < 4; ++k) if (P.mod_idx[k] == (uint32_t)at) len += P.mod_add[k];
		if (len + add >= RW_MAX_LEN) return false;
		P.mod_idx[step] = (uint32_t)at; P.mod_add[step] = add;
		return true;
	}
	if (leading) { P.front[1] = P.front[0]; P.front[0] = add << 4 | kind; ++P.nf; }
	else { if (P.nb == 0) P.back[0] = add << 4 | kind; else P.back[1] = add << 4 | kind; ++P.nb; }
	return true;
}
// one thread per promise: update_cigar as a plan (reweave.rs:271-304), the output length, the duplicate-id check on the sorted list
__global__ __launch_bounds__(RW_THREADS) void k_rw_cigar_plan(RwDev V)
{
	for (uint64_t p = (uint64_t)blockIdx.x * RW_THREADS + threadIdx.x; p <= V.n_matches; p += (uint64_t)gridDim.x * RW_THREADS) {
		if (p == V.n_matches) { V.n_out[p] = 0; continue; }
		const uint32_t m = V.pm[p];
		const RwMatch M = V.mt[m];
		const pga_plan_match_t Mt = V.o_match[m];
		if (p > 0) { const uint32_t m1 = V.pm[p - 1]; if (V.mt[m1].group == M.group && V.o_match[m1].new_block_id == Mt.new_block_id) rw_fail(V, RW_ERR_DUP_ID, m); }
		const uint32_t a = (uint32_t)Mt.anchor, n = M.n_cigar, rev = M.reverse ? 1u : 0u;
		const uint32_t *cig = V.cig + M.cigar_off;
		int64_t lead_i = -1, lead_d = -1, trail_i = -1, trail_d = -1;
		bool has_m = false;
		for (uint32_t i = 0; i < n; ++i) {
			const uint32_t op = rw_base_op(cig, n, a, rev, i) & 15u;
			if (rw_is_match(op)) { has_m = true; break; }
			if (op == RW_OP_I) lead_i = i; else if (op == RW_OP_D) lead_d = i;
		}
		for (uint32_t i = n; i-- > 0;) {
			const uint32_t op = rw_base_op(cig, n, a, rev, i) & 15u;
			if (rw_is_match(op)) break;
			if (op == RW_OP_I) trail_i = i; else if (op == RW_OP_D) trail_d = i;
		}
		const RwExt A = V.ext[2 * m + a], Q = V.ext[2 * m + (1u - a)];
		RwPlan P;
		P.nf = P.nb = 0;
		P.front[0] = P.front[1] = P.back[0] = P.back[1] = 0;
#pragma unroll
		for (int k = 0; k < 4; ++k) { P.mod_idx[k] = 0xffffffffu; P.mod_add[k] = 0; }
		bool ok = rw_add_flank(P, cig, n, a, rev, has_m, lead_d, trail_d, RW_OP_D, A.left, true, 0);
		ok = rw_add_flank(P, cig, n, a, rev, has_m, lead_d, trail_d, RW_OP_D, A.right, false, 1) && ok;
		ok = rw_add_flank(P, cig, n, a, rev, has_m, lead_i, trail_i, RW_OP_I, Q.left, !rev, 2) && ok;
		ok = rw_add_flank(P, cig, n, a, rev, has_m, lead_i, trail_i, RW_OP_I, Q.right, rev != 0, 3) && ok;
		if (!ok) rw_fail(V, RW_ERR_OP_LEN, m);
		V.plan[p] = P;
		V.n_out[p] = (rw_u64)P.nf + n + P.nb;
	}
}
// one wave per promise: the operations in their places (lanes over operations), the record
__global__ __launch_bounds__(RW_THREADS) void k_rw_cigar_write(RwDev V)
{
	const uint32_t lane = threadIdx.x & 63u;
	for (uint64_t p = (uint64_t)blockIdx.x * RW_WAVES + (threadIdx.x >> 6); p < V.n_matches; p += (uint64_t)gridDim.x * RW_WAVES) {
		const uint32_t m = V.pm[p];
		const RwMatch &M = V.mt[m];
		const pga_plan_match_t Mt = V.o_match[m];
		const RwPlan P = V.plan[p];
		const uint32_t a = (uint32_t)Mt.anchor, n = M.n_cigar, rev = M.reverse ? 1u : 0u;
		const uint32_t *cig = V.cig + M.cigar_off;
		const rw_u64 c0 = V.c_off[p];
		for (uint32_t t = lane; t < P.nf + n + P.nb; t += 64) {
			uint32_t w;
			if (t < P.nf) w = t == 0 ? P.front[0] : P.front[1];
			else if (t < P.nf + n) {
				const uint32_t i = t - P.nf;
				w = rw_base_op(cig, n, a, rev, i);
				const uint32_t op = w & 15u;
				if (!rw_is_match(op) && op != RW_OP_I && op != RW_OP_D) rw_fail(V, RW_ERR_OP_KIND, m);
#pragma unroll
				for (int k = 0; k < 4; ++k) if (P.mod_idx[k] == i) w += P.mod_add[k] << 4;
			} else w = t == P.nf + n ? P.back[0] : P.back[1];
			if (c0 + t < V.cap_cig) V.o_cig[c0 + t] = w;
		}
		if (lane == 0)
			V.o_prom[p] = pga_plan_promise_t{Mt.new_block_id, (int64_t)m, V.iv_of[2 * m + a], V.iv_of[2 * m + (1u - a)], c0, M.blk[a], M.blk[1u - a], P.nf + n + P.nb, (int32_t)rev};
	}
}

// ---------------------------------------------------------------- host side: validation and the tables every launch reads
struct RwTables {
	std::vector<RwBlk> blk; std::vector<RwMatch> mt;
	std::vector<uint32_t> hb_block;          // per block with a hit, in output order: its index in the input
	std::vector<uint32_t> eq;                // matches of equal depth
	uint64_t cigar_in = 0; uint32_t n_groups = 0;
};
struct RwResident { const uint16_t *nmask; uint64_t pos; };   // where a block's bit plane lies (nmask == NULL: not resident)

// Throws std::runtime_error on what fails the call before anything is launched.
static void rw_build_tables(int32_t n_groups, const int64_t *group_off, const pga_plan_block_t *blocks, int64_t n_matches, const pga_match_t *matches,
                            const uint32_t *cigars, uint64_t n_ops, const RwResident *res, RwTables &T)
{
	auto fail = [](const std::string &what) { throw std::runtime_error("pga_plan_merge: " + what); };
	if (n_groups < 0 || !group_off) fail("null or negative group table");
	if (group_off[0] != 0) fail("group_off[0] must be 0");
	for (int32_t g = 0; g < n_groups; ++g) if (group_off[g + 1] < group_off[g]) fail("group offsets decrease");
	const int64_t nb = group_off[n_groups];
	if (nb >= (1LL << 31) || n_matches >= (1LL << 30) || n_ops >= (1ULL << 32)) fail("more than 2^31 blocks, 2^30 matches or 2^32 CIGAR operations");
	if (nb && !blocks) fail("null block list");
	if (n_matches && !matches) fail("null match list");
	T.n_groups = (uint32_t)n_groups;
	T.blk.resize((size_t)nb);
	std::vector<uint32_t> order;
	for (int32_t g = 0; g < n_groups; ++g) {
		const int64_t b0 = group_off[g], b1 = group_off[g + 1];
		order.resize((size_t)(b1 - b0));
		for (int64_t i = b0; i < b1; ++i) {
			order[(size_t)(i - b0)] = (uint32_t)i;
			if (blocks[i].cons_len && !blocks[i].consensus) fail("null letters with cons_len > 0 (block " + std::to_string(i) + ")");
		}
		std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return blocks[x].block_id < blocks[y].block_id; });
		for (size_t r = 0; r < order.size(); ++r) {
			const uint32_t i = order[r];
			if (r && blocks[order[r - 1]].block_id == blocks[i].block_id) fail("two blocks of group " + std::to_string(g) + " share the block id " + std::to_string(blocks[i].block_id));
			T.blk[i] = RwBlk{blocks[i].block_id, res ? res[i].nmask : nullptr, res ? res[i].pos : 0, blocks[i].cons_len, blocks[i].depth, (uint32_t)(b0 + (int64_t)r), 0u};
		}
	}
	T.mt.resize((size_t)n_matches);
	std::vector<uint8_t> has_hit((size_t)nb, 0);
	for (int64_t m = 0; m < n_matches; ++m) {
		const pga_match_t &A = matches[m];
		const std::string at = " (match " + std::to_string(m) + ")";
		if (A.group < 0 || A.group >= n_groups) fail("group outside the group table" + at);
		const int64_t b0 = group_off[A.group], n = group_off[A.group + 1] - b0;
		if (A.qry < 0 || A.qry >= n || A.ref < 0 || A.ref >= n) fail("block index outside its group" + at);
		if (A.qry == A.ref) fail("a match of a block with itself" + at);
		const uint32_t rb = (uint32_t)(b0 + A.ref), qb = (uint32_t)(b0 + A.qry);
		if (A.ref_start < 0 || A.ref_start >= A.ref_end || A.qry_start < 0 || A.qry_start >= A.qry_end) fail("an empty hit" + at);
		if ((uint64_t)A.ref_end > blocks[rb].cons_len || (uint64_t)A.qry_end > blocks[qb].cons_len) fail("a hit outside its block" + at);
		if (A.cigar_off > n_ops || A.n_cigar > n_ops - A.cigar_off) fail("CIGAR outside the pool" + at);
		if (A.n_cigar && !cigars) fail("null CIGAR pool" + at);
		RwMatch &M = T.mt[(size_t)m];
		M.cigar_off = A.cigar_off; M.blk[0] = rb; M.blk[1] = qb;
		M.start[0] = (uint32_t)A.ref_start; M.end[0] = (uint32_t)A.ref_end; M.start[1] = (uint32_t)A.qry_start; M.end[1] = (uint32_t)A.qry_end;
		M.n_cigar = A.n_cigar; M.reverse = A.reverse ? 1u : 0u; M.group = (uint32_t)A.group; M.letters = 0;
		has_hit[rb] = has_hit[qb] = 1;
		if (blocks[rb].depth == blocks[qb].depth) T.eq.push_back((uint32_t)m);
		T.cigar_in += A.n_cigar;
	}
	std::vector<uint32_t> by_ord((size_t)nb);
	for (int64_t i = 0; i < nb; ++i) by_ord[T.blk[(size_t)i].ord] = (uint32_t)i;
	for (int64_t r = 0; r < nb; ++r) { const uint32_t i = by_ord[(size_t)r]; if (has_hit[i]) { T.blk[i].hb = (uint32_t)T.hb_block.size(); T.hb_block.push_back(i); } }
}

} // namespace pga
