// pga_ksw_shared.h -- what the kernel classes of the dual-affine DP (pga_ksw*.hip, pga_ll.hip) have in common, once: the ksw2 flag bits and
// size limits, the diagonal range, the gap-cost prologue, the view of a problem's two windows in the packed store, and the windowed backtrack
// with its CIGAR hand-over.  Everything here is __forceinline__ (plus template parameters where the classes differ): a kernel that uses a piece
// compiles to what its own copy compiled to.
//
// The constants stand in front of the include of pga_dp.h, and pga_dp.h includes this header behind its descriptors: the length-bound stop
// there tests flag bits by name, and the pieces below need the descriptors -- either header may be included first.
#pragma once

#define KSW_NEG_INF (-0x40000000)
// DpJob.flag: the KSW_EZ_* bits of ksw2.h:12-21 (and PGA_JOB_LL, pga_dp.h)
#define EZ_RIGHT       0x02
#define EZ_APPROX_MAX  0x08
#define EZ_APPROX_DROP 0x10
#define EZ_EXTZ_ONLY   0x40
#define EZ_REV_CIGAR   0x80
#define WIDE_LDS_MAX (152 * 1024)   // dynamic LDS the workgroup kernel may ask for (160 KB per CU minus its static arrays); dp_class sizes classes with it
#define BAND_MAXLEN 1024            // longest query / target the corridor kernel takes (LDS sequence buffers)

#include "pga_dp.h"
#include "pga_wave.h"

namespace pga {

__device__ __forceinline__ int sx8(int v) { return __builtin_amdgcn_sbfe(v, 0, 8); }

// the columns [st0, en0] of anti-diagonal r (ksw2_extd2_sse.c:140-145); st0 > en0: the band has slid past the target
__host__ __device__ __forceinline__ void diag_range(int r, int qlen, int tlen, int w, int &st0, int &en0)
{
	int st = 0, en = tlen - 1;
	if (st < r - qlen + 1) st = r - qlen + 1;
	if (en > r) en = r;
	if (st < (r - w + 1) >> 1) st = (r - w + 1) >> 1;
	if (en > (r + w) >> 1) en = (r + w) >> 1;
	st0 = st, en0 = en;
}
// ... of a problem whose band never binds (w >= qlen and w >= tlen)
__device__ __forceinline__ void diag_range(int r, int qlen, int tlen, int &st0, int &en0)
{
	st0 = r - qlen + 1 > 0 ? r - qlen + 1 : 0;
	en0 = r < tlen - 1 ? r : tlen - 1;
}

// The gap costs of a problem as ksw2_extd2_sse.c:73-89 prepares them: (q, e) is the pair that is cheaper to open, qe_h is taken before the swap.
struct GapCosts {
	int q, e, q2, e2, qe_h, qe, qe2, long_thres, long_diff, sc_N;
	__device__ __forceinline__ explicit GapCosts(const DpParams &P)
	{
		q = P.q, e = P.e, q2 = P.q2, e2 = P.e2;
		qe_h = q + e;
		if (q2 + e2 < q + e) { int t = q; q = q2, q2 = t, t = e, e = e2, e2 = t; }
		qe = q + e, qe2 = q2 + e2;
		sc_N = P.sc_ambi == 0 ? -e2 : P.sc_ambi;
		long_thres = e != e2 ? (q2 - q) / (e - e2) - 1 : 0;
		if (q2 + e2 + long_thres * e2 > q + e + long_thres * e) ++long_thres;
		long_diff = long_thres * (e - e2) - (q2 - q) - e2;
	}
	// u of row 0 / v of column 0 on diagonal r (ksw2_extd2_sse.c:155-163); the caller wraps it to the width of its rows
	__device__ __forceinline__ int first_row(int r) const { return r == 0 ? -q - e : r < long_thres ? -e : r == long_thres ? long_diff : -e2; }
};

// The two windows of a problem in the packed store.  Reversal (left extension, align.c:711-713) and reverse complement (align.c:970-975) are index
// transforms applied when a base is read.  *_in: the index lies inside the window; the others return 0 outside it (the reference's zero padding).
struct SeqView {
	PkBases nt; uint64_t t_base, q_base;   // the packed store; target window start / query sequence start in it
	int32_t qlen_full, qs, qlen, tlen;
	bool q_rev, seq_rev;
	__device__ __forceinline__ SeqView(PkBases bases, const DpJob &J)
		: nt(bases), t_base(J.t_off), q_base(J.q_off), qlen_full(J.qlen_full), qs(J.qs), qlen(J.qlen), tlen(J.tlen), q_rev(J.q_rev), seq_rev(J.seq_rev) {}
	__device__ __forceinline__ int target_in(int i) const { return nt.at(t_base + (uint64_t)(seq_rev ? tlen - 1 - i : i)); }
	__device__ __forceinline__ int target(int i) const { return i < tlen ? target_in(i) : 0; }               // i >= 0
	__device__ __forceinline__ int target_any(int i) const { return (i >= 0 && i < tlen) ? target_in(i) : 0; }
	__device__ __forceinline__ int query_in(int j) const
	{
		const int pj = qs + (seq_rev ? qlen - 1 - j : j);
		if (!q_rev) return nt.at(q_base + (uint64_t)(pj));
		return PkBases::complement(nt.at(q_base + (uint64_t)(qlen_full - 1 - pj)));
	}
	__device__ __forceinline__ int query(int j) const { return (j < 0 || j >= qlen) ? 0 : query_in(j); }
};

// ---- the backtrack (ksw2.h:127-159, is_rot = 1) ----
#define BT_WIN 64   // rows (diagonals) and columns of the LDS window

// ONE wave walks the path back from (bi, bj) through a BT_WIN x BT_WIN window of the direction matrix in LDS: the wave refills the window around
// the path's head with coalesced loads (ROWS_IN_FLIGHT rows requested before the first is stored) and every lane tracks (i, j, state) while the
// path stays inside it; the operation being extended lives in registers, lane 0 stores one word per operation to cig_tmp (end of the alignment
// first).  Returns the number of operations, or a negative count when more than guard_max windows were filled (a safety net: a stuck wave would
// take the device down).
//   range(r, st0, en0)  the diagonal's columns; the matrix holds p[r][t - off] for the sixteen-rounded off ... off_end, and the walk forces the
//                       state outside them
//   fetch(r, col)       the direction byte of (r, col), r >= 0 and col >= 0, or 0 where the class stored none: the matrix's layout (flat or
//                       chunked) and what counts as stored are the caller's
//   guard               the caller's counter (its lifetime is the caller's too)
//   TAIL_AFTER_GUARD    the leading insertion / deletion is pushed even when the guard has tripped
template <int ROWS_IN_FLIGHT, bool TAIL_AFTER_GUARD, class Range, class Fetch>
__device__ __forceinline__ int backtrack_windowed(int lane, int bi, int bj, uint8_t *s_win, uint32_t *cig_tmp, long long &guard, long long guard_max, Range range, Fetch fetch)
{
	int n_cigar = 0, i = bi, j = bj, state = 0;
	uint32_t last_op = 0xffffffffu, run_len = 0;
	auto cg_push = [&](uint32_t op, uint32_t len) {
		if (op == last_op) { run_len += len; return; }
		if (last_op != 0xffffffffu) { if (lane == 0) cig_tmp[n_cigar] = run_len << 4 | last_op; ++n_cigar; }
		last_op = op; run_len = len;
	};
	auto cg_flush = [&] { if (last_op != 0xffffffffu && n_cigar >= 0) { if (lane == 0) cig_tmp[n_cigar] = run_len << 4 | last_op; ++n_cigar; last_op = 0xffffffffu; } };
	while (i >= 0 && j >= 0) {                                          // wave-uniform loop
		if (++guard > guard_max) { n_cigar = -7; break; }
		// window: rows r_hi-63 .. r_hi, target columns i-63 .. i (the path moves at most one column per step)
		const int r_hi = i + j, c_lo = i - (BT_WIN - 1);
		for (int part = 0; part < BT_WIN; part += ROWS_IN_FLIGHT) {
			uint8_t wv[ROWS_IN_FLIGHT];
#pragma unroll
			for (int rw = 0; rw < ROWS_IN_FLIGHT; ++rw) {
				const int r = r_hi - (part + rw), col = c_lo + lane;
				uint8_t val = 0;
				if (r >= 0 && col >= 0) val = fetch(r, col);
				wv[rw] = val;
			}
#pragma unroll
			for (int rw = 0; rw < ROWS_IN_FLIGHT; ++rw) s_win[(part + rw) * BT_WIN + lane] = wv[rw];
		}
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // one wave: LDS is in order, a fence replaces the barrier
		// walk while the path stays inside the window
		while (i >= 0 && j >= 0) {
			const int r = i + j, row = r_hi - r;
			if (row >= BT_WIN || i < c_lo) break;
			int st0, en0; range(r, st0, en0);
			const int off = st0 / 16 * 16, off_end = (en0 + 16) / 16 * 16 - 1;
			int force_state = -1;
			if (i < off) force_state = 2;
			if (i > off_end) force_state = 1;
			const uint32_t tmp = force_state < 0 ? s_win[row * BT_WIN + (i - c_lo)] : 0;
			if (state == 0) state = tmp & 7;
			else if (!(tmp >> (state + 2) & 1)) state = 0;
			if (state == 0) state = tmp & 7;
			if (force_state >= 0) state = force_state;
			uint32_t op;
			if (state == 0) op = 0, --i, --j;
			else if (state == 1 || state == 3) op = 2, --i;
			else op = 1, --j;
			cg_push(op, 1u);
		}
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
	}
	if (bi >= 0 && bj >= 0 && (TAIL_AFTER_GUARD || n_cigar >= 0)) {
		if (i >= 0) cg_push(2u, (uint32_t)(i + 1));
		if (j >= 0) cg_push(1u, (uint32_t)(j + 1));
	}
	cg_flush();
	return n_cigar;
}

// n_cigar words of the CIGAR pool with ONE atomic (by the lane for which `take` holds); the offset goes to every lane from lane `src`
__device__ __forceinline__ unsigned long long cigar_reserve(bool take, int src, int n_cigar, unsigned long long *pool_cursor)
{
	unsigned long long base = 0;
	if (take) base = atomicAdd(pool_cursor, (unsigned long long)n_cigar);
	return ((unsigned long long)(unsigned)__shfl((int)(base >> 32), src) << 32) | (unsigned)__shfl((int)(base & 0xffffffffULL), src);
}

// the ksw_extz_t part of a result; n_cigar, pad and cigar_off are the caller's and cigar_commit's
__device__ __forceinline__ DpRes ez_record(int max, int max_q, int max_t, int mqe, int mqe_t, int mte, int mte_q, int score, int zdropped, int reach_end)
{
	DpRes R;
	R.max = max, R.max_q = max_q, R.max_t = max_t, R.mqe = mqe, R.mqe_t = mqe_t, R.mte = mte, R.mte_q = mte_q;
	R.score = score, R.zdropped = zdropped, R.reach_end = reach_end, R.n_cigar = 0, R.pad = 0, R.cigar_off = 0;
	return R;
}

// The end of a problem, by the wave that walked its path: the pool words are reserved, the operations copied out of cig_tmp (reversed into
// alignment order unless rev_cigar) and the record stored with their offset.  The copy is dropped when the pool is full (the host sees the cursor).
//   FENCE       between the reservation and the copy (callers that have fenced cig_tmp themselves pass false)
//   TEST_EMPTY  the copy stands under n_cigar > 0
template <bool FENCE, bool TEST_EMPTY>
__device__ __forceinline__ void cigar_commit(int lane, int n_cigar, bool rev_cigar, const uint32_t *cig_tmp, uint32_t *__restrict__ cigar_pool, unsigned long long *__restrict__ pool_cursor,
                                             unsigned long long pool_cap, DpRes R, DpRes *out)
{
	const unsigned long long base = cigar_reserve(lane == 0 && n_cigar > 0, 0, n_cigar, pool_cursor);
	if (FENCE) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
	if ((!TEST_EMPTY || n_cigar > 0) && base + (unsigned long long)n_cigar <= pool_cap)
		for (int c = lane; c < n_cigar; c += 64) cigar_pool[base + c] = rev_cigar ? cig_tmp[c] : cig_tmp[n_cigar - 1 - c];
	if (lane == 0) { R.cigar_off = base; *out = R; }
}

} // namespace pga
