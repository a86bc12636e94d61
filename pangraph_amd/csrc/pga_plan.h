// pga_plan.h -- records exchanged between the alignment driver (pga_align.cpp) and the device-side planner (pga_plan.hip), and the part of
// mm_align1's arithmetic before its first DP call that both of them run: the view of a query's anchors, the end trimming and the extension windows
#pragma once
#include "pga_common.h"

namespace pga {

// anchor flag bits (mmpriv.h:18-24)
static const uint64_t A_LONG_JOIN = 1ULL << 40, A_IGNORE = 1ULL << 41, A_TANDEM = 1ULL << 42, A_SELF = 1ULL << 43;

__host__ __device__ __forceinline__ int plan_min(int a, int b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ int plan_max(int a, int b) { return a > b ? a : b; }
__host__ __device__ __forceinline__ int plan_abs(int a) { return a < 0 ? -a : a; }

// ---- anchors of one query, in host or device memory: x = strand<<63 | target<<32 | target position, y = flags | span<<32 | query position (lchain.c:140-147) ----
struct Anchors {
	u128 *a; int32_t n;
	__host__ __device__ __forceinline__ int32_t tpos(int i) const { return (int32_t)a[i].x; }
	__host__ __device__ __forceinline__ int32_t qpos(int i) const { return (int32_t)a[i].y; }
	__host__ __device__ __forceinline__ int32_t span(int i) const { return (int32_t)(a[i].y >> 32 & 0xff); }
	__host__ __device__ __forceinline__ uint64_t target_key(int i) const { return a[i].x >> 32; }        // strand + target id
	__host__ __device__ __forceinline__ bool flagged(int i, uint64_t f) const { return (a[i].y & f) != 0; }
	__host__ __device__ __forceinline__ void flag(int i, uint64_t f) { a[i].y |= f; }
	// query advance minus target advance between anchor i-1 and i: > 0 insertion, < 0 deletion
	__host__ __device__ __forceinline__ int32_t indel(int i) const { return (qpos(i) - qpos(i - 1)) - (tpos(i) - tpos(i - 1)); }
};

// Seeds at either end of the chain [r_as, r_as + r_cnt) that sit off the diagonal of what follows are cut off (mm_fix_bad_ends, align.c:471-509):
// [as1, as1 + cnt1) is what is left.  (In the kernel every lane calls this with the same arguments: the loads are broadcast.)
__host__ __device__ __forceinline__ void trim_chain_ends(const Anchors &A, int r_as, int r_cnt, int32_t r_mlen, int bw, int min_match, int32_t &as1, int32_t &cnt1)
{
	as1 = r_as, cnt1 = r_cnt;
	if (r_cnt < 3) return;
	const int last = r_as + r_cnt - 1;
	int32_t len, match;
	len = match = A.span(r_as);
	for (int i = r_as + 1; i < last; ++i) {
		if (A.flagged(i, A_LONG_JOIN)) break;
		const int32_t dt = A.tpos(i) - A.tpos(i - 1), dq = A.qpos(i) - A.qpos(i - 1), lo = plan_min(dt, dq), hi = plan_max(dt, dq);
		if (hi - lo > len >> 1) as1 = i;
		len += lo, match += plan_min(lo, A.span(i));
		if (len >= bw << 1 || (match >= min_match && match >= bw) || match >= r_mlen >> 1) break;
	}
	cnt1 = last + 1 - as1;
	len = match = A.span(last);
	for (int i = last - 1; i > as1; --i) {
		if (A.flagged(i + 1, A_LONG_JOIN)) break;
		const int32_t dt = A.tpos(i + 1) - A.tpos(i), dq = A.qpos(i + 1) - A.qpos(i), lo = plan_min(dt, dq), hi = plan_max(dt, dq);
		if (hi - lo > len >> 1) cnt1 = i + 1 - as1;
		len += lo, match += plan_min(lo, A.span(i + 1));
		if (len >= bw << 1 || (match >= min_match && match >= bw) || match >= r_mlen >> 1) break;
	}
}

// The extension windows (align.c:633-696).  rs, qs, re, qe: the trimmed chain's ends; rs0, qs0, re0, qe0: in, the untrimmed chain's ends -- out, where
// the left extension may start and the right one may end; (rs1, qs1), (re1, qe1): what the scans over the neighbouring chains found (0, 0 and
// tlen_ref, qlen when nothing); self: the chain's first anchor carries A_SELF, then r_rs .. r_qe (chain_extent) bound the windows.
__host__ __device__ __forceinline__ void extension_windows(int32_t rs, int32_t qs, int32_t re, int32_t qe, int32_t &rs0, int32_t &qs0, int32_t &re0, int32_t &qe0,
                                                         int32_t rs1, int32_t qs1, int32_t re1, int32_t qe1, int32_t qlen, int32_t tlen_ref,
                                                         bool self, int32_t r_rs, int32_t r_qs, int32_t r_re, int32_t r_qe, int max_gap, int a, int q, int e)
{
	if (qs > 0 && rs > 0) {
		int32_t l = plan_min(qs, max_gap);
		qs1 = plan_max(qs1, qs - l);
		qs0 = plan_min(qs0, qs1);
		l += l * a > q ? (l * a - q) / e : 0;
		l = plan_min(plan_min(l, max_gap), rs);
		rs1 = plan_max(rs1, rs - l);
		rs0 = plan_min(plan_min(rs0, rs1), rs);
	} else rs0 = rs, qs0 = qs;
	if (qe < qlen && re < tlen_ref) {
		int32_t l = plan_min(qlen - qe, max_gap);
		qe1 = plan_min(qe1, qe + l);
		qe0 = plan_max(qe0, qe1);
		l += l * a > q ? (l * a - q) / e : 0;
		l = plan_min(plan_min(l, max_gap), tlen_ref - re);
		re1 = plan_min(re1, re + l);
		re0 = plan_max(re0, re1);
	} else re0 = re, qe0 = qe;
	if (self) {
		int max_ext = plan_abs(r_qs - r_rs);
		if (r_rs - rs0 > max_ext) rs0 = r_rs - max_ext;
		if (r_qs - qs0 > max_ext) qs0 = r_qs - max_ext;
		max_ext = plan_abs(r_qe - r_re);
		if (re0 - r_re > max_ext) re0 = r_re + max_ext;
		if (qe0 - r_qe > max_ext) qe0 = r_qe + max_ext;
	}
}

struct PlanIn {                 // one region = one chain (or a piece split off one)
	uint64_t a_off;             // index of the QUERY's first compacted anchor in the device array
	uint64_t item_off;          // this region's slice of the item pool
	uint32_t item_cap;
	int32_t n_a;                // anchors of the query (neighbouring chains are scanned for the extension windows)
	int32_t as, cnt;            // the chain inside the query's anchors
	int32_t qlen, qid, base;    // query length, sequence index of the query, first sequence of its group
	int32_t pad;
};

struct PlanOut {
	int32_t status;             // 0 ok, 1 item slice too small (n_items says how many), 2 too many long gaps for the kernel, 3 empty chain
	int32_t rid, rev;
	int32_t r_rs, r_re, r_qs, r_qe, r_mlen, r_blen;          // chain_extent (hit.c:8-38)
	int32_t as1, cnt1, rs, qs, rs0, qs0, re0, qe0, T_re, T_qe; // what mm_align1 fixes before its first DP call (align.c:583-700)
	uint32_t n_items; int32_t n_long_gaps;
};

struct PlanItem {               // kind 0: a RUN of consecutive segments the identity probe answered "nM" (m mismatches in all, bw1 = how many segments);
	int32_t kind, i, rs, qs, re, qe, bw1, m, i_prev;          // kind 1 / 2: a segment that needs a DP problem (2: equally long windows, the probe said no); i = its
	int32_t pad[3];             // last anchor (chain-relative to as1), i_prev = the anchor it starts at
};

struct PlanParams {
	int32_t k, bw, bw_long, max_gap, min_cnt, min_chain_score, min_ksw_len, a, q, e, no_end_flt, probe_m_max;
	int32_t g_max, pad;         // long gaps of a region the kernel plans itself (<= PLAN_G_MAX of pga_plan.hip; PGA_PLAN_G_MAX lowers it: tests of the host route)
	int64_t max_sw_mat;
};

void plan_regions(const std::vector<PlanIn> &in, u128 *d_anchors, PkBases bases, const uint64_t *d_seq_off, const uint32_t *d_seq_len, const PlanParams &P,
                  std::vector<PlanOut> &out, std::vector<PlanItem> &items, hipStream_t st);
void gather_anchors(const std::vector<uint64_t> &idx, const u128 *d_anchors, std::vector<u128> &out, hipStream_t st);

} // namespace pga
