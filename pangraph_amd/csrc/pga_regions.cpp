// pga_regions.cpp -- hit.c's region bookkeeping (mm_gen_regs, mm_split_reg, mm_filter_regs, mm_hit_sort, mm_set_mapq: hit.c:8-88,106-123,188-218,
// 290-329,396-466) and the dp_max rescaling of align.c:897-960 (reference: packages/minimap2-sys/minimap2/), over the records of pga_pipeline.h.
#include "pga_regions.h"
#include "pga_sort_exact.h"
#include <cmath>

namespace pga {

static void sort_by_x(std::vector<u128> &v) { uint32_t head[256], tail[256]; if (!v.empty()) radix_sort_128x_exact(v.data(), v.data() + v.size(), head, tail); }

// ---------------------------------------------------------------- region records from chains
// Coordinates of a chain (hit.c:23-38) and its approximate match / block lengths (hit.c:8-21): one pass over the anchors.
static void chain_extent(Reg &r, int32_t qlen, const Anchors &A)
{
	const int first = r.as, last = r.as + r.cnt - 1;
	const int32_t sp0 = A.span(first);
	r.rev = (uint32_t)(A.a[first].x >> 63);
	r.rid = (int32_t)(A.a[first].x << 1 >> 33);
	r.rs = std::max(0, A.tpos(first) + 1 - sp0);
	r.re = A.tpos(last) + 1;
	const int32_t q_lo = A.qpos(first) + 1 - sp0, q_hi = A.qpos(last) + 1;       // on the aligned strand
	if (r.rev) r.qs = qlen - q_hi, r.qe = qlen - q_lo; else r.qs = q_lo, r.qe = q_hi;
	int32_t covered = 0, block = 0;
	if (r.cnt > 0) {
		covered = block = sp0;
		for (int i = first + 1; i <= last; ++i) {
			const int32_t dt = A.tpos(i) - A.tpos(i - 1), dq = A.qpos(i) - A.qpos(i - 1), sp = A.span(i);
			block += std::max(dt, dq);
			covered += (dt > sp && dq > sp) ? sp : std::min(dt, dq);
		}
	}
	r.mlen = covered, r.blen = block;
}

static inline uint64_t mix64(uint64_t k) // the 64-bit finalizer hit.c:40-50 salts region keys with
{
	k = ~k + (k << 21); k ^= k >> 24;
	k = k + (k << 3) + (k << 8); k ^= k >> 14;
	k = k + (k << 2) + (k << 4); k ^= k >> 28;
	k += k << 31;
	return k;
}

// One region per chain, ordered by descending (score<<32 | cnt) ^ salt(first anchor, query) -- hit.c:52-88.  The order of equal keys
// is the one minimap2's radix sort leaves, so the keys go through its exact replay.
void regions_from_chains(uint32_t query_salt, int qlen, int n_chains, const uint64_t *u, const Anchors &A, std::vector<Reg> &regs, const u128 *heads)
{
	// heads: the first anchor of every chain, gathered on the device (then A holds no anchors and the extents are left to the planner)
	regs.clear();
	if (n_chains == 0) return;
	std::vector<u128> key((size_t)n_chains);
	int32_t start = 0;
	for (int c = 0; c < n_chains; ++c) {
		const u128 h0 = heads ? heads[c] : A.a[start];
		const uint32_t salt = (uint32_t)mix64((mix64(h0.x) + mix64(h0.y)) ^ query_salt);
		const int32_t cnt = (int32_t)u[c];
		key[(size_t)c].x = u[c] ^ salt;
		key[(size_t)c].y = (uint64_t)start << 32 | (uint32_t)cnt;
		start += cnt;
	}
	sort_by_x(key);
	regs.resize((size_t)n_chains);
	for (int c = 0; c < n_chains; ++c) {
		const u128 &k = key[(size_t)(n_chains - 1 - c)];          // descending
		Reg &r = regs[(size_t)c] = Reg();
		r.id = c, r.parent = -1;                                   // -X: no primary/secondary selection, parents stay unset
		r.score = r.score0 = (int32_t)(k.x >> 32), r.hash = (uint32_t)k.x;
		r.cnt = (int32_t)(uint32_t)k.y, r.as = (int32_t)(k.y >> 32);
		if (!heads) chain_extent(r, qlen, A);
	}
}

// The tail of `head` from its anchor `n_keep` on becomes its own region (hit.c:106-123); scores are shared out by anchor counts.
void cut_region(Reg &head, Reg &tail, int n_keep, int qlen, const Anchors &A, bool extents)
{
	if (n_keep <= 0 || n_keep >= head.cnt) return;
	const int total = head.cnt;
	tail = head;
	tail.id = -1, tail.split_inv = 0;
	tail.has_p = false, tail.cigar.clear(), tail.dp_score = tail.dp_max = tail.dp_max2 = 0, tail.n_ambi = 0;
	tail.as = head.as + n_keep, tail.cnt = total - n_keep;
	tail.score = (int32_t)(head.score * ((float)tail.cnt / total) + .499);
	if (head.parent == head.id) tail.parent = -2;                 // MM_PARENT_TMP_PRI
	head.cnt = n_keep, head.score -= tail.score;
	// (device-side planning: the tail's extent comes back with its plan; the head's is overwritten by what its alignment found)
	if (extents) { chain_extent(tail, qlen, A); chain_extent(head, qlen, A); }
	head.split |= 1, tail.split |= 2;
}

static bool region_survives(const mm_mapopt_t &opt, int qlen, const Reg &r) // hit.c:290-309
{
	if (!r.inv && r.cnt < opt.min_cnt) return false;
	if (!r.has_p) return true;
	if (r.mlen < opt.min_chain_score || r.dp_max < opt.min_dp_max) return false;
	return !(r.qs > qlen * opt.max_clip_ratio && qlen - r.qe > qlen * opt.max_clip_ratio);
}
void drop_weak_regions(const mm_mapopt_t &opt, int qlen, std::vector<Reg> &regs)
{
	regs.erase(std::remove_if(regs.begin(), regs.end(), [&](const Reg &r) { return !region_survives(opt, qlen, r); }), regs.end());
}

// descending DP score (chain score without a CIGAR), ties by the salted hash, equal keys as minimap2's sort leaves them (hit.c:188-218)
void order_regions(std::vector<Reg> &regs)
{
	if (regs.size() <= 1) return;
	std::vector<u128> key; key.reserve(regs.size());
	for (size_t i = 0; i < regs.size(); ++i) {
		const Reg &r = regs[i];
		if (!r.inv && r.cnt <= 0) continue;
		key.push_back(u128{(uint64_t)(r.has_p ? r.dp_max : r.score) << 32 | r.hash, (uint64_t)i});
	}
	sort_by_x(key);
	std::vector<Reg> out; out.reserve(key.size());
	for (auto it = key.rbegin(); it != key.rend(); ++it) out.push_back(std::move(regs[it->y]));
	regs.swap(out);
}

// mapping quality of one primary region (hit.c:421-466, long reads); float arithmetic in the reference's order
static uint32_t region_mapq(const Reg &r, float uniq_ratio, int min_chain_sc, int match_sc)
{
	const float coef = 40.0f;
	const float by_score = (r.score > 100 ? 1.0f : 0.01f * r.score) * uniq_ratio, by_cnt = r.cnt > 10 ? 1.0f : 0.1f * r.cnt;
	const float pen = by_score < by_cnt ? by_score : by_cnt;
	const int subsc = std::max(r.subsc, min_chain_sc);
	int mapq;
	if (r.has_p && r.dp_max2 > 0 && r.dp_max > 0) {
		const float identity = (float)r.mlen / r.blen;
		const float x = (float)r.dp_max2 * subsc / r.dp_max / r.score0;
		mapq = (int)(identity * pen * coef * (1.0f - x * x) * logf((float)r.dp_max / match_sc));
		const int alt = (int)(6.02f * identity * identity * (r.dp_max - r.dp_max2) / match_sc + .499f);
		mapq = std::min(mapq, alt);
	} else {
		const float x = (float)subsc / r.score0;
		if (r.has_p) { const float identity = (float)r.mlen / r.blen; mapq = (int)(identity * pen * coef * (1.0f - x) * logf((float)r.dp_max / match_sc)); }
		else mapq = (int)(pen * coef * (1.0f - x) * logf(r.score));
	}
	mapq -= (int)(4.343f * logf(r.n_sub + 1) + .499f);
	uint32_t q = (uint32_t)std::min(60, std::max(0, mapq));
	if (r.has_p && r.dp_max > r.dp_max2 && q == 0) q = 1;
	return q;
}
void assign_mapq(std::vector<Reg> &regs, int min_chain_sc, int match_sc, int rep_len)
{
	if (regs.empty()) return;
	int64_t primary_sum = 0;
	for (const Reg &r : regs) if (r.parent == r.id) primary_sum += r.score;
	const float uniq_ratio = (float)primary_sum / (primary_sum + rep_len);
	for (Reg &r : regs) r.mapq = (!r.inv && r.parent == r.id) ? region_mapq(r, uniq_ratio, min_chain_sc, match_sc) : 0;
	// an inversion inherits the weaker of its two flanks (hit.c:396-419)
	if (regs.size() < 3 || std::none_of(regs.begin(), regs.end(), [](const Reg &r) { return r.inv != 0; })) return;
	std::vector<u128> by_pos;
	for (int i = 0; i < (int)regs.size(); ++i) if (regs[(size_t)i].parent == i || regs[(size_t)i].parent < 0) by_pos.push_back(u128{(uint64_t)regs[(size_t)i].rid << 32 | (uint32_t)regs[(size_t)i].rs, (uint64_t)i});
	sort_by_x(by_pos);
	for (size_t i = 1; i + 1 < by_pos.size(); ++i) {
		Reg &mid = regs[by_pos[i].y];
		if (mid.inv) mid.mapq = std::min(regs[by_pos[i - 1].y].mapq, regs[by_pos[i + 1].y].mapq);
	}
}

static inline float log2_approx(float x) // mmpriv.h:118-126 (valid for x >= 2)
{
	union { float f; uint32_t i; } z = { x };
	float r = (float)(((z.i >> 23) & 255) - 128);
	z.i &= ~(255u << 23);
	z.i += 127u << 23;
	r += (-0.34484843f * z.f + 2.02466578f) * z.f - 0.67487759f;
	return r;
}

// Re-scale dp_max of all regions of a query by the divergence of its best one (align.c:897-960).  The operation lists supply the
// gap lengths in order (the reference's double accumulation is order-bound).
void rescale_dp_max(int qlen, std::vector<Reg> &regs, float frac, int a, int b)
{
	if (regs.size() < 2) return;
	int best = -1, top = -1, second = -1;
	for (int i = 0; i < (int)regs.size(); ++i) {
		const Reg &r = regs[(size_t)i];
		if (!r.has_p) continue;
		if (r.dp_max > top) second = top, top = r.dp_max, best = i;
		else if (r.dp_max > second) second = r.dp_max;
	}
	if (best < 0 || top < 0 || second < 0) return;
	const Reg &lead = regs[(size_t)best];
	if (lead.qe - lead.qs < (double)qlen * frac || second < (double)top * frac) return;
	int32_t n_open = 0, n_base = 0;
	for (uint32_t c : lead.cigar) { const uint32_t op = c & 0xf; if (op == 1 || op == 2) ++n_open, n_base += (int32_t)(c >> 4); }
	const double identity = (double)lead.mlen / (lead.blen + (int32_t)lead.n_ambi - n_base + n_open);     // mm_event_identity
	double div = 1. - identity;
	if (div < 0.02) div = 0.02;
	double b2 = 0.5 / div;
	if (b2 * a < b) b2 = (double)a / b;
	for (Reg &r : regs) {
		if (!r.has_p) continue;
		double gap_cost = 0.0; int32_t gap_bases = 0;
		for (uint32_t c : r.cigar) { const uint32_t op = c & 0xf; if (op == 1 || op == 2) { gap_cost += b2 + (double)log2_approx((float)(1.0 + (c >> 4))); gap_bases += (int32_t)(c >> 4); } }
		const int32_t n_mis = r.blen + (int32_t)r.n_ambi - r.mlen - gap_bases;
		r.dp_max = std::max(0, (int32_t)(a * (r.mlen - b2 * n_mis - gap_cost) + .499));
	}
}

} // namespace pga
