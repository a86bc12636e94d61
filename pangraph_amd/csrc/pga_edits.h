// pga_edits.h -- host arithmetic over pangraph edit lists that more than one entry needs (pga_reconsensus.hip, pga_promise.hip):
// BandParameters::from_edits and the list-order rules of Edit::apply (reference: packages/pangraph/src/pangraph/edits.rs).
#pragma once
#include "../../include/pga_align.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <utility>
#include <vector>

namespace pga {

// a PREPARED edit list (see prepare_edit): deletions as merged intervals with the count of deleted positions before each, insertions
// sorted by (position, letters) with the count of inserted letters before each
struct RcDelIv { uint32_t start, end, before; };
struct RcInsP { uint32_t pos, len, before; uint64_t seq_off; };

static int64_t aligned_count_after(const std::vector<pga_del_t> &dels, uint32_t p, uint32_t cons_len)     // edits.rs:418-440
{
	const int64_t total = cons_len > p ? (int64_t)cons_len - p : 0;
	int64_t overlap = 0;
	for (const pga_del_t &d : dels) if ((uint64_t)d.pos + d.len > p) overlap += (int64_t)((uint64_t)d.pos + d.len) - std::max<int64_t>(p, d.pos);
	return std::max<int64_t>(total - overlap, 0);
}
// BandParameters::from_edits (map_variations.rs:29-37) = (Edit::aln_mean_shift, Edit::aln_bandwidth), edits.rs:442-531; false: no aligned position
static bool band_from_edits(const std::vector<pga_del_t> &dels, const std::vector<std::pair<uint32_t, uint32_t>> &inss /* (pos, len) in list order */, uint32_t cons_len, int64_t &ms, int64_t &bw)
{
	const int64_t ac = aligned_count_after(dels, 0, cons_len);
	if (ac == 0) return false;
	int64_t total = 0;
	for (auto &x : inss) total -= (int64_t)x.second * aligned_count_after(dels, x.first, cons_len);
	for (const pga_del_t &d : dels) total += (int64_t)d.len * aligned_count_after(dels, d.pos, cons_len);
	ms = (int64_t)std::llround((double)total / (double)ac);              // f64::round: half away from zero
	std::vector<std::pair<uint32_t, int64_t>> tp;
	for (auto &x : inss) tp.emplace_back(x.first, -(int64_t)x.second);
	for (const pga_del_t &d : dels) tp.emplace_back(d.pos, (int64_t)d.len);
	std::stable_sort(tp.begin(), tp.end(), [](const std::pair<uint32_t, int64_t> &a, const std::pair<uint32_t, int64_t> &b) { return a.first < b.first; });
	bw = 0; int64_t cur = 0;
	for (size_t i = 0; i < tp.size(); ++i) {
		if (i == 0 && tp[i].first > 0) bw = std::max<int64_t>(bw, std::llabs(cur - ms));
		cur += tp[i].second;
		if (i + 1 == tp.size() && (tp[i].first == cons_len || (tp[i].second > 0 && (int64_t)tp[i].first + tp[i].second == (int64_t)cons_len))) continue;
		bw = std::max<int64_t>(bw, std::llabs(cur - ms));
	}
	return true;
}

// prepared lists of one edit (for k_rc_apply); returns the length of the applied sequence
struct PreparedEdit { std::vector<pga_sub_t> subs; std::vector<RcDelIv> dels; std::vector<RcInsP> inss; };
static uint32_t prepare_edit(const pga_sub_t *subs, uint32_t n_subs, const pga_del_t *dels, uint32_t n_dels, const pga_ins_t *inss, uint32_t n_inss, const char *ins_seq, uint32_t cons_len, PreparedEdit &P)
{
	P.subs.assign(subs, subs + n_subs);
	std::stable_sort(P.subs.begin(), P.subs.end(), [](const pga_sub_t &a, const pga_sub_t &b) { return a.pos < b.pos; });
	std::vector<std::pair<uint32_t, uint32_t>> iv;
	for (uint32_t t = 0; t < n_dels; ++t) if (dels[t].len) iv.emplace_back(dels[t].pos, dels[t].pos + dels[t].len);
	std::sort(iv.begin(), iv.end());
	P.dels.clear();
	uint32_t before = 0;
	for (auto &x : iv) {
		if (!P.dels.empty() && x.first <= P.dels.back().end) { if (x.second > P.dels.back().end) { before += x.second - P.dels.back().end; P.dels.back().end = x.second; } continue; }
		P.dels.push_back(RcDelIv{x.first, x.second, before});
		before += x.second - x.first;
	}
	std::vector<uint32_t> ord(n_inss); std::iota(ord.begin(), ord.end(), 0u);
	std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {       // Ins: Ord by (pos, seq), edits.rs:321 `sorted()`
		if (inss[a].pos != inss[b].pos) return inss[a].pos < inss[b].pos;
		const uint32_t la = inss[a].len, lb = inss[b].len; const int c = memcmp(ins_seq + inss[a].seq_off, ins_seq + inss[b].seq_off, std::min(la, lb));
		return c != 0 ? c < 0 : la < lb; });
	P.inss.clear();
	uint32_t ib = 0;
	for (uint32_t o : ord) { P.inss.push_back(RcInsP{inss[o].pos, inss[o].len, ib, inss[o].seq_off}); ib += inss[o].len; }
	return cons_len - before + ib;
}

} // namespace pga
