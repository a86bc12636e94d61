// pga_runs.h -- a member sequence as a chain of RUNS, and the complement table: what the entries that build sequences on the device from a
// consensus and an edit list share (pga_promise.hip: the members of a merge promise; pga_rows.h: the pieces of a row -- the nodes of a path for
// pga_reconstruct.hip, the pieces of an exported row for pga_export.hip), and the host threads their list bookkeeping runs on.
#pragma once
#include "pga_edits.h"
#include <exception>
#include <thread>

namespace pga {

// f(t, a, z) over [0, n) in contiguous ranges on a few host threads (range t is the t-th in order; under 64 items: inline, as range 0);
// exceptions are passed on
static inline int range_threads() { return (int)std::min<unsigned>(8, std::max(1u, std::thread::hardware_concurrency())); }
template <class F> static void thread_ranges(uint64_t n, int n_threads, F f)
{
	if (n < 64 || n_threads <= 1) { f(0, (uint64_t)0, n); return; }
	const uint64_t per = (n + (uint64_t)n_threads - 1) / (uint64_t)n_threads;
	std::vector<std::thread> th; std::vector<std::exception_ptr> err((size_t)n_threads);
	for (int t = 0; t < n_threads; ++t) th.emplace_back([&, t]() { try { f(t, std::min(n, per * t), std::min(n, per * (t + 1))); } catch (...) { err[t] = std::current_exception(); } });
	for (auto &x : th) x.join();
	for (auto &e : err) if (e) std::rethrow_exception(e);
}

// io/seq.rs:9-29: ACGTYRWSKMDVHBN- and nothing else (0: rejected; lower case is rejected)
struct CompTable { uint8_t t[256]; };
constexpr CompTable make_comp_table()
{
	CompTable c{};
	const char from[] = "ACGTYRWSKMDVHBN-", to[] = "TGCARYWSMKHBDVN-";
	for (int i = 0; i < 16; ++i) c.t[(unsigned char)from[i]] = (uint8_t)to[i];
	return c;
}
static constexpr CompTable h_comp = make_comp_table();
static __constant__ CompTable d_comp = make_comp_table();            // (one copy per translation unit that includes this)

// one run of a member sequence: built letters [out, out of the next run) come from cons[src ..] (kind 0), ins_seq[src ..] (kind 1) or
// are the one letter `src` (kind 2)
struct PrSeg { uint32_t out, kind; uint64_t src; };

// the runs of one prepared edit over a consensus of cons_len letters that starts at cons_base; returns the built length
static uint32_t promise_segments(const PreparedEdit &P, uint32_t cons_len, uint64_t cons_base, uint64_t ins_base, std::vector<PrSeg> &out)
{
	uint32_t o = 0, p = 0;
	size_t ii = 0, di = 0, si = 0;
	auto copy_run = [&](uint32_t from, uint32_t to) {                     // consensus positions [from, to): none deleted, no insertion inside
		while (si < P.subs.size() && P.subs[si].pos < from) ++si;           // substitutions of deleted positions
		uint32_t q = from;
		while (q < to) {
			const uint32_t sp = si < P.subs.size() && P.subs[si].pos < to ? P.subs[si].pos : to;
			if (sp > q) { out.push_back(PrSeg{o, 0u, cons_base + q}); o += sp - q; q = sp; }
			if (q < to) {
				while (si + 1 < P.subs.size() && P.subs[si + 1].pos == q) ++si;   // the last of equal positions wins (edits.rs:310-312)
				out.push_back(PrSeg{o, 2u, (uint64_t)(P.subs[si].alt & 255u)}); ++o; ++q; ++si;
			}
		}
	};
	for (;;) {
		for (; ii < P.inss.size() && P.inss[ii].pos == p; ++ii) if (P.inss[ii].len) { out.push_back(PrSeg{o, 1u, P.inss[ii].seq_off - ins_base}); o += P.inss[ii].len; }
		if (p >= cons_len) break;
		const uint32_t next = ii < P.inss.size() ? std::min(P.inss[ii].pos, cons_len) : cons_len;
		while (p < next) {
			while (di < P.dels.size() && P.dels[di].end <= p) ++di;
			if (di < P.dels.size() && P.dels[di].start <= p) { p = std::min(P.dels[di].end, next); continue; }
			const uint32_t stop = di < P.dels.size() ? std::min(P.dels[di].start, next) : next;
			copy_run(p, stop); p = stop;
		}
	}
	return o;
}

// Edit::apply_aligned (edits.rs:331-347) as runs: besides PrSeg's kinds a GAP run (kind 3: n times '-', no source).  Over the prepared edit:
// consensus runs, one-letter runs for the substitutions that survive (none under a deletion; of equal positions the last in list order,
// which prepare_edit's stable sort keeps), one gap run per merged deletion interval; insertions are ignored.  Returns the built length,
// counted run by run: the caller checks it against cons_len.
constexpr uint32_t PR_GAP = 3;
static uint32_t aligned_segments(const PreparedEdit &P, uint32_t cons_len, uint64_t cons_base, std::vector<PrSeg> &out)
{
	uint32_t o = 0, p = 0;
	size_t di = 0, si = 0;
	while (p < cons_len) {
		while (di < P.dels.size() && P.dels[di].end <= p) ++di;
		if (di < P.dels.size() && P.dels[di].start <= p) {                  // (merged intervals: the next one starts behind this one's end)
			const uint32_t end = std::min(P.dels[di].end, cons_len);
			out.push_back(PrSeg{o, PR_GAP, 0u}); o += end - p; p = end;
			continue;
		}
		const uint32_t stop = di < P.dels.size() ? std::min(P.dels[di].start, cons_len) : cons_len;
		while (si < P.subs.size() && P.subs[si].pos < p) ++si;              // substitutions of deleted positions
		while (p < stop) {
			const uint32_t sp = si < P.subs.size() && P.subs[si].pos < stop ? P.subs[si].pos : stop;
			if (sp > p) { out.push_back(PrSeg{o, 0u, cons_base + p}); o += sp - p; p = sp; }
			if (p < stop) {
				while (si + 1 < P.subs.size() && P.subs[si + 1].pos == p) ++si;   // the last of equal positions wins (edits.rs:336-338)
				out.push_back(PrSeg{o, 2u, (uint64_t)(P.subs[si].alt & 255u)}); ++o; ++p; ++si;
			}
		}
	}
	return o;
}

} // namespace pga
