// pga_reweave.hip -- the front half of reweave (packages/pangraph/src/pangraph/reweave.rs:132-340, 408-443 over pangraph_interval.rs:98-255 and
// align/bam/cigar.rs:26-96) for all merges of a tree level: filtered matches in; new block ids, anchor decisions, the refined interval table
// of every block with a hit (what pga_slice_blocks takes) and the promises with their CIGARs (what pga_solve_promises takes) out.  The
// reference walks block after block, clones every alignment twice and edits CIGARs operation by operation; here a MATCH, a HIT and a PROMISE
// are the units, and every rule is a test on a record and its two neighbours in a sorted list.
//   host              validation and the block / match tables (rw_build_tables); the letters route's intervals into pinned staging
//   k_rw_mask         one wave per side of an equal-depth match: popcount of the batch's "not ACGT" plane over the interval
//   k_rw_letters      one wave per side that needs letters: bytes equal to 'N', 16 per lane and turn
//   k_rw_match        one thread per match: anchor and route, XXH64 id, two hit keys (block rank, start), the promise key
//   rocPRIM           hits by key; promises by id, then stably by group (the route of pga_filter.hip for lists of this size)
//   k_rw_hits         one thread per sorted hit: the intervals it owns before and after refinement, its extensions, its error code
//   rocPRIM           two exclusive sums over the hits
//   k_rw_intervals    one thread per sorted hit: its refined intervals (gap ids hashed here), the slice table, the blocks' ends and errors
//   k_rw_blocks       one thread per block with a hit: its record
//   k_rw_cigar_plan   one thread per promise: update_cigar's at most four flanks as a plan, the output length
//   rocPRIM           exclusive sum of the lengths
//   k_rw_cigar_write  one wave per promise: operations copied (forward, or reversed and I <-> D), lengthened or inserted per plan; the record
// Everything is queued on one stream and the call waits once.  With a batch, the matches whose bit plane is not empty are known only after
// that wait: their letters are staged, counted, and the lists are built a second time.  The index arithmetic is pga_reweave_idx.h.
#include "pga_common.h"
#include "pga_graph_host.h"
#include "../../include/pga_align.h"
#include "pga_reweave_idx.h"
#include "pga_runs.h"

namespace pga {

static unsigned rw_grid(uint64_t items, uint64_t per_block) { return grid_for(items, per_block, 2048); }
static int rw_bits(uint64_t n) { int b = 1; while (b < 64 && (n >> b)) ++b; return b; }

void plan_merge_host(int32_t n_groups, const int64_t *group_off, const pga_plan_block_t *blocks, int64_t n_matches, const pga_match_t *matches, const uint32_t *cigars,
                     uint64_t n_ops, uint32_t thr_len, const RwResident *res, pga_plan_out_t *out)
{
	auto fail = [](const std::string &what) { throw std::runtime_error("pga_plan_merge: " + what); };
	// ---- validation and tables: everything the host can refuse is refused here ----
	RwTables T;
	rw_build_tables(n_groups, group_off, blocks, n_matches, matches, cigars, n_ops, res, T);
	if (n_matches == 0) return;
	const uint64_t nm = (uint64_t)n_matches, nh = 2 * nm, n_hb = T.hb_block.size(), nb = T.blk.size();
	const uint64_t cap_iv = 2 * nh + n_hb, cap_cig = T.cigar_in + 4 * nm;
	out->matches = host_array<pga_plan_match_t>(nm, "pga_plan_merge");
	out->blocks = host_array<pga_plan_block_res_t>(n_hb, "pga_plan_merge");
	out->intervals = host_array<pga_plan_interval_t>(cap_iv, "pga_plan_merge");
	out->slice_intervals = host_array<pga_slice_interval_t>(cap_iv, "pga_plan_merge");
	out->promises = host_array<pga_plan_promise_t>(nm, "pga_plan_merge");
	out->cigars = host_array<uint32_t>(cap_cig, "pga_plan_merge");
	// ---- the device ----
	StreamLease stream;
	hipStream_t st = stream.s;
	DBuf<RwBlk> d_blk(nb); DBuf<RwMatch> d_mt(nm); DBuf<uint32_t> d_cig(n_ops + 1), d_ncnt(nh);
	DBuf<pga_plan_match_t> d_omatch(nm);
	DBuf<rw_u64> d_hkey(nh), d_hkey2(nh), d_pkey(nm), d_pkey2(nm);
	DBuf<uint32_t> d_hval(nh), d_hs(nh), d_pval(nm), d_byid(nm), d_pgrp(nm), d_pgrp2(nm), d_pm(nm);
	DBuf<uint32_t> d_cntb(nh + 1), d_cnta(nh + 1), d_herr(nh + 1), d_offb(nh + 1), d_offa(nh + 1);
	DBuf<RwExt> d_ext(nh); DBuf<rw_u64> d_ivof(nh), d_bfirst(n_hb), d_bfirstb(n_hb), d_bend(n_hb), d_berr(n_hb);
	DBuf<pga_plan_block_res_t> d_oblk(n_hb); DBuf<pga_plan_interval_t> d_oiv(cap_iv); DBuf<pga_slice_interval_t> d_osiv(cap_iv);
	DBuf<RwPlan> d_plan(nm); DBuf<rw_u64> d_nout(nm + 1), d_coff(nm + 1);
	DBuf<pga_plan_promise_t> d_oprom(nm); DBuf<uint32_t> d_ocig(cap_cig + 1);
	DBuf<rw_u64> d_counters(RW_COUNTERS); DBuf<uint32_t> d_err(4);
	PGA_HIP(hipMemcpyAsync(d_blk.p, T.blk.data(), nb * sizeof(RwBlk), hipMemcpyHostToDevice, st));
	if (n_ops) PGA_HIP(hipMemcpyAsync(d_cig.p, cigars, n_ops * sizeof(uint32_t), hipMemcpyHostToDevice, st));
	d_ncnt.zero(st);
	RwDev V;
	V.n_matches = nm; V.n_hits = nh; V.n_hb = n_hb; V.cap_iv = cap_iv; V.cap_cig = cap_cig; V.thr_len = thr_len; V.pad = 0;
	V.blk = d_blk.p; V.mt = d_mt.p; V.cig = d_cig.p; V.ncnt = d_ncnt.p; V.o_match = d_omatch.p;
	V.hkey = d_hkey.p; V.hval = d_hval.p; V.pkey = d_pkey.p; V.pval = d_pval.p; V.pgrp = d_pgrp.p; V.hs = d_hs.p;
	V.cnt_b = d_cntb.p; V.cnt_a = d_cnta.p; V.herr = d_herr.p; V.off_b = d_offb.p; V.off_a = d_offa.p; V.ext = d_ext.p; V.iv_of = d_ivof.p;
	V.b_first = d_bfirst.p; V.b_firstb = d_bfirstb.p; V.b_end = d_bend.p; V.b_err = d_berr.p; V.o_blk = d_oblk.p; V.o_iv = d_oiv.p; V.o_siv = d_osiv.p;
	V.pm = d_pm.p; V.plan = d_plan.p; V.n_out = d_nout.p; V.c_off = d_coff.p; V.o_prom = d_oprom.p; V.o_cig = d_ocig.p;
	V.counters = d_counters.p; V.err = d_err.p;

	// the letters route: the intervals of `sides` (two per match of `which`) packed into pinned staging, each at a multiple of 16
	PinVec<uint8_t> stage; std::vector<RwJob> jobs; DBuf<uint8_t> d_stage; DBuf<RwJob> d_jobs;
	auto stage_letters = [&](const std::vector<uint32_t> &which) {
		jobs.clear();
		uint64_t bytes = 0;
		for (uint32_t m : which) for (uint32_t s = 0; s < 2; ++s) {
			const RwMatch &M = T.mt[m];
			jobs.push_back(RwJob{bytes, 2 * m + s, M.end[s] - M.start[s]});
			bytes += ((uint64_t)(M.end[s] - M.start[s]) + 15) & ~15ULL;
		}
		stage.resize((size_t)bytes);
		thread_ranges(jobs.size(), range_threads(), [&](int, uint64_t j0, uint64_t j1) {
			for (uint64_t j = j0; j < j1; ++j) {
				const RwJob &J = jobs[j]; const RwMatch &M = T.mt[J.side >> 1]; const uint32_t s = J.side & 1;
				memcpy(stage.data() + J.off, blocks[M.blk[s]].consensus + M.start[s], J.len);
				memset(stage.data() + J.off + J.len, 0, (size_t)((16 - (J.len & 15)) & 15));
			}
		});
		for (uint32_t m : which) T.mt[m].letters = 1;
		d_stage.alloc((size_t)bytes + 16); d_jobs.alloc(jobs.size() + 1);
		if (bytes) PGA_HIP(hipMemcpyAsync(d_stage.p, stage.data(), (size_t)bytes, hipMemcpyHostToDevice, st));
		PGA_HIP(hipMemcpyAsync(d_jobs.p, jobs.data(), jobs.size() * sizeof(RwJob), hipMemcpyHostToDevice, st));
	};
	const bool resident = res != nullptr;
	std::vector<uint32_t> sides; DBuf<uint32_t> d_sides;                            // the mask route: both sides of every equal-depth match
	if (!resident && !T.eq.empty()) stage_letters(T.eq);
	if (resident && !T.eq.empty()) {
		sides.reserve(2 * T.eq.size());
		for (uint32_t m : T.eq) { sides.push_back(2 * m); sides.push_back(2 * m + 1); }
		d_sides.upload(sides, st);
	}

	std::vector<uint32_t> h_ncnt; rw_u64 counters[RW_COUNTERS]; uint32_t err[4]; rw_u64 tot_b = 0, tot_a = 0, tot_c = 0;
	for (int pass = 0; pass < 2; ++pass) {
		PGA_HIP(hipMemcpyAsync(d_mt.p, T.mt.data(), nm * sizeof(RwMatch), hipMemcpyHostToDevice, st));
		d_counters.zero(st); d_err.zero(st);
		PGA_HIP(hipMemsetAsync(d_berr.p, 0xff, n_hb * sizeof(rw_u64), st));
		if (pass == 0 && resident && !T.eq.empty())
			hipLaunchKernelGGL(k_rw_mask, dim3(rw_grid(sides.size(), RW_WAVES)), dim3(RW_THREADS), 0, st, V, (const uint32_t*)d_sides.p, (uint64_t)sides.size());
		if (!jobs.empty()) hipLaunchKernelGGL(k_rw_letters, dim3(rw_grid(jobs.size(), RW_WAVES)), dim3(RW_THREADS), 0, st, V, (const RwJob*)d_jobs.p, (uint64_t)jobs.size(), (const RwV4*)d_stage.p);
		hipLaunchKernelGGL(k_rw_match, dim3(rw_grid(nm, RW_THREADS)), dim3(RW_THREADS), 0, st, V);
		radix_sort_pairs(d_hkey.p, d_hkey2.p, d_hval.p, d_hs.p, nh, 32 + rw_bits(nb), st);
		radix_sort_pairs(d_pkey.p, d_pkey2.p, d_pval.p, d_byid.p, nm, 64, st);
		hipLaunchKernelGGL(k_rw_groups, dim3(rw_grid(nm, RW_THREADS)), dim3(RW_THREADS), 0, st, V, (const uint32_t*)d_byid.p);
		radix_sort_pairs(d_pgrp.p, d_pgrp2.p, d_byid.p, d_pm.p, nm, rw_bits(T.n_groups), st);
		hipLaunchKernelGGL(k_rw_hits, dim3(rw_grid(nh + 1, RW_THREADS)), dim3(RW_THREADS), 0, st, V);
		excl_scan(d_cntb.p, d_offb.p, nh + 1, st);
		excl_scan(d_cnta.p, d_offa.p, nh + 1, st);
		hipLaunchKernelGGL(k_rw_intervals, dim3(rw_grid(nh, RW_THREADS)), dim3(RW_THREADS), 0, st, V);
		hipLaunchKernelGGL(k_rw_blocks, dim3(rw_grid(n_hb, RW_THREADS)), dim3(RW_THREADS), 0, st, V);
		hipLaunchKernelGGL(k_rw_cigar_plan, dim3(rw_grid(nm + 1, RW_THREADS)), dim3(RW_THREADS), 0, st, V);
		excl_scan(d_nout.p, d_coff.p, nm + 1, st);
		hipLaunchKernelGGL(k_rw_cigar_write, dim3(rw_grid(nm, RW_WAVES)), dim3(RW_THREADS), 0, st, V);
		PGA_HIP(hipGetLastError());
		// ---- the one wait ----
		{
			Downloads dl(st);
			if (pass == 0 && resident) dl.add(h_ncnt, d_ncnt.p, nh);
			uint32_t tb = 0, ta = 0;
			PGA_HIP(hipMemcpyAsync(counters, d_counters.p, sizeof(counters), hipMemcpyDeviceToHost, st));
			PGA_HIP(hipMemcpyAsync(err, d_err.p, sizeof(err), hipMemcpyDeviceToHost, st));
			PGA_HIP(hipMemcpyAsync(&tb, d_offb.p + nh, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
			PGA_HIP(hipMemcpyAsync(&ta, d_offa.p + nh, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
			PGA_HIP(hipMemcpyAsync(&tot_c, d_coff.p + nm, sizeof(rw_u64), hipMemcpyDeviceToHost, st));
			PGA_HIP(hipMemcpyAsync(out->matches, d_omatch.p, nm * sizeof(pga_plan_match_t), hipMemcpyDeviceToHost, st));
			PGA_HIP(hipMemcpyAsync(out->blocks, d_oblk.p, n_hb * sizeof(pga_plan_block_res_t), hipMemcpyDeviceToHost, st));
			PGA_HIP(hipMemcpyAsync(out->intervals, d_oiv.p, cap_iv * sizeof(pga_plan_interval_t), hipMemcpyDeviceToHost, st));
			PGA_HIP(hipMemcpyAsync(out->slice_intervals, d_osiv.p, cap_iv * sizeof(pga_slice_interval_t), hipMemcpyDeviceToHost, st));
			PGA_HIP(hipMemcpyAsync(out->promises, d_oprom.p, nm * sizeof(pga_plan_promise_t), hipMemcpyDeviceToHost, st));
			if (cap_cig) PGA_HIP(hipMemcpyAsync(out->cigars, d_ocig.p, cap_cig * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
			dl.wait();
			PGA_HIP(sync_stream(st));
			tot_b = tb; tot_a = ta;
		}
		if (counters[RW_C_UNDECIDED] == 0) break;
		if (pass == 1) fail("internal: matches undecided after the letters pass");
		// the bit plane is an upper bound: these matches need their letters, then everything behind the decision is built again
		std::vector<uint32_t> need;
		for (uint32_t m : T.eq) if (h_ncnt[2 * (size_t)m] | h_ncnt[2 * (size_t)m + 1]) need.push_back(m);
		if (need.size() != counters[RW_C_UNDECIDED]) fail("internal: the device and the host disagree on the matches that need letters");
		stage_letters(need);
	}
	if (err[0]) {
		const uint64_t where = (uint64_t)err[1] | (uint64_t)err[2] << 32;
		switch (err[0]) {
		case RW_ERR_OVERLAP: fail("two hits on one block overlap (sorted hit " + std::to_string(where) + ")");
		case RW_ERR_DUP_ID: fail("two matches of a group have the same new block id (match " + std::to_string(where) + ")");
		case RW_ERR_OP_LEN: fail("a CIGAR operation would reach 2^28 after a flank (match " + std::to_string(where) + ")");
		default: fail("Unexpected CIGAR operation in a match (match " + std::to_string(where) + ")");
		}
	}
	if (tot_b > cap_iv || tot_a > cap_iv || tot_c > cap_cig) fail("internal: the device counted more than the lists hold");
	// ---- the record of the call ----
	out->n_matches = n_matches; out->n_blocks = (int64_t)n_hb; out->n_failed = (int64_t)counters[RW_C_FAILED];
	for (uint64_t b = 0; b < n_hb; ++b) out->blocks[b].block = T.hb_block[b];
	pga_plan_counters_t &C = out->counters;
	C.by_depth = counters[RW_C_DEPTH]; C.by_mask = counters[RW_C_MASK]; C.by_letters = counters[RW_C_LETTERS]; C.hits = nh;
	C.intervals_before = tot_b; C.cigar_in = T.cigar_in;
	if (out->n_failed) {
		free(out->intervals); free(out->slice_intervals); free(out->promises); free(out->cigars);
		out->intervals = nullptr; out->slice_intervals = nullptr; out->promises = nullptr; out->cigars = nullptr;
		for (uint64_t b = 0; b < n_hb; ++b) { out->blocks[b].first_interval = 0; out->blocks[b].n_intervals = 0; }
		return;
	}
	out->n_intervals = (int64_t)tot_a; out->n_promises = n_matches; out->n_cigar = tot_c;
	C.intervals_after = tot_a; C.cigar_out = tot_c;
}

} // namespace pga
