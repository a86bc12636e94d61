// pga_merge.hip -- the block concatenations of `pangraph simplify` (commands/simplify/simplify_run.rs:23-38 over circularize/circularize.rs:11-76):
// merge_blocks.rs:92-148 merge_alignment / concatenate_alignments for any number of independent edges in one call, over
// PangraphBlock::reverse_complement (pangraph_block.rs:63-75) and Edit::{reverse_complement, shift, concat} (edits.rs:257-304).
// The reference merges one transitive edge at a time, walks every node of every path for each, and clones, complements and re-sorts whole
// blocks for one concatenation.  Here a batch of disjoint edges is one call; an OUTPUT MEMBER (edge, k) is the unit of work.
//   host              validation (all of it before anything is launched), O(edits + members): the member table (two sides per output
//                     member), every input member's running insertion lengths, the row jobs; one upload of every list
//   k_merge_lists     one wave per output member, lanes over entries: which lists are not the reversed list after *_rc (or hold right
//                     insertions at one position), the first left' insertion at L_left, what the right' insertions at 0 hold
//   k_merge_count     the number of output insertions; for the rare lists above every right insertion's leader (quadratic for those only)
//   k_merge_scan      ONE wave: exclusive sums of the output insertion counts in member order (the one kernel with wave intrinsics)
//   k_merge_write     one wave per output member, lanes over SOURCE entries: mapped position, shift, place in the primed list (identity,
//                     reversed, or the exact stable rank), `alt` through the complement table, the insertion merge rule, and per source
//                     insertion the run of its letters in the member's row
//   k_rows<false>     (pga_rows.h) the letters: one row per output consensus (two runs), one per output member's inserted letters
// The list kernels and the tables are pga_merge_idx.h (no wave intrinsic: tests/emu/merge_emu.cpp runs them on the host).
// All arithmetic is integer; atomics feed only sums, counts, minima and flags, so the result does not depend on the launch geometry.
#include "pga_common.h"
#include "pga_graph_host.h"
#include "pga_wave.h"
#include "../../include/pga_align.h"
#include "pga_merge_idx.h"

namespace pga {

// ONE wave: ins_off[o] = the output insertions of the members before o; ins_off[n] = their total
__global__ __launch_bounds__(64) void k_merge_scan(const uint32_t *n_ins, uint64_t n, mg_u64 *ins_off)
{
	const uint32_t lane = threadIdx.x;
	mg_u64 run = 0;
	for (uint64_t c0 = 0; c0 < n; c0 += 64) {
		const uint64_t o = c0 + lane;
		const mg_u64 v = o < n ? (mg_u64)n_ins[o] : 0ULL, in = wave_incl_u64(v, lane);
		if (o < n) ins_off[o] = run + in - v;
		run += __shfl(in, 63);
	}
	if (lane == 0) ins_off[n] = run;
}

static unsigned mg_grid(uint64_t items, uint64_t per_block) { return grid_for(items, per_block, 1u << 16); }

void merge_blocks_host(int64_t n_blocks, const pga_rc_block_t *blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss,
                       const char *ins_seq, int64_t n_edges, const pga_merge_edge_t *edges, const uint32_t *partner, pga_merge_out_t *out)
{
	auto fail = [](const std::string &what) { throw std::runtime_error("pga_merge_blocks: " + what); };
	// ---- validation and tables: everything that fails the call does so here ----
	RowGraph G;
	row_graph_init(G, "pga_merge_blocks", n_blocks, blocks, members, subs, dels, inss, ins_seq, true, 1);
	MgTables T;
	mg_build_tables(G, n_edges, edges, partner, T);
	const uint64_t n_mem = T.mem.size(), n_jobs = T.jobs.size();
	out->edges = host_array<pga_merge_res_t>((uint64_t)n_edges, "pga_merge_blocks");
	out->blocks = host_array<pga_rc_block_t>((uint64_t)n_edges, "pga_merge_blocks");
	out->members = host_array<pga_rc_member_t>(n_mem, "pga_merge_blocks");
	out->subs = host_array<pga_sub_t>(T.n_sub, "pga_merge_blocks"); out->dels = host_array<pga_del_t>(T.n_del, "pga_merge_blocks");
	const uint64_t cons_bytes = T.cons_units * ROW_LETTERS, ins_bytes = (T.units - T.cons_units) * ROW_LETTERS;
	out->cons = host_array<char>(cons_bytes + 1, "pga_merge_blocks"); out->ins_seq = host_array<char>(ins_bytes + 1, "pga_merge_blocks");
	for (int64_t e = 0; e < n_edges; ++e) {
		out->edges[e].member_off = T.member_off[e];
		out->blocks[e].consensus = out->cons + T.cons_off[e];
		out->blocks[e].cons_len = blocks[edges[e].left].cons_len + blocks[edges[e].right].cons_len;
		out->blocks[e].n_members = blocks[edges[e].left].n_members;
	}
	if (n_edges == 0 || (n_mem == 0 && n_jobs == 0)) { out->inss = host_array<pga_ins_t>(0, "pga_merge_blocks"); return; }   // (only empty blocks: nothing to build)
	// ---- the device ----
	StreamLease stream;
	hipStream_t st = stream.s;
	const uint64_t n_sub_in = G.sub_off[G.n_mem], n_del_in = G.del_off[G.n_mem], n_ins_in = G.ins_off[G.n_mem];
	DBuf<MgMem> d_mem(n_mem + 1);
	if (n_mem) PGA_HIP(hipMemcpyAsync(d_mem.p, T.mem.data(), n_mem * sizeof(MgMem), hipMemcpyHostToDevice, st));
	DBuf<pga_sub_t> d_subs(n_sub_in + 1); DBuf<pga_del_t> d_dels(n_del_in + 1); DBuf<pga_ins_t> d_inss(n_ins_in + 1);
	DBuf<mg_u64> d_cum(T.cum.size() + 1);
	if (n_sub_in) PGA_HIP(hipMemcpyAsync(d_subs.p, subs, n_sub_in * sizeof(pga_sub_t), hipMemcpyHostToDevice, st));
	if (n_del_in) PGA_HIP(hipMemcpyAsync(d_dels.p, dels, n_del_in * sizeof(pga_del_t), hipMemcpyHostToDevice, st));
	if (n_ins_in) PGA_HIP(hipMemcpyAsync(d_inss.p, inss, n_ins_in * sizeof(pga_ins_t), hipMemcpyHostToDevice, st));
	if (!T.cum.empty()) PGA_HIP(hipMemcpyAsync(d_cum.p, T.cum.data(), T.cum.size() * sizeof(mg_u64), hipMemcpyHostToDevice, st));
	DBuf<uint32_t> d_words(3 * n_mem + (uint64_t)n_edges + 1), d_first(n_mem + 1), d_lead(T.n_lead + 1);   // flags | b_cnt | n_ins | edge_bad
	DBuf<mg_u64> d_bsum(n_mem + 1), d_ioff(n_mem + 1);
	d_words.zero(st); d_bsum.zero(st);
	PGA_HIP(hipMemsetAsync(d_first.p, 0xff, (n_mem + 1) * sizeof(uint32_t), st));
	MgDev V;
	V.mem = d_mem.p; V.n_mem = n_mem; V.subs = d_subs.p; V.dels = d_dels.p; V.inss = d_inss.p; V.cum = d_cum.p;
	V.flags = d_words.p; V.b_cnt = d_words.p + n_mem; V.n_ins = d_words.p + 2 * n_mem; V.edge_bad = d_words.p + 3 * n_mem;
	V.first_l = d_first.p; V.b_sum = d_bsum.p; V.lead = d_lead.p; V.ins_off = d_ioff.p;
	uint64_t n_ins_out = 0;
	DBuf<RowRun> d_runs(T.n_runs + 1);
	DBuf<pga_sub_t> d_osubs(T.n_sub + 1); DBuf<pga_del_t> d_odels(T.n_del + 1); DBuf<pga_ins_t> d_oinss;
	if (!T.cons_runs.empty()) PGA_HIP(hipMemcpyAsync(d_runs.p, T.cons_runs.data(), T.cons_runs.size() * sizeof(RowRun), hipMemcpyHostToDevice, st));
	if (n_mem) {
		hipLaunchKernelGGL(k_merge_lists, dim3(mg_grid(n_mem, MG_WAVES)), dim3(MG_THREADS), 0, st, V);
		hipLaunchKernelGGL(k_merge_count, dim3(mg_grid(n_mem, MG_WAVES)), dim3(MG_THREADS), 0, st, V);
		hipLaunchKernelGGL(k_merge_scan, dim3(1), dim3(64), 0, st, V.n_ins, n_mem, d_ioff.p);
		PGA_HIP(hipGetLastError());
		// ---- the one read-back before the write pass: the total sizes the output ----
		mg_u64 tot = 0;
		PGA_HIP(hipMemcpyAsync(&tot, d_ioff.p + n_mem, sizeof(tot), hipMemcpyDeviceToHost, st));
		PGA_HIP(sync_stream(st));
		n_ins_out = tot;
		uint64_t bound = 0;
		for (const MgMem &M : T.mem) bound += (uint64_t)M.s[0].n_ins + M.s[1].n_ins;
		if (n_ins_out > bound) fail("internal: more output insertions than the two sides hold");
		d_oinss.alloc(n_ins_out + 1);
		hipLaunchKernelGGL(k_merge_write, dim3(mg_grid(n_mem, MG_WAVES)), dim3(MG_THREADS), 0, st, V, d_osubs.p, d_odels.p, d_oinss.p, d_runs.p);
		PGA_HIP(hipGetLastError());
	}
	out->inss = host_array<pga_ins_t>(n_ins_out, "pga_merge_blocks");
	// ---- the letters: consensus rows, then the rows of inserted letters, one unit space ----
	const uint64_t il = T.ins_lo < T.ins_hi ? T.ins_lo : 0, ih = T.ins_lo < T.ins_hi ? T.ins_hi : 0;
	DBuf<char> d_cons(T.cons.size() + 16), d_iseq(ih - il + 16), d_out(T.units * ROW_LETTERS + 16);
	DBuf<RowJob> d_jobs(n_jobs + 1); DBuf<uint32_t> d_flags(n_jobs + 1);
	std::vector<uint32_t> j_flags, e_bad, m_nins;
	if (n_jobs) {
		if (!T.cons.empty()) PGA_HIP(hipMemcpyAsync(d_cons.p, T.cons.data(), T.cons.size(), hipMemcpyHostToDevice, st));
		if (ih > il) PGA_HIP(hipMemcpyAsync(d_iseq.p, ins_seq + il, ih - il, hipMemcpyHostToDevice, st));
		PGA_HIP(hipMemcpyAsync(d_jobs.p, T.jobs.data(), n_jobs * sizeof(RowJob), hipMemcpyHostToDevice, st));
		d_flags.zero(st);
		const unsigned grid = (unsigned)std::min<uint64_t>((T.units + ROW_THREADS - 1) / ROW_THREADS, 2048);
		hipLaunchKernelGGL(k_rows<false>, dim3(grid), dim3(ROW_THREADS), 0, st, d_jobs.p, (int)n_jobs, (uint64_t)0, T.units, d_runs.p, d_cons.p, d_iseq.p, il,
		                   d_out.p, d_flags.p, 0u, (const char*)nullptr, (unsigned long long*)nullptr, (unsigned long long*)nullptr);
		PGA_HIP(hipGetLastError());
	}
	{
		Downloads dl(st);
		if (n_jobs) dl.add(j_flags, d_flags.p, n_jobs);
		dl.add(e_bad, V.edge_bad, (size_t)n_edges);
		if (n_mem) dl.add(m_nins, V.n_ins, n_mem);
		if (cons_bytes) PGA_HIP(hipMemcpyAsync(out->cons, d_out.p, cons_bytes, hipMemcpyDeviceToHost, st));
		if (ins_bytes) PGA_HIP(hipMemcpyAsync(out->ins_seq, d_out.p + cons_bytes, ins_bytes, hipMemcpyDeviceToHost, st));
		if (T.n_sub) PGA_HIP(hipMemcpyAsync(out->subs, d_osubs.p, T.n_sub * sizeof(pga_sub_t), hipMemcpyDeviceToHost, st));
		if (T.n_del) PGA_HIP(hipMemcpyAsync(out->dels, d_odels.p, T.n_del * sizeof(pga_del_t), hipMemcpyDeviceToHost, st));
		if (n_ins_out) PGA_HIP(hipMemcpyAsync(out->inss, d_oinss.p, n_ins_out * sizeof(pga_ins_t), hipMemcpyDeviceToHost, st));
		dl.wait();
		PGA_HIP(sync_stream(st));
	}
	for (uint64_t o = 0; o < n_mem; ++o) {
		out->members[o].n_subs = T.mem[o].s[0].n_sub + T.mem[o].s[1].n_sub;
		out->members[o].n_dels = T.mem[o].s[0].n_del + T.mem[o].s[1].n_del;
		out->members[o].n_inss = m_nins[o];
	}
	for (int64_t e = 0; e < n_edges; ++e) if (e_bad[e]) out->edges[e].status = 2;
	for (uint64_t j = 0; j < n_jobs; ++j) if (j_flags[j] & ROW_BAD_COMP) out->edges[T.job_edge[j]].status = 2;
}

} // namespace pga
