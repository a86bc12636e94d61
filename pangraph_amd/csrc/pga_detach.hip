// pga_detach.hip -- detach_unaligned_nodes (packages/pangraph/src/pangraph/detach_unaligned.rs:24-114): the members of a batch of blocks
// whose alignment holds no aligned position (Edit::aligned_count == 0, edits.rs:439-442) leave their blocks, and each becomes a singleton
// block of its own sequence (Edit::apply, edits.rs:307-329; reverse-complemented, io/seq.rs:9-33, when its node was reverse).  The reference
// walks block after block, clones every removed edit and applies it letter by letter.  Here the whole batch is one call; a MEMBER is the unit.
//   host              validation (all of it before anything is launched) and, over the deletions it has just checked, the same decision as
//                     the device takes: that gives the orphans, so that runs are built for them alone (row_piece_runs, pga_rows.h), and
//                     the totals, so that every output array exists before the first launch.  The alternative -- downloading the flags
//                     before the row table is built -- costs a second wait on the stream; this route has ONE, at the end.
//   k_detach_count    one wave per member, lanes over its deletions: the 64-bit sum of their lengths, kept / unaligned
//   k_detach_scan     five waves, one per quantity: exclusive sums over the members (the one kernel with wave intrinsics)
//   k_detach_pack     one wave per member, lanes over entries: the kept members' records and lists in their new places, member_map, the
//                     orphan records
//   k_rows<false>     (pga_rows.h) the orphans' letters: one row per orphan, one piece, unaligned mode, ONE launch, flags ROW_BAD_COMP / ROW_GAP
//   host              the block ids: XXH64 over the downloaded letters, one orphan per task on the library's host threads.  The letters
//                     come back anyway (they are the caller's new consensus sequences); a device XXH64 is one dependent multiply chain per
//                     orphan and would, with few orphans, lose to a host core on long sequences (reasoned, not measured).
// The totals the device summed are compared with the host's before anything is handed out.  The index arithmetic is pga_detach_idx.h.
#include "pga_common.h"
#include "pga_graph_host.h"
#include "pga_wave.h"
#include "../../include/pga_align.h"
#include "pga_detach_idx.h"

namespace pga {

// workgroup q, ONE wave: off[q][m] = what scan q adds for the members before m; off[q][n_mem] = the total
__global__ __launch_bounds__(64) void k_detach_scan(DtDev V)
{
	const uint32_t lane = threadIdx.x;
	const int q = (int)blockIdx.x;
	dt_u64 *off = V.off + (uint64_t)q * (V.n_mem + 1);
	dt_u64 run = 0;
	for (uint64_t c0 = 0; c0 < V.n_mem; c0 += 64) {
		const uint64_t m = c0 + lane;
		const dt_u64 v = m < V.n_mem ? dt_scan_value(V.members[m], V.unal[m], q) : 0ULL, in = wave_incl_u64(v, lane);
		if (m < V.n_mem) off[m] = run + in - v;
		run += __shfl(in, 63);
	}
	if (lane == 0) off[V.n_mem] = run;
}

static unsigned dt_grid(uint64_t items, uint64_t per_block) { return grid_for(items, per_block, 1u << 16); }

void detach_unaligned_host(int64_t n_blocks, const pga_rc_block_t *blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss,
                           const char *ins_seq, const pga_detach_member_t *who, pga_detach_out_t *out)
{
	auto fail = [](const std::string &what) { throw std::runtime_error("pga_detach_unaligned: " + what); };
	// ---- validation and tables: everything that fails the call does so here ----
	RowGraph G;
	row_graph_init(G, "pga_detach_unaligned", n_blocks, blocks, members, subs, dels, inss, ins_seq, true, range_threads());
	DtTables T;
	dt_build_tables(G, who, range_threads(), T);
	const uint64_t n_mem = G.n_mem, n_orph = T.orphans.size(), n_jobs = T.rows.jobs.size();
	out->n_blocks = n_blocks + (int64_t)n_orph; out->n_orphans = (int64_t)n_orph;
	out->blocks = host_array<pga_rc_block_t>((uint64_t)out->n_blocks, "pga_detach_unaligned");
	out->members = host_array<pga_rc_member_t>(n_mem, "pga_detach_unaligned");
	out->subs = host_array<pga_sub_t>(T.tot[DT_SUB], "pga_detach_unaligned"); out->dels = host_array<pga_del_t>(T.tot[DT_DEL], "pga_detach_unaligned"); out->inss = host_array<pga_ins_t>(T.tot[DT_INS], "pga_detach_unaligned");
	out->member_map = host_array<int64_t>(n_mem, "pga_detach_unaligned");
	const uint64_t cons_bytes = T.rows.units * ROW_LETTERS;
	if (n_orph) { out->orphans = host_array<pga_detach_orphan_t>(n_orph, "pga_detach_unaligned"); out->cons = host_array<char>(cons_bytes + 1, "pga_detach_unaligned"); }
	for (int64_t b = 0; b < n_blocks; ++b) out->blocks[b] = pga_rc_block_t{blocks[b].consensus, blocks[b].cons_len, T.kept_in[b]};
	for (uint64_t k = 0; k < n_orph; ++k) out->blocks[n_blocks + k] = pga_rc_block_t{out->cons + T.cons_off[k], T.len[k], 1u};
	if (n_mem == 0) return;                                                  // (no member: nothing to decide, nothing to pack)
	// ---- the device ----
	StreamLease stream;
	hipStream_t st = stream.s;
	const uint64_t n_sub_in = G.sub_off[n_mem], n_del_in = G.del_off[n_mem], n_ins_in = G.ins_off[n_mem];
	std::vector<uint32_t> cons_len(n_mem);
	for (uint64_t m = 0; m < n_mem; ++m) cons_len[m] = blocks[G.blk_of[m]].cons_len;
	DBuf<pga_rc_member_t> d_members(n_mem), d_omembers(n_mem);
	DBuf<uint32_t> d_len(n_mem), d_unal(n_mem);
	DBuf<uint64_t> d_offs(3 * (n_mem + 1));
	DBuf<pga_detach_member_t> d_who(n_mem);
	DBuf<pga_sub_t> d_subs(n_sub_in + 1), d_osubs(n_sub_in + 1);              // (the outputs as large as the inputs: whatever the device decides fits)
	DBuf<pga_del_t> d_dels(n_del_in + 1), d_odels(n_del_in + 1);
	DBuf<pga_ins_t> d_inss(n_ins_in + 1), d_oinss(n_ins_in + 1);
	DBuf<dt_u64> d_sum(n_mem), d_off((uint64_t)DT_SCANS * (n_mem + 1));
	DBuf<int64_t> d_map(n_mem);
	DBuf<pga_detach_orphan_t> d_orph(n_orph + 1);
	PGA_HIP(hipMemcpyAsync(d_members.p, members, n_mem * sizeof(pga_rc_member_t), hipMemcpyHostToDevice, st));
	PGA_HIP(hipMemcpyAsync(d_len.p, cons_len.data(), n_mem * sizeof(uint32_t), hipMemcpyHostToDevice, st));
	PGA_HIP(hipMemcpyAsync(d_offs.p, G.sub_off.data(), (n_mem + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
	PGA_HIP(hipMemcpyAsync(d_offs.p + (n_mem + 1), G.del_off.data(), (n_mem + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
	PGA_HIP(hipMemcpyAsync(d_offs.p + 2 * (n_mem + 1), G.ins_off.data(), (n_mem + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
	PGA_HIP(hipMemcpyAsync(d_who.p, who, n_mem * sizeof(pga_detach_member_t), hipMemcpyHostToDevice, st));
	if (n_sub_in) PGA_HIP(hipMemcpyAsync(d_subs.p, subs, n_sub_in * sizeof(pga_sub_t), hipMemcpyHostToDevice, st));
	if (n_del_in) PGA_HIP(hipMemcpyAsync(d_dels.p, dels, n_del_in * sizeof(pga_del_t), hipMemcpyHostToDevice, st));
	if (n_ins_in) PGA_HIP(hipMemcpyAsync(d_inss.p, inss, n_ins_in * sizeof(pga_ins_t), hipMemcpyHostToDevice, st));
	DtDev V;
	V.n_mem = n_mem; V.n_blocks_in = (uint64_t)n_blocks; V.cap_orphans = n_orph;
	V.members = d_members.p; V.cons_len = d_len.p; V.sub_off = d_offs.p; V.del_off = d_offs.p + (n_mem + 1); V.ins_off = d_offs.p + 2 * (n_mem + 1);
	V.subs = d_subs.p; V.dels = d_dels.p; V.inss = d_inss.p; V.who = d_who.p;
	V.del_sum = d_sum.p; V.unal = d_unal.p; V.off = d_off.p;
	hipLaunchKernelGGL(k_detach_count, dim3(dt_grid(n_mem, DT_WAVES)), dim3(DT_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_detach_scan, dim3(DT_SCANS), dim3(64), 0, st, V);
	hipLaunchKernelGGL(k_detach_pack, dim3(dt_grid(n_mem, DT_WAVES)), dim3(DT_THREADS), 0, st, V, d_omembers.p, d_osubs.p, d_odels.p, d_oinss.p, d_map.p, d_orph.p);
	PGA_HIP(hipGetLastError());
	// ---- the letters: one row per orphan that has any ----
	const RowTable &R = T.rows;
	const uint64_t il = R.ins_lo < R.ins_hi ? R.ins_lo : 0, ih = R.ins_lo < R.ins_hi ? R.ins_hi : 0;
	DBuf<char> d_cons(R.cons.size() + 16), d_iseq(ih - il + 16), d_out(cons_bytes + 16);
	DBuf<RowJob> d_jobs(n_jobs + 1); DBuf<RowRun> d_runs(R.runs.size() + 1); DBuf<uint32_t> d_flags(n_jobs + 1);
	if (n_jobs) {
		if (!R.cons.empty()) PGA_HIP(hipMemcpyAsync(d_cons.p, R.cons.data(), R.cons.size(), hipMemcpyHostToDevice, st));
		if (ih > il) PGA_HIP(hipMemcpyAsync(d_iseq.p, ins_seq + il, ih - il, hipMemcpyHostToDevice, st));
		PGA_HIP(hipMemcpyAsync(d_jobs.p, R.jobs.data(), n_jobs * sizeof(RowJob), hipMemcpyHostToDevice, st));
		PGA_HIP(hipMemcpyAsync(d_runs.p, R.runs.data(), R.runs.size() * sizeof(RowRun), hipMemcpyHostToDevice, st));
		d_flags.zero(st);
		const unsigned grid = (unsigned)std::min<uint64_t>((R.units + ROW_THREADS - 1) / ROW_THREADS, 2048);
		hipLaunchKernelGGL(k_rows<false>, dim3(grid), dim3(ROW_THREADS), 0, st, d_jobs.p, (int)n_jobs, (uint64_t)0, R.units, d_runs.p, d_cons.p, d_iseq.p, il,
		                   d_out.p, d_flags.p, ROW_GAP, (const char*)nullptr, (unsigned long long*)nullptr, (unsigned long long*)nullptr);
		PGA_HIP(hipGetLastError());
	}
	// ---- the one wait ----
	std::vector<uint32_t> j_flags;
	dt_u64 tot[DT_SCANS];
	{
		Downloads dl(st);
		if (n_jobs) dl.add(j_flags, d_flags.p, n_jobs);
		for (int q = 0; q < DT_SCANS; ++q) PGA_HIP(hipMemcpyAsync(&tot[q], d_off.p + (uint64_t)q * (n_mem + 1) + n_mem, sizeof(dt_u64), hipMemcpyDeviceToHost, st));
		PGA_HIP(hipMemcpyAsync(out->members, d_omembers.p, n_mem * sizeof(pga_rc_member_t), hipMemcpyDeviceToHost, st));
		PGA_HIP(hipMemcpyAsync(out->member_map, d_map.p, n_mem * sizeof(int64_t), hipMemcpyDeviceToHost, st));
		if (T.tot[DT_SUB]) PGA_HIP(hipMemcpyAsync(out->subs, d_osubs.p, T.tot[DT_SUB] * sizeof(pga_sub_t), hipMemcpyDeviceToHost, st));
		if (T.tot[DT_DEL]) PGA_HIP(hipMemcpyAsync(out->dels, d_odels.p, T.tot[DT_DEL] * sizeof(pga_del_t), hipMemcpyDeviceToHost, st));
		if (T.tot[DT_INS]) PGA_HIP(hipMemcpyAsync(out->inss, d_oinss.p, T.tot[DT_INS] * sizeof(pga_ins_t), hipMemcpyDeviceToHost, st));
		if (n_orph) PGA_HIP(hipMemcpyAsync(out->orphans, d_orph.p, n_orph * sizeof(pga_detach_orphan_t), hipMemcpyDeviceToHost, st));
		if (cons_bytes) PGA_HIP(hipMemcpyAsync(out->cons, d_out.p, cons_bytes, hipMemcpyDeviceToHost, st));
		dl.wait();
		PGA_HIP(sync_stream(st));
	}
	for (int q = 0; q < DT_SCANS; ++q) if (tot[q] != T.tot[q]) fail("internal: the device and the host disagree on which members are unaligned");
	// ---- lengths, statuses, block ids ----
	std::vector<uint32_t> o_flags(n_orph, 0);
	for (uint64_t j = 0; j < n_jobs; ++j) o_flags[R.job_row[j]] = j_flags[j];
	thread_ranges(n_orph, range_threads(), [&](int, uint64_t k0, uint64_t k1) {
		std::vector<uint8_t> buf;
		for (uint64_t k = k0; k < k1; ++k) {
			pga_detach_orphan_t &O = out->orphans[k];
			if (O.member != T.orphans[k]) fail("internal: the device and the host disagree on the order of the orphans");
			O.len = T.len[k];
			O.status = (o_flags[k] & ROW_BAD_COMP) ? 2 : (o_flags[k] & ROW_GAP) ? 3 : 0;
			O.block_id = O.status ? 0ULL : dt_block_id(O.node_id, out->cons + T.cons_off[k], O.len, buf);
		}
	});
}

} // namespace pga
