// pga_remove.hip -- the first step of `pangraph simplify` (commands/simplify/simplify_run.rs:23-38): Pangraph::remove_path
// (pangraph/pangraph.rs:110-132) for every path that is not kept, in one call on the flat graph of pga_plan_simplify and the block arrays of
// pga_merge_blocks.  The reference pops every node of a removed path from two maps and then walks all blocks for empty ones, once per path;
// here a MEMBER, a path POSITION and a LIST ELEMENT are the units of work.
//   host               validation (all of it before anything is launched), the totals of the three lists, the path table after (O(paths))
//   k_topo_keys / _check   pga_topo_idx.h: the path of every position, every (block, member) slot named exactly once
//   k_remove_mark      one thread per position: the members of kept paths
//   k_ts_sums / _scan / _offsets (pga_tile_scan.h), members   seven exclusive sums over the members, side by side: the kept flag, where the
//                      three lists of a member start in the input, where they start in the output
//   host               the first wait: the checks, the totals
//   k_remove_blocks / _members / _nodes   kept counts per block, member_map, the slot renumbering, the nodes at their places
//   k_remove_copy<list>   one thread per element of an output list (never one thread per member: a member has no edit or 10^4)
//   with PGA_REMOVE_COMPACT_LETTERS: the scan again over the output insertions' lengths, a wait (the bounds of every kept insertion were
//                      checked by the copy; the letter total), k_remove_letters one thread per letter, k_remove_seq_off
//   host               the last wait: the output
// The kernels and the host tables are pga_remove_idx.h (no wave intrinsic: tests/emu/remove_emu.cpp runs them on the host).
// All arithmetic is integer; atomics feed only minima, so the result does not depend on the launch geometry.
#include "pga_common.h"
#include "pga_graph_host.h"
#include "../../include/pga_align.h"
#include "pga_remove_idx.h"

namespace pga {

static unsigned rm_grid(uint64_t items) { return grid_for(items, RM_THREADS, 2048); }
static unsigned rm_tile_grid(uint64_t items) { return grid_for(items, RM_TILE, 1u << 16); }

// the stream's clock at four places of the last call of this thread: upload, kernels (their waits included), download, in ms
static thread_local double g_rm_ms[3] = {0, 0, 0};
void remove_last_ms(double *ms) { for (int i = 0; i < 3; ++i) ms[i] = g_rm_ms[i]; }

void remove_paths_host(int64_t n_blocks, const pga_topo_block_t *blocks, int64_t n_paths, const pga_topo_path_t *paths, int64_t n_nodes, const pga_topo_node_t *nodes,
                       const pga_rc_block_t *rc_blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss,
                       const char *ins_seq, uint64_t ins_seq_len, const uint8_t *keep, uint32_t flags, pga_remove_out_t *out)
{
	RmTables R;
	rm_validate(n_blocks, blocks, n_paths, paths, n_nodes, nodes, rc_blocks, members, subs, dels, inss, keep, flags, R);
	const uint64_t nn = (uint64_t)n_nodes, np = (uint64_t)n_paths, nb = (uint64_t)n_blocks, nm = R.n_members, np_out = R.o_paths.size(), nn_out = R.n_out_nodes;
	const bool letters = (flags & PGA_REMOVE_COMPACT_LETTERS) != 0;
	out->n_blocks = n_blocks;
	out->blocks = host_array<pga_topo_block_t>(nb, "pga_remove_paths"); out->rc_blocks = host_array<pga_rc_block_t>(nb, "pga_remove_paths");
	out->path_map = host_array<int32_t>(np, "pga_remove_paths"); out->member_map = host_array<int64_t>(nm, "pga_remove_paths");
	if (n_paths == 0) {                                                      // no path, so no member (rm_validate): nothing to launch
		for (uint64_t b = 0; b < nb; ++b) {
			const bool alive = blocks[b].alive != 0;
			out->blocks[b] = alive ? pga_topo_block_t{blocks[b].block_id, blocks[b].cons_len, 0u, 1, 0} : pga_topo_block_t{blocks[b].block_id, 0u, 0u, 0, 0};
			out->rc_blocks[b] = pga_rc_block_t{rc_blocks[b].consensus, rc_blocks[b].cons_len, 0u};
			out->n_dead_blocks += alive ? 0 : 1;
		}
		out->paths = host_array<pga_topo_path_t>(0, "pga_remove_paths"); out->nodes = host_array<pga_topo_node_t>(0, "pga_remove_paths"); out->members = host_array<pga_rc_member_t>(0, "pga_remove_paths");
		out->subs = host_array<pga_sub_t>(0, "pga_remove_paths"); out->dels = host_array<pga_del_t>(0, "pga_remove_paths"); out->inss = host_array<pga_ins_t>(0, "pga_remove_paths");
		if (letters) out->ins_seq = host_array<char>(0, "pga_remove_paths");
		return;
	}
	out->n_paths = (int64_t)np_out; out->n_nodes = (int64_t)nn_out;
	out->paths = host_array<pga_topo_path_t>(np_out, "pga_remove_paths"); out->nodes = host_array<pga_topo_node_t>(nn_out, "pga_remove_paths");
	std::copy(R.o_paths.begin(), R.o_paths.end(), out->paths); std::copy(R.path_map.begin(), R.path_map.end(), out->path_map);
	StreamLease stream;
	hipStream_t st = stream.s;
	StageClock clock(st);
	clock.at(0);
	// ---- the uploads (every buffer one entry longer than its count: none is empty) ----
	const uint64_t n_letters_in = letters && ins_seq ? ins_seq_len : 0;
	DBuf<pga_topo_node_t> d_nodes(nn + 1), d_onodes(nn_out + 1); DBuf<pga_topo_path_t> d_paths(np + 1); DBuf<pga_topo_block_t> d_blocks(nb + 1), d_oblocks(nb + 1);
	DBuf<uint32_t> d_depth(nb + 1), d_first(nb + 1), d_mkeep(nm + 1); DBuf<uint8_t> d_keep(np + 1); DBuf<rm_u64> d_newoff(np + 1);
	DBuf<pga_rc_member_t> d_members(nm + 1); DBuf<pga_sub_t> d_subs(R.n_subs + 1); DBuf<pga_del_t> d_dels(R.n_dels + 1); DBuf<pga_ins_t> d_inss(R.n_inss + 1);
	DBuf<char> d_seq(n_letters_in + 1);
	upload(d_nodes, nodes, nn, st); upload(d_paths, paths, np, st); upload(d_blocks, blocks, nb, st);
	upload(d_depth, R.T.depth.data(), nb, st); upload(d_first, R.T.slot_first.data(), nb + 1, st); upload(d_keep, keep, np, st);
	upload(d_newoff, (const rm_u64*)R.path_new_off.data(), np, st); upload(d_members, members, nm, st);
	upload(d_subs, subs, R.n_subs, st); upload(d_dels, dels, R.n_dels, st); upload(d_inss, inss, R.n_inss, st); upload(d_seq, ins_seq, n_letters_in, st);
	clock.at(1);
	// ---- the checks of the graph, as pga_plan_simplify makes them; the kept members; the member scan ----
	DBuf<uint32_t> d_pathof(nn + 1), d_cnts(nm + nb + 1), d_terr(TP_ERRS);
	DBuf<tp_u64> d_key(nn + 1); DBuf<rm_u64> d_err(RM_ERRS);
	d_cnts.zero(st); d_mkeep.zero(st);
	PGA_HIP(hipMemsetAsync(d_terr.p, 0xff, TP_ERRS * sizeof(uint32_t), st));
	PGA_HIP(hipMemsetAsync(d_err.p, 0xff, RM_ERRS * sizeof(rm_u64), st));
	TpDev T;
	memset(&T, 0, sizeof(T));
	T.n_nodes = nn; T.n_paths = np; T.n_blocks = nb; T.n_slots = nm;
	T.nodes = d_nodes.p; T.paths = d_paths.p; T.depth = d_depth.p; T.slot_first = d_first.p; T.path_of = d_pathof.p; T.key = d_key.p;
	T.slot_cnt = d_cnts.p; T.blk_cnt = d_cnts.p + nm; T.err = d_terr.p;
	TileScanBufs<rm_u64> b_mem, b_let;
	RmDev V;
	memset(&V, 0, sizeof(V));
	V.n_nodes = nn; V.n_paths = np; V.n_blocks = nb; V.n_members = nm; V.ins_seq_len = ins_seq_len; V.flags = flags;
	V.nodes = d_nodes.p; V.paths = d_paths.p; V.blocks = d_blocks.p; V.slot_first = d_first.p; V.path_of = d_pathof.p; V.keep = d_keep.p; V.path_new_off = d_newoff.p;
	V.members = d_members.p; V.subs = d_subs.p; V.dels = d_dels.p; V.inss = d_inss.p; V.ins_seq = letters && ins_seq ? d_seq.p : nullptr;
	V.mkeep = d_mkeep.p; V.err = d_err.p;
	V.scan[RM_SCAN_MEMBERS] = b_mem.make(nm, RM_QS);
	hipLaunchKernelGGL(k_topo_keys, dim3(rm_grid(nn)), dim3(TP_THREADS), 0, st, T);
	hipLaunchKernelGGL(k_topo_check, dim3(rm_grid(std::max(nm, nb))), dim3(TP_THREADS), 0, st, T);
	hipLaunchKernelGGL(k_remove_mark, dim3(rm_grid(nn)), dim3(RM_THREADS), 0, st, V);
	tile_scan_launch(V.scan[RM_SCAN_MEMBERS], RmMemberValue{V}, st);
	PGA_HIP(hipGetLastError());
	// ---- the first wait: nothing behind it runs on input that was not checked ----
	uint32_t terr[TP_ERRS];
	rm_u64 tot[RM_QS];
	fetch(terr, (const uint32_t*)d_terr.p, TP_ERRS, st);
	for (int q = 0; q < RM_QS; ++q) fetch(&tot[q], ts_off(V.scan[RM_SCAN_MEMBERS], q) + nm, 1, st);
	PGA_HIP(sync_stream(st));
	rm_report(terr);
	if (tot[RM_Q_IN_SUB] != R.n_subs || tot[RM_Q_IN_DEL] != R.n_dels || tot[RM_Q_IN_INS] != R.n_inss || tot[RM_Q_KEPT] > nm || tot[RM_Q_OUT_SUB] > R.n_subs ||
	    tot[RM_Q_OUT_DEL] > R.n_dels || tot[RM_Q_OUT_INS] > R.n_inss) rm_fail("internal: the device and the host disagree on the list totals");
	const uint64_t nm_out = tot[RM_Q_KEPT], ns_out = tot[RM_Q_OUT_SUB], nd_out = tot[RM_Q_OUT_DEL], ni_out = tot[RM_Q_OUT_INS];
	// ---- blocks, members, nodes, the three lists ----
	DBuf<pga_rc_member_t> d_omembers(nm_out + 1); DBuf<pga_sub_t> d_osubs(ns_out + 1); DBuf<pga_del_t> d_odels(nd_out + 1); DBuf<pga_ins_t> d_oinss(ni_out + 1);
	DBuf<long long> d_map(nm + 1);
	V.o_blocks = d_oblocks.p; V.o_nodes = d_onodes.p; V.o_members = d_omembers.p; V.o_subs = d_osubs.p; V.o_dels = d_odels.p; V.o_inss = d_oinss.p; V.member_map = d_map.p;
	hipLaunchKernelGGL(k_remove_blocks, dim3(rm_grid(nb)), dim3(RM_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_remove_members, dim3(rm_grid(nm)), dim3(RM_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_remove_nodes, dim3(rm_grid(nn)), dim3(RM_THREADS), 0, st, V);
	if (ns_out) hipLaunchKernelGGL(k_remove_copy<RM_LIST_SUB>, dim3(rm_tile_grid(ns_out)), dim3(RM_THREADS), 0, st, V);
	if (nd_out) hipLaunchKernelGGL(k_remove_copy<RM_LIST_DEL>, dim3(rm_tile_grid(nd_out)), dim3(RM_THREADS), 0, st, V);
	if (ni_out) hipLaunchKernelGGL(k_remove_copy<RM_LIST_INS>, dim3(rm_tile_grid(ni_out)), dim3(RM_THREADS), 0, st, V);
	PGA_HIP(hipGetLastError());
	// ---- the letters ----
	uint64_t nl_out = 0;
	DBuf<char> d_oseq;
	if (letters) {
		V.scan[RM_SCAN_LETTERS] = b_let.make(ni_out, 1);
		tile_scan_launch(V.scan[RM_SCAN_LETTERS], RmLetterValue{V}, st);
		PGA_HIP(hipGetLastError());
		rm_u64 err[RM_ERRS], n_let = 0;
		fetch(err, (const rm_u64*)d_err.p, RM_ERRS, st); fetch(&n_let, ts_off(V.scan[RM_SCAN_LETTERS], 0) + ni_out, 1, st);
		PGA_HIP(sync_stream(st));
		rm_report_letters(err);                                                  // (before a letter is read)
		nl_out = n_let;
		d_oseq.alloc(nl_out + 1);
		V.o_ins_seq = d_oseq.p;
		if (nl_out) hipLaunchKernelGGL(k_remove_letters, dim3(rm_tile_grid(nl_out)), dim3(RM_THREADS), 0, st, V);
		if (ni_out) hipLaunchKernelGGL(k_remove_seq_off, dim3(rm_grid(ni_out)), dim3(RM_THREADS), 0, st, V);
		PGA_HIP(hipGetLastError());
	}
	clock.at(2);
	// ---- the output ----
	out->members = host_array<pga_rc_member_t>(nm_out, "pga_remove_paths"); out->subs = host_array<pga_sub_t>(ns_out, "pga_remove_paths"); out->dels = host_array<pga_del_t>(nd_out, "pga_remove_paths");
	out->inss = host_array<pga_ins_t>(ni_out, "pga_remove_paths");
	if (letters) out->ins_seq = host_array<char>(nl_out + 1, "pga_remove_paths");
	fetch(out->blocks, (const pga_topo_block_t*)d_oblocks.p, nb, st); fetch(out->nodes, (const pga_topo_node_t*)d_onodes.p, nn_out, st);
	fetch(out->members, (const pga_rc_member_t*)d_omembers.p, nm_out, st); fetch(out->subs, (const pga_sub_t*)d_osubs.p, ns_out, st);
	fetch(out->dels, (const pga_del_t*)d_odels.p, nd_out, st); fetch(out->inss, (const pga_ins_t*)d_oinss.p, ni_out, st);
	fetch((long long*)out->member_map, (const long long*)d_map.p, nm, st);
	if (letters) fetch(out->ins_seq, (const char*)d_oseq.p, nl_out, st);
	clock.at(3);
	PGA_HIP(sync_stream(st));
	clock.read(g_rm_ms);
	for (uint64_t b = 0; b < nb; ++b) {
		out->rc_blocks[b] = pga_rc_block_t{rc_blocks[b].consensus, rc_blocks[b].cons_len, out->blocks[b].depth};
		out->n_dead_blocks += out->blocks[b].alive ? 0 : 1;
	}
	out->n_members = (int64_t)nm_out; out->n_subs = ns_out; out->n_dels = nd_out; out->n_inss = ni_out; out->n_ins_letters = nl_out;
}

} // namespace pga
