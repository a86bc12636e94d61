// pga_apply.hip -- the graph update of one merge round on the flat graph of pga_plan_simplify: what reweave leaves behind its slices
// (split_block's n_new / b_new, reweave.rs:359-401; Pangraph::update, pangraph.rs:68-107, block after block, reweave.rs:445-450) and the
// insertion of the merged blocks (graph_merging.rs:156-165).  The reference pops every old node from a map and splices its path list, once
// per node; here a kept slice MEMBER and a path POSITION are the units of work and a round is one call.
//   host               validation (all of it before anything is launched), the cut / interval / entry tables; one upload
//   k_topo_keys / _check   pga_topo_idx.h: the path of every position, every (block, member) slot named exactly once
//   k_apply_slot_pos   one thread per position: where every slot lies
//   k_apply_members    one thread per kept member: member < depth, its word of the (member, interval) matrix, the new node (XXH64), the old id
//   rocPRIM            the entries' ids sorted; k_apply_entries / _survivors: the block table after, block_map, equal ids found
//   rocPRIM            members sorted by node id, then (stable) by the rank of their block; k_apply_slots: member slots, member_src, equal ids found
//   host               the first wait: the checks
//   rocPRIM            the matrix scanned; k_apply_order: the new nodes in path order (a reverse old node mirrors its row); k_apply_positions: cnt[] / repl[]
//   k_topo_tile_sums / _tile_scan / _splice / _paths   pga_topo_idx.h: the general splice; its total is held against the host's before it scatters
// The kernels and the host tables are pga_apply_idx.h (no wave intrinsic: tests/emu/apply_emu.cpp runs them on the host).
// All arithmetic is integer; atomics feed only counts and minima, so the result does not depend on the launch geometry.
#include "pga_common.h"
#include "pga_graph_host.h"
#include "../../include/pga_align.h"
#include "pga_apply_idx.h"
#include <numeric>

namespace pga {

static unsigned ap_grid(uint64_t items) { return grid_for(items, TP_THREADS, 2048); }

void apply_merge_host(int64_t n_blocks, const pga_topo_block_t *blocks, int64_t n_paths, const pga_topo_path_t *paths, int64_t n_nodes, const pga_topo_node_t *nodes,
                      int64_t n_cut, const pga_apply_cut_t *cut, const pga_plan_interval_t *intervals, const pga_slice_res_t *slices, const pga_slice_member_t *members,
                      pga_apply_out_t *out)
{
	ApTables A;
	ap_validate(n_blocks, blocks, n_paths, paths, n_nodes, nodes, n_cut, cut, intervals, slices, members, A);
	if (n_cut == 0) return;
	const uint64_t nn = (uint64_t)n_nodes, np = (uint64_t)n_paths, nb = (uint64_t)n_blocks, nc = (uint64_t)n_cut;
	const uint64_t ni = A.n_intervals, nm = A.n_members, ne = A.entries.size(), ns = A.surv_ids.size(), n_out = A.n_out_nodes, nb_out = ns + ne;
	StreamLease stream;
	hipStream_t st = stream.s;
	// ---- the uploads (every buffer one entry longer than its count: none is empty) ----
	DBuf<pga_topo_node_t> d_nodes(nn + 1); DBuf<pga_topo_path_t> d_paths(np + 1); DBuf<pga_topo_block_t> d_blocks(nb + 1);
	DBuf<uint32_t> d_depth(nb + 1), d_first(nb + 1), d_cutof(nb + 1), d_matoff(nc + 1), d_ivcut(ni + 1), d_iventry(ni + 1), d_survrank(nb + 1), d_iota(std::max(nm, ne) + 1);
	DBuf<pga_apply_cut_t> d_cut(nc + 1); DBuf<pga_plan_interval_t> d_iv(ni + 1); DBuf<pga_slice_res_t> d_slices(ni + 1); DBuf<pga_slice_member_t> d_members(nm + 1);
	DBuf<ApEntry> d_entries(ne + 1); DBuf<tp_u64> d_eids(ne + 1), d_seids(ne + 1), d_survids(ns + 1);
	upload(d_nodes, nodes, nn, st); upload(d_paths, paths, np, st); upload(d_blocks, blocks, nb, st);
	upload(d_depth, A.T.depth.data(), nb, st); upload(d_first, A.T.slot_first.data(), nb + 1, st); upload(d_cutof, A.cut_of.data(), nb, st);
	upload(d_matoff, A.mat_off.data(), nc + 1, st); upload(d_ivcut, A.iv_cut.data(), ni, st); upload(d_iventry, A.iv_entry.data(), ni, st);
	upload(d_survrank, A.surv_rank.data(), nb, st); upload(d_cut, cut, nc, st); upload(d_iv, intervals, ni, st); upload(d_slices, slices, ni, st);
	upload(d_members, members, nm, st); upload(d_entries, A.entries.data(), ne, st); upload(d_eids, (const tp_u64*)A.entry_ids.data(), ne, st);
	upload(d_survids, (const tp_u64*)A.surv_ids.data(), ns, st);
	std::vector<uint32_t> iota(std::max(nm, ne) + 1);
	std::iota(iota.begin(), iota.end(), 0u);
	upload(d_iota, iota.data(), iota.size(), st);
	// ---- the checks of the graph, as pga_plan_simplify makes them ----
	DBuf<uint32_t> d_pathof(nn + 1), d_cnts(A.T.n_slots + nb + 1), d_terr(TP_ERRS), d_err(AP_ERRS);
	DBuf<tp_u64> d_key(nn + 1);
	d_cnts.zero(st);
	PGA_HIP(hipMemsetAsync(d_terr.p, 0xff, TP_ERRS * sizeof(uint32_t), st));
	PGA_HIP(hipMemsetAsync(d_err.p, 0xff, AP_ERRS * sizeof(uint32_t), st));
	TpDev T;
	memset(&T, 0, sizeof(T));
	T.n_nodes = nn; T.n_paths = np; T.n_blocks = nb; T.n_slots = A.T.n_slots;
	T.nodes = d_nodes.p; T.paths = d_paths.p; T.depth = d_depth.p; T.slot_first = d_first.p; T.path_of = d_pathof.p; T.key = d_key.p;
	T.slot_cnt = d_cnts.p; T.blk_cnt = d_cnts.p + A.T.n_slots; T.err = d_terr.p;
	hipLaunchKernelGGL(k_topo_keys, dim3(ap_grid(nn)), dim3(TP_THREADS), 0, st, T);
	hipLaunchKernelGGL(k_topo_check, dim3(ap_grid(std::max(A.T.n_slots, nb))), dim3(TP_THREADS), 0, st, T);
	// ---- the members, the block table, the member slots ----
	DBuf<uint32_t> d_slotpos(A.T.n_slots + 1), d_mat(A.n_mat + 1), d_matscan(A.n_mat + 1), d_mslice(nm + 1), d_ment(nm + 1);
	DBuf<pga_topo_node_t> d_new(nm + 1); DBuf<uint64_t> d_old(nm + 1), d_msrc(nm + 1); DBuf<tp_u64> d_nkey(nm + 1), d_nkey_s(nm + 1);
	DBuf<uint32_t> d_sentry(ne + 1), d_erank(ne + 1), d_rindex(ne + 1), d_rdepth(ne + 1), d_rmoff(ne + 1), d_bmap(nb + 1);
	DBuf<pga_topo_block_t> d_oblocks(nb_out + 1); DBuf<pga_apply_block_t> d_onew(ne + 1);
	DBuf<uint32_t> d_byid(nm + 1), d_key2(nm + 1), d_key2s(nm + 1), d_byslot(nm + 1);
	d_slotpos.zero(st); d_mat.zero(st);
	ApDev V;
	memset(&V, 0, sizeof(V));
	V.n_nodes = nn; V.n_paths = np; V.n_blocks = nb; V.n_intervals = ni; V.n_members = nm; V.n_mat = A.n_mat; V.n_entries = ne; V.n_surv = ns;
	V.nodes = d_nodes.p; V.paths = d_paths.p; V.blocks = d_blocks.p; V.depth = d_depth.p; V.slot_first = d_first.p; V.path_of = d_pathof.p;
	V.cut_of = d_cutof.p; V.cut = d_cut.p; V.mat_off = d_matoff.p; V.iv_cut = d_ivcut.p; V.iv_entry = d_iventry.p;
	V.intervals = d_iv.p; V.slices = d_slices.p; V.members = d_members.p;
	V.slot_pos = d_slotpos.p; V.mat = d_mat.p; V.mat_scan = d_matscan.p; V.m_slice = d_mslice.p; V.m_ent = d_ment.p;
	V.o_new = d_new.p; V.o_old = d_old.p; V.node_key = d_nkey.p; V.err = d_err.p;
	V.entries = d_entries.p; V.sorted_ids = d_seids.p; V.sorted_entry = d_sentry.p; V.surv_ids = d_survids.p; V.surv_rank = d_survrank.p;
	V.entry_rank = d_erank.p; V.rank_index = d_rindex.p; V.rank_depth = d_rdepth.p; V.rank_moff = d_rmoff.p;
	V.block_map = d_bmap.p; V.o_blocks = d_oblocks.p; V.o_new_blocks = d_onew.p;
	V.by_id = d_byid.p; V.key2 = d_key2.p; V.key2_sorted = d_key2s.p; V.by_slot = d_byslot.p; V.member_src = d_msrc.p;
	const unsigned g_mem = ap_grid(nm), g_pos = ap_grid(nn), g_ent = ap_grid(ne + 1);
	hipLaunchKernelGGL(k_apply_slot_pos, dim3(g_pos), dim3(TP_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_apply_members, dim3(g_mem), dim3(TP_THREADS), 0, st, V);
	radix_sort_pairs(d_eids.p, d_seids.p, d_iota.p, d_sentry.p, ne, 64, st);
	hipLaunchKernelGGL(k_apply_entries, dim3(g_ent), dim3(TP_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_apply_survivors, dim3(ap_grid(nb)), dim3(TP_THREADS), 0, st, V);
	excl_scan(d_rdepth.p, d_rmoff.p, ne + 1, st);
	hipLaunchKernelGGL(k_apply_new_blocks, dim3(g_ent), dim3(TP_THREADS), 0, st, V);
	radix_sort_pairs(d_nkey.p, d_nkey_s.p, d_iota.p, d_byid.p, nm, 64, st);
	hipLaunchKernelGGL(k_apply_key2, dim3(g_mem), dim3(TP_THREADS), 0, st, V);
	radix_sort_pairs(d_key2.p, d_key2s.p, d_byid.p, d_byslot.p, nm, 32, st);
	hipLaunchKernelGGL(k_apply_slots, dim3(g_mem), dim3(TP_THREADS), 0, st, V);
	PGA_HIP(hipGetLastError());
	// ---- the first wait: nothing behind it runs on input that was not checked ----
	uint32_t terr[TP_ERRS], err[AP_ERRS];
	fetch(terr, (const uint32_t*)d_terr.p, TP_ERRS, st); fetch(err, (const uint32_t*)d_err.p, AP_ERRS, st);
	PGA_HIP(sync_stream(st));
	ap_report(terr, err);
	// ---- the new nodes in path order, cnt[] / repl[], the tile sums ----
	const uint32_t n_tiles = (uint32_t)((nn + TP_TILE - 1) / TP_TILE);
	DBuf<pga_topo_node_t> d_ordered(nm + 1), d_nodes2(nn + 1), d_onodes(n_out + 1); DBuf<pga_topo_path_t> d_opaths(np + 1);
	DBuf<uint32_t> d_cnt(nn + 1), d_repl(nn + 1), d_tsum(n_tiles + 1), d_toff(n_tiles + 1), d_poff(nn + 1);
	V.ordered = d_ordered.p; V.nodes2 = d_nodes2.p; V.cnt = d_cnt.p; V.repl = d_repl.p;
	excl_scan(d_mat.p, d_matscan.p, A.n_mat + 1, st);
	hipLaunchKernelGGL(k_apply_order, dim3(g_mem), dim3(TP_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_apply_positions, dim3(g_pos), dim3(TP_THREADS), 0, st, V);
	d_poff.zero(st); d_toff.zero(st);
	T.nodes = d_nodes2.p; T.o_new = d_ordered.p; T.cnt = d_cnt.p; T.repl = d_repl.p; T.n_tiles = n_tiles; T.tile_sum = d_tsum.p; T.tile_off = d_toff.p; T.pos_off = d_poff.p;
	T.o_nodes = d_onodes.p; T.o_paths = d_opaths.p;
	uint32_t total = 0;
	if (n_tiles) {
		hipLaunchKernelGGL(k_topo_tile_sums, dim3(std::min<uint32_t>(n_tiles, 2048u)), dim3(TP_THREADS), 0, st, T);
		hipLaunchKernelGGL(k_topo_tile_scan, dim3(1), dim3(TP_THREADS), 0, st, T);
	}
	PGA_HIP(hipGetLastError());
	fetch(&total, (const uint32_t*)d_toff.p + n_tiles, 1, st);
	PGA_HIP(sync_stream(st));
	if (total != n_out) ap_fail("internal: the splice counts " + std::to_string(total) + " nodes, " + std::to_string(n_out) + " expected");   // (before it writes one)
	if (n_tiles) hipLaunchKernelGGL(k_topo_splice, dim3(std::min<uint32_t>(n_tiles, 2048u)), dim3(TP_THREADS), 0, st, T);
	hipLaunchKernelGGL(k_topo_paths, dim3(ap_grid(np)), dim3(TP_THREADS), 0, st, T);
	PGA_HIP(hipGetLastError());
	// ---- the output ----
	out->new_nodes = host_array<pga_topo_node_t>(nm, "pga_apply_merge"); out->old_node = host_array<uint64_t>(nm, "pga_apply_merge"); out->member_src = host_array<uint64_t>(nm, "pga_apply_merge");
	out->new_blocks = host_array<pga_apply_block_t>(ne, "pga_apply_merge"); out->block_map = host_array<uint32_t>(nb, "pga_apply_merge");
	out->paths = host_array<pga_topo_path_t>(np, "pga_apply_merge"); out->nodes = host_array<pga_topo_node_t>(n_out, "pga_apply_merge"); out->blocks = host_array<pga_topo_block_t>(nb_out, "pga_apply_merge");
	fetch(out->new_nodes, (const pga_topo_node_t*)d_new.p, nm, st); fetch(out->old_node, (const uint64_t*)d_old.p, nm, st);
	fetch(out->member_src, (const uint64_t*)d_msrc.p, nm, st); fetch(out->new_blocks, (const pga_apply_block_t*)d_onew.p, ne, st);
	fetch(out->block_map, (const uint32_t*)d_bmap.p, nb, st); fetch(out->paths, (const pga_topo_path_t*)d_opaths.p, np, st);
	fetch(out->nodes, (const pga_topo_node_t*)d_onodes.p, n_out, st); fetch(out->blocks, (const pga_topo_block_t*)d_oblocks.p, nb_out, st);
	PGA_HIP(sync_stream(st));
	out->n_new_nodes = (int64_t)nm; out->n_new_blocks = (int64_t)ne; out->n_blocks = (int64_t)nb_out; out->n_paths = n_paths; out->n_nodes = (int64_t)n_out;
}

} // namespace pga
