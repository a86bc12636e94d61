// pga_topo.hip -- the path side of one round of `pangraph simplify` / remove_transitive_edges (circularize/circularize.rs:11-76,
// circularize/merge_blocks.rs:33-89 and :196-234): edge counts, the transitive edges, a round of disjoint edges with their orientation, the
// node pairings (the `partner` of pga_merge_blocks), the new nodes with their ids, and the rewritten paths.  The reference walks every node of
// every path once to count, once per merged edge to pair and once per merged edge to rebuild the path lists; here a POSITION of the
// concatenated paths is the unit of work and a round is one call.
//   host              validation (all of it before anything is launched), the depth and slot tables; one upload of the three arrays
//   k_topo_keys       one thread per position: its path (binary search), its successor, the 64-bit key of its edge; slot and block counts
//   k_topo_check      one thread per slot / block: every (block, member) named exactly once, every block as often as it is deep
//   rocPRIM           the keys sorted: the sorted order is the output order
//   k_topo_heads / _runs / _keep / _compact   run heads, (scan) run starts, count == depth of both blocks, (scan) the transitive list
//   host              the list comes back (small: through pinned memory); the greedy walk or the schedule check, the orientation, the
//                     per-block choice table -- sequential by definition, O(transitive edges)
//   k_topo_pair       one thread per position: whether the pair with its successor is an occurrence of a chosen edge -- then partner, the
//                     new node (XXH64 here), old_left / old_right -- and its own fate: kept, replaced by the new node, or dropped
//   k_topo_tile_sums / _tile_scan / _splice / _paths   the general splice (position -> 0 .. k nodes) in tiles of PGA_TOPO_TILE positions
// The kernels and the host tables are pga_topo_idx.h (no wave intrinsic: tests/emu/topo_emu.cpp runs them on the host).
// All arithmetic is integer; atomics feed only counts and minima, so the result does not depend on the launch geometry.
#include "pga_common.h"
#include "pga_graph_host.h"
#include "../../include/pga_align.h"
#include "pga_topo_idx.h"

namespace pga {

static unsigned tp_grid(uint64_t items, uint64_t per_block) { return grid_for(items, per_block, 2048); }

void plan_simplify_host(int64_t n_blocks, const pga_topo_block_t *blocks, int64_t n_paths, const pga_topo_path_t *paths, int64_t n_nodes, const pga_topo_node_t *nodes,
                        int64_t n_sched, const pga_topo_sched_t *sched, uint32_t flags, pga_topo_out_t *out)
{
	// ---- validation: everything the host can refuse is refused here ----
	TpTables T;
	tp_validate(n_blocks, blocks, n_paths, paths, n_nodes, nodes, n_sched, sched, flags, T);
	if (n_paths == 0 || n_nodes == 0) {
		TpRound R;
		tp_choose(n_blocks, blocks, nullptr, 0, n_sched, sched, R);         // (a schedule names edges that are not there)
		return;
	}
	const uint64_t nn = (uint64_t)n_nodes, np = (uint64_t)n_paths, nb = (uint64_t)n_blocks;
	// ---- the device: keys, checks, the sorted runs ----
	StreamLease stream;
	hipStream_t st = stream.s;
	DBuf<pga_topo_node_t> d_nodes(nn); DBuf<pga_topo_path_t> d_paths(np);
	DBuf<uint32_t> d_depth(nb), d_first(nb + 1), d_pathof(nn), d_cnts(T.n_slots + nb + 1), d_err(TP_ERRS);
	DBuf<tp_u64> d_key(nn), d_skey(nn);
	DBuf<uint32_t> d_head(nn + 1), d_hoff(nn + 1), d_rstart(nn + 1), d_keep(nn + 1), d_koff(nn + 1);
	DBuf<pga_topo_edge_t> d_trans(nn), d_counts;
	if (flags & PGA_TOPO_COUNTS) d_counts.alloc(nn);
	PGA_HIP(hipMemcpyAsync(d_nodes.p, nodes, nn * sizeof(pga_topo_node_t), hipMemcpyHostToDevice, st));
	PGA_HIP(hipMemcpyAsync(d_paths.p, paths, np * sizeof(pga_topo_path_t), hipMemcpyHostToDevice, st));
	PGA_HIP(hipMemcpyAsync(d_depth.p, T.depth.data(), nb * sizeof(uint32_t), hipMemcpyHostToDevice, st));
	PGA_HIP(hipMemcpyAsync(d_first.p, T.slot_first.data(), (nb + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
	d_cnts.zero(st);
	PGA_HIP(hipMemsetAsync(d_err.p, 0xff, TP_ERRS * sizeof(uint32_t), st));
	TpDev V;
	memset(&V, 0, sizeof(V));
	V.n_nodes = nn; V.n_paths = np; V.n_blocks = nb; V.n_slots = T.n_slots;
	V.nodes = d_nodes.p; V.paths = d_paths.p; V.depth = d_depth.p; V.slot_first = d_first.p; V.path_of = d_pathof.p; V.key = d_key.p;
	V.slot_cnt = d_cnts.p; V.blk_cnt = d_cnts.p + T.n_slots; V.err = d_err.p;
	V.skey = d_skey.p; V.head = d_head.p; V.head_off = d_hoff.p; V.run_start = d_rstart.p; V.keep = d_keep.p; V.keep_off = d_koff.p;
	V.o_trans = d_trans.p; V.o_counts = d_counts.p;
	const unsigned g_pos = tp_grid(nn + 1, TP_THREADS);
	hipLaunchKernelGGL(k_topo_keys, dim3(g_pos), dim3(TP_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_topo_check, dim3(tp_grid(std::max(T.n_slots, nb), TP_THREADS)), dim3(TP_THREADS), 0, st, V);
	radix_sort_keys(d_key.p, d_skey.p, nn, 64, st);
	hipLaunchKernelGGL(k_topo_heads, dim3(g_pos), dim3(TP_THREADS), 0, st, V);
	excl_scan(d_head.p, d_hoff.p, nn + 1, st);
	hipLaunchKernelGGL(k_topo_runs, dim3(g_pos), dim3(TP_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_topo_keep, dim3(g_pos), dim3(TP_THREADS), 0, st, V);
	excl_scan(d_keep.p, d_koff.p, nn + 1, st);
	hipLaunchKernelGGL(k_topo_compact, dim3(g_pos), dim3(TP_THREADS), 0, st, V);
	PGA_HIP(hipGetLastError());
	// ---- the first wait: the checks and the two list lengths; then the lists themselves ----
	uint32_t err[TP_ERRS], n_runs = 0, n_trans = 0;
	fetch(err, d_err.p, TP_ERRS, st); fetch(&n_runs, d_hoff.p + nn, 1, st); fetch(&n_trans, d_koff.p + nn, 1, st);
	PGA_HIP(sync_stream(st));
	if (err[TP_E_DEPTH] != TP_NONE) tp_fail("the nodes of a block do not sum to its depth (block " + std::to_string(err[TP_E_DEPTH]) + ")");
	if (err[TP_E_SLOT] != TP_NONE) {
		const uint32_t slot = err[TP_E_SLOT] >> 1;
		const uint32_t b = (uint32_t)(std::upper_bound(T.slot_first.begin(), T.slot_first.end() - 1, slot) - T.slot_first.begin()) - 1;
		tp_fail(std::string("a (block, member) slot is named by ") + ((err[TP_E_SLOT] & 1u) ? "two nodes" : "no node") + " (block " + std::to_string(b) + ", member " + std::to_string(slot - T.slot_first[b]) + ")");
	}
	if (n_runs > nn || n_trans > n_runs) tp_fail("internal: the device counted more edges than positions");
	std::vector<pga_topo_edge_t> trans;
	{
		Downloads dl(st);
		dl.add(trans, (const pga_topo_edge_t*)d_trans.p, n_trans);
		if (flags & PGA_TOPO_COUNTS) { out->edge_counts = host_array<pga_topo_edge_t>(n_runs, "pga_plan_simplify"); fetch(out->edge_counts, (const pga_topo_edge_t*)d_counts.p, n_runs, st); }
		dl.wait();
		PGA_HIP(sync_stream(st));
	}
	out->n_counts = (flags & PGA_TOPO_COUNTS) ? n_runs : 0;
	out->transitive = host_array<pga_topo_edge_t>(n_trans, "pga_plan_simplify");
	if (n_trans) memcpy(out->transitive, trans.data(), n_trans * sizeof(pga_topo_edge_t));
	out->n_transitive = n_trans;
	// ---- the round ----
	TpRound R;
	if (flags & PGA_TOPO_EDGES_ONLY) return;
	tp_choose(n_blocks, blocks, trans.data(), n_trans, n_sched, sched, R);
	const uint64_t n_round = R.round.size(), n_partner = R.n_partner;
	out->round = host_array<pga_topo_round_t>(n_round, "pga_plan_simplify");
	if (n_round == 0) return;
	memcpy(out->round, R.round.data(), n_round * sizeof(pga_topo_round_t));
	out->n_round = (int64_t)n_round; out->n_partner = (int64_t)n_partner;
	out->partner = host_array<uint32_t>(n_partner, "pga_plan_simplify"); out->new_nodes = host_array<pga_topo_node_t>(n_partner, "pga_plan_simplify");
	out->old_left = host_array<uint64_t>(n_partner, "pga_plan_simplify"); out->old_right = host_array<uint64_t>(n_partner, "pga_plan_simplify");
	out->blocks = host_array<pga_topo_block_t>(nb, "pga_plan_simplify"); out->paths = host_array<pga_topo_path_t>(np, "pga_plan_simplify");
	tp_blocks_after(n_blocks, blocks, R, out->blocks);
	// ---- the pairing and the splice ----
	const uint32_t n_tiles = (uint32_t)((nn + TP_TILE - 1) / TP_TILE);
	DBuf<uint32_t> d_choice(nb), d_partner(n_partner + 1), d_cnt(nn + 1), d_repl(nn), d_tsum(n_tiles), d_toff(n_tiles + 1), d_poff(nn + 1);
	DBuf<TpPick> d_pick(n_round); DBuf<pga_topo_node_t> d_new(n_partner + 1), d_onodes(nn); DBuf<uint64_t> d_left(n_partner + 1), d_right(n_partner + 1);
	DBuf<pga_topo_path_t> d_opaths(np);
	PGA_HIP(hipMemcpyAsync(d_choice.p, R.choice.data(), nb * sizeof(uint32_t), hipMemcpyHostToDevice, st));
	PGA_HIP(hipMemcpyAsync(d_pick.p, R.pick.data(), n_round * sizeof(TpPick), hipMemcpyHostToDevice, st));
	PGA_HIP(hipMemsetAsync(d_partner.p, 0xff, (n_partner + 1) * sizeof(uint32_t), st));
	V.choice = d_choice.p; V.pick = d_pick.p; V.o_partner = d_partner.p; V.o_new = d_new.p; V.o_left = d_left.p; V.o_right = d_right.p;
	V.cnt = d_cnt.p; V.repl = d_repl.p; V.n_tiles = n_tiles; V.tile_sum = d_tsum.p; V.tile_off = d_toff.p; V.pos_off = d_poff.p;
	V.o_nodes = d_onodes.p; V.o_paths = d_opaths.p;
	hipLaunchKernelGGL(k_topo_pair, dim3(g_pos), dim3(TP_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_topo_tile_sums, dim3(std::min<uint32_t>(n_tiles, 2048u)), dim3(TP_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_topo_tile_scan, dim3(1), dim3(TP_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_topo_splice, dim3(std::min<uint32_t>(n_tiles, 2048u)), dim3(TP_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_topo_paths, dim3(tp_grid(np, TP_THREADS)), dim3(TP_THREADS), 0, st, V);
	PGA_HIP(hipGetLastError());
	// every pair drops one node: the size of the node list is known without asking the device; its own count is held against it
	const uint64_t n_out = nn - n_partner;
	out->nodes = host_array<pga_topo_node_t>(n_out, "pga_plan_simplify");
	uint32_t total = 0;
	fetch(&total, (const uint32_t*)d_toff.p + n_tiles, 1, st);
	fetch(out->partner, (const uint32_t*)d_partner.p, n_partner, st); fetch(out->new_nodes, (const pga_topo_node_t*)d_new.p, n_partner, st);
	fetch(out->old_left, (const uint64_t*)d_left.p, n_partner, st); fetch(out->old_right, (const uint64_t*)d_right.p, n_partner, st);
	fetch(out->paths, (const pga_topo_path_t*)d_opaths.p, np, st);
	fetch(out->nodes, (const pga_topo_node_t*)d_onodes.p, n_out, st);   // (the splice writes at most n_nodes entries whatever it counted: d_onodes holds them)
	PGA_HIP(sync_stream(st));
	for (uint64_t e = 0; e < n_round; ++e) for (uint64_t k = 0; k < trans[R.round[e].transitive].count; ++k)
		if (out->partner[R.round[e].partner_off + k] == TP_NONE) tp_fail("a slot of a partner list was left unwritten (round edge " + std::to_string(e) + ", member " + std::to_string(k) + ")");
	if (total != n_out) tp_fail("internal: the splice wrote " + std::to_string(total) + " nodes, " + std::to_string(n_out) + " expected");
	out->n_blocks = n_blocks; out->n_paths = n_paths; out->n_nodes = (int64_t)n_out;
}

} // namespace pga
