// pga_join.hip -- graph_join (graph_merging.rs:74-93) on the two flat layouts: the child graphs of a guide-tree node put into one.  The
// reference inserts every block, path and node of the right graph into the left one's BTreeMaps and panics on a key that is there; here a
// BLOCK, a PATH, a NODE, an OUTPUT MEMBER, a LIST ELEMENT and a LETTER are the units of work.
//   host               validation per part (all of it before anything is launched), the parts' places in the concatenated buffers, the alive
//                      block ids; every array of every part uploaded straight to its place
//   k_join_keys        the sort keys of the paths and the nodes
//   k_join_ins         every insertion inside its own part's letters, then rebased to the concatenated letters
//   rocPRIM            the alive block ids and the path ids sorted with their concatenated index, the node ids alone
//   k_join_rank        the block and path tables after, block_map, path_map, equal neighbours of the three sorted lists
//   k_ts_* (pga_tile_scan.h)   before: where a member's lists start; blocks: the first member of a block after; paths: node_off after
//   k_join_desc        one thread per member after: descriptor, who, origin_part, origin
//   k_join_nodes / _check   one thread per node: its place after, the slot counts; one per slot: named exactly once
//   k_ts_*, out        where the lists start in the output
//   host               the first wait: the checks, the three list totals
//   k_assemble_copy<list>, k_ts_* letters   pga_assemble_idx.h: one thread per element of an output list; the insertion lengths
//   host               the second wait: the bounds of every insertion, the letter total
//   k_assemble_letters / _seq_off   one thread per letter
//   host               the third wait: the output; then the consensus pointers, or the copied letters (host copies on thread_ranges)
// The call waits for the device three times.  No consensus letter goes to the device.
// All arithmetic is integer; atomics feed only counts and minima, so the result does not depend on the launch geometry.
#include "pga_common.h"
#include "pga_graph_host.h"
#include "../../include/pga_align.h"
#include "pga_join_idx.h"
#include "pga_runs.h"

namespace pga {

static unsigned jn_grid(uint64_t items) { return grid_for(items, JN_THREADS, 2048); }
static unsigned jn_tile_grid(uint64_t items) { return grid_for(items, JN_TILE, 1u << 16); }

static thread_local double g_jn_ms[3] = {0, 0, 0};
void join_last_ms(double *ms) { for (int i = 0; i < 3; ++i) ms[i] = g_jn_ms[i]; }

template <class T> static void put(T *dst, const T *src, uint64_t n, hipStream_t st) { if (n) PGA_HIP(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, st)); }

void join_graphs_host(int32_t n_parts, const pga_join_part_t *parts, uint32_t flags, pga_join_out_t *out)
{
	const char *me = "pga_join_graphs";
	JnTables J;
	jn_validate(n_parts, parts, flags, J);
	const uint64_t P = (uint64_t)n_parts, nb = J.blk_off[P], np = J.path_off[P], nn = J.node_off[P], nm = J.mem_off[P], na = J.alive_id.size();
	const uint64_t ns = J.list_off[0][P], nd = J.list_off[1][P], ni = J.ins_off[P], nl = J.let_off[P];
	out->n_parts = n_parts; out->n_blocks = (int64_t)na; out->n_paths = (int64_t)np; out->n_nodes = (int64_t)nn; out->n_members = (int64_t)nm;
	out->blocks = host_array<pga_topo_block_t>(na, me); out->paths = host_array<pga_topo_path_t>(np, me); out->nodes = host_array<pga_topo_node_t>(nn, me);
	out->rc_blocks = host_array<pga_rc_block_t>(na, me); out->members = host_array<pga_rc_member_t>(nm, me);
	out->who = host_array<pga_detach_member_t>(nm, me); out->origin = host_array<int64_t>(nm, me); out->origin_part = host_array<int32_t>(nm, me);
	out->block_map = host_array<uint32_t>(nb, me); out->path_map = host_array<uint32_t>(np, me);
	out->block_map_off = host_array<uint64_t>(P + 1, me); out->path_map_off = host_array<uint64_t>(P + 1, me);
	std::copy(J.blk_off.begin(), J.blk_off.end(), out->block_map_off); std::copy(J.path_off.begin(), J.path_off.end(), out->path_map_off);
	if (nb == 0 && np == 0) {                                                  // every part is empty: nothing to launch
		out->subs = host_array<pga_sub_t>(0, me); out->dels = host_array<pga_del_t>(0, me); out->inss = host_array<pga_ins_t>(0, me);
		out->ins_seq = host_array<char>(0, me); out->cons = host_array<char>(0, me);
		return;
	}
	StreamLease stream;
	hipStream_t st = stream.s;
	StageClock clock(st);
	clock.at(0);
	// ---- the uploads: every part's arrays straight to their place (every buffer one entry longer than its count: none is empty) ----
	DBuf<pga_topo_block_t> d_blocks(nb + 1), d_oblocks(na + 1); DBuf<pga_topo_path_t> d_paths(np + 1), d_opaths(np + 1); DBuf<pga_topo_node_t> d_nodes(nn + 1), d_onodes(nn + 1);
	DBuf<pga_rc_member_t> d_members(nm + 1), d_omembers(nm + 1); DBuf<pga_detach_member_t> d_who(nm + 1), d_owho(nm + 1);
	DBuf<pga_sub_t> d_subs(ns + 1); DBuf<pga_del_t> d_dels(nd + 1); DBuf<pga_ins_t> d_inss(ni + 1); DBuf<char> d_letters(nl + 1);
	DBuf<jn_u64> d_off(6 * (P + 1)), d_aid(na + 1), d_sbid(na + 1), d_pid(np + 1), d_spid(np + 1), d_nid(nn + 1), d_snid(nn + 1), d_err(JN_ERRS), d_aerr(AS_ERRS);
	DBuf<uint32_t> d_first(nb + 1), d_ablock(na + 1), d_sblock(na + 1), d_pidx(np + 1), d_spath(np + 1), d_osrc(na + 1), d_bmap(nb + 1), d_pmap(np + 1), d_cnt(nm + 1), d_hit(JN_ERRS);
	DBuf<int32_t> d_opart(nm + 1); DBuf<long long> d_origin(nm + 1); DBuf<AsDesc> d_desc(nm + 1);
	for (int32_t p = 0; p < n_parts; ++p) {
		const pga_join_part_t &X = parts[p];
		put(d_blocks.p + J.blk_off[p], X.blocks, J.blk_off[p + 1] - J.blk_off[p], st); put(d_paths.p + J.path_off[p], X.paths, J.path_off[p + 1] - J.path_off[p], st);
		put(d_nodes.p + J.node_off[p], X.nodes, J.node_off[p + 1] - J.node_off[p], st);
		put(d_members.p + J.mem_off[p], X.members, J.mem_off[p + 1] - J.mem_off[p], st); put(d_who.p + J.mem_off[p], X.who, J.mem_off[p + 1] - J.mem_off[p], st);
		put(d_subs.p + J.list_off[0][p], X.subs, J.list_off[0][p + 1] - J.list_off[0][p], st); put(d_dels.p + J.list_off[1][p], X.dels, J.list_off[1][p + 1] - J.list_off[1][p], st);
		put(d_inss.p + J.ins_off[p], X.inss, J.ins_off[p + 1] - J.ins_off[p], st); put(d_letters.p + J.let_off[p], X.ins_seq, J.let_off[p + 1] - J.let_off[p], st);
	}
	const std::vector<jn_u64> *offs[6] = {&J.blk_off, &J.path_off, &J.node_off, &J.mem_off, &J.ins_off, &J.let_off};
	for (int k = 0; k < 6; ++k) put(d_off.p + k * (P + 1), offs[k]->data(), P + 1, st);
	put(d_first.p, J.first_member.data(), nb + 1, st); put(d_aid.p, J.alive_id.data(), na, st); put(d_ablock.p, J.alive_block.data(), na, st);
	clock.at(1);
	// ---- the checks, the order, the tables after ----
	d_cnt.zero(st); d_hit.zero(st);
	PGA_HIP(hipMemsetAsync(d_err.p, 0xff, JN_ERRS * sizeof(jn_u64), st));
	PGA_HIP(hipMemsetAsync(d_aerr.p, 0xff, AS_ERRS * sizeof(as_u64), st));
	PGA_HIP(hipMemsetAsync(d_bmap.p, 0xff, (nb + 1) * sizeof(uint32_t), st));
	PGA_HIP(hipMemsetAsync(d_pmap.p, 0xff, (np + 1) * sizeof(uint32_t), st));
	TileScanBufs<jn_u64> b_before, b_blocks, b_paths, b_out, b_let;
	JnDev V;
	memset(&V, 0, sizeof(V));
	V.n_parts = P; V.n_blocks = nb; V.n_paths = np; V.n_nodes = nn; V.n_members = nm; V.n_alive = na; V.n_inss = ni;
	V.blk_off = d_off.p; V.path_off = d_off.p + (P + 1); V.node_off = d_off.p + 2 * (P + 1); V.mem_off = d_off.p + 3 * (P + 1); V.ins_off = d_off.p + 4 * (P + 1); V.let_off = d_off.p + 5 * (P + 1);
	V.blocks = d_blocks.p; V.paths = d_paths.p; V.nodes = d_nodes.p; V.first_member = d_first.p; V.who = d_who.p; V.inss = d_inss.p;
	V.path_id = d_pid.p; V.node_id = d_nid.p; V.path_idx = d_pidx.p;
	V.s_block_id = d_sbid.p; V.s_block = d_sblock.p; V.s_path_id = d_spid.p; V.s_path = d_spath.p; V.s_node_id = d_snid.p;
	V.o_blocks = d_oblocks.p; V.o_src = d_osrc.p; V.o_paths = d_opaths.p; V.o_nodes = d_onodes.p; V.block_map = d_bmap.p; V.path_map = d_pmap.p;
	V.o_who = d_owho.p; V.o_part = d_opart.p; V.slot_cnt = d_cnt.p; V.err = d_err.p; V.hit = d_hit.p;
	V.A.n_out_members = nm; V.A.ins_seq_len = nl; V.A.p_ins_seq_len = 0;
	V.A.members = d_members.p; V.A.subs = d_subs.p; V.A.dels = d_dels.p; V.A.inss = d_inss.p; V.A.letters = d_letters.p;
	V.A.desc = d_desc.p; V.A.o_members = d_omembers.p; V.A.origin = d_origin.p; V.A.err = d_aerr.p;
	V.scan[JN_SCAN_BEFORE] = b_before.make(nm, 3); V.scan[JN_SCAN_BLOCKS] = b_blocks.make(na, 1); V.scan[JN_SCAN_PATHS] = b_paths.make(np, 1);
	V.A.scan[AS_SCAN_OUT] = b_out.make(nm, 3);
	hipLaunchKernelGGL(k_join_keys, dim3(jn_grid(std::max(np, nn))), dim3(JN_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_join_ins, dim3(jn_grid(ni)), dim3(JN_THREADS), 0, st, V);
	tile_scan_launch(V.scan[JN_SCAN_BEFORE], AsBeforeValue{V.A}, st);
	radix_sort_pairs<jn_u64>(d_aid.p, d_sbid.p, d_ablock.p, d_sblock.p, na, 64, st);
	radix_sort_pairs<jn_u64>(d_pid.p, d_spid.p, d_pidx.p, d_spath.p, np, 64, st);
	if (nn) radix_sort_keys<jn_u64>(d_nid.p, d_snid.p, nn, 64, st);
	hipLaunchKernelGGL(k_join_rank, dim3(jn_grid(std::max(std::max(na, np), nn))), dim3(JN_THREADS), 0, st, V);
	tile_scan_launch(V.scan[JN_SCAN_BLOCKS], JnDepthValue{V}, st);
	tile_scan_launch(V.scan[JN_SCAN_PATHS], JnPathValue{V}, st);
	hipLaunchKernelGGL(k_join_desc, dim3(jn_grid(nm)), dim3(JN_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_join_nodes, dim3(jn_grid(std::max(np, nn))), dim3(JN_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_join_check, dim3(jn_grid(nm)), dim3(JN_THREADS), 0, st, V);
	tile_scan_launch(V.A.scan[AS_SCAN_OUT], AsOutValue{V.A}, st);
	PGA_HIP(hipGetLastError());
	// ---- the first wait: nothing behind it runs on input that was not checked ----
	jn_u64 err[JN_ERRS], tot[3], n_mem_dev = 0, n_node_dev = 0;
	uint32_t hit[JN_ERRS];
	as_u64 aerr[AS_ERRS];
	fetch(err, (const jn_u64*)d_err.p, JN_ERRS, st); fetch(hit, (const uint32_t*)d_hit.p, JN_ERRS, st);
	for (int q = 0; q < 3; ++q) fetch(&tot[q], ts_off(V.A.scan[AS_SCAN_OUT], q) + nm, 1, st);
	fetch(&n_mem_dev, ts_off(V.scan[JN_SCAN_BLOCKS], 0) + na, 1, st); fetch(&n_node_dev, ts_off(V.scan[JN_SCAN_PATHS], 0) + np, 1, st);
	PGA_HIP(sync_stream(st));
	jn_report_host(n_parts, parts, err, hit, J);
	if (n_mem_dev != nm || n_node_dev != nn || tot[0] != ns || tot[1] != nd || tot[2] != ni) jn_fail("internal: the device and the host disagree on the totals");
	// ---- the three lists, the letter scan ----
	DBuf<pga_sub_t> d_osubs(ns + 1); DBuf<pga_del_t> d_odels(nd + 1); DBuf<pga_ins_t> d_oinss(ni + 1);
	V.A.o_subs = d_osubs.p; V.A.o_dels = d_odels.p; V.A.o_inss = d_oinss.p;
	if (ns) hipLaunchKernelGGL(k_assemble_copy<RM_LIST_SUB>, dim3(jn_tile_grid(ns)), dim3(AS_THREADS), 0, st, V.A);
	if (nd) hipLaunchKernelGGL(k_assemble_copy<RM_LIST_DEL>, dim3(jn_tile_grid(nd)), dim3(AS_THREADS), 0, st, V.A);
	if (ni) hipLaunchKernelGGL(k_assemble_copy<RM_LIST_INS>, dim3(jn_tile_grid(ni)), dim3(AS_THREADS), 0, st, V.A);
	V.A.scan[AS_SCAN_LETTERS] = b_let.make(ni, 1);
	tile_scan_launch(V.A.scan[AS_SCAN_LETTERS], AsLetterValue{V.A}, st);
	PGA_HIP(hipGetLastError());
	// ---- the second wait: every insertion lies inside the letters before one is read ----
	as_u64 n_let = 0;
	fetch(aerr, (const as_u64*)d_aerr.p, AS_ERRS, st); fetch(&n_let, ts_off(V.A.scan[AS_SCAN_LETTERS], 0) + ni, 1, st);
	PGA_HIP(sync_stream(st));
	if (aerr[AS_E_SEQ_RANGE] != AS_NONE) jn_fail("internal: an insertion that passed its part's range lies beyond the letters (insertion " + std::to_string(aerr[AS_E_SEQ_RANGE]) + " of the output)");
	const uint64_t nl_out = n_let;
	DBuf<char> d_oseq(nl_out + 1);
	V.A.o_ins_seq = d_oseq.p;
	if (nl_out) hipLaunchKernelGGL(k_assemble_letters, dim3(jn_tile_grid(nl_out)), dim3(AS_THREADS), 0, st, V.A);
	if (ni) hipLaunchKernelGGL(k_assemble_seq_off, dim3(jn_grid(ni)), dim3(AS_THREADS), 0, st, V.A);
	PGA_HIP(hipGetLastError());
	clock.at(2);
	// ---- the output ----
	out->subs = host_array<pga_sub_t>(ns, me); out->dels = host_array<pga_del_t>(nd, me); out->inss = host_array<pga_ins_t>(ni, me);
	out->ins_seq = host_array<char>(nl_out + 1, me);
	fetch(out->blocks, (const pga_topo_block_t*)d_oblocks.p, na, st); fetch(out->paths, (const pga_topo_path_t*)d_opaths.p, np, st); fetch(out->nodes, (const pga_topo_node_t*)d_onodes.p, nn, st);
	fetch(out->members, (const pga_rc_member_t*)d_omembers.p, nm, st); fetch((long long*)out->origin, (const long long*)d_origin.p, nm, st);
	fetch(out->origin_part, (const int32_t*)d_opart.p, nm, st); fetch(out->who, (const pga_detach_member_t*)d_owho.p, nm, st);
	fetch(out->block_map, (const uint32_t*)d_bmap.p, nb, st); fetch(out->path_map, (const uint32_t*)d_pmap.p, np, st);
	fetch(out->subs, (const pga_sub_t*)d_osubs.p, ns, st); fetch(out->dels, (const pga_del_t*)d_odels.p, nd, st);
	fetch(out->inss, (const pga_ins_t*)d_oinss.p, ni, st); fetch(out->ins_seq, (const char*)d_oseq.p, nl_out, st);
	clock.at(3);
	PGA_HIP(sync_stream(st));
	clock.read(g_jn_ms);
	out->n_subs = ns; out->n_dels = nd; out->n_inss = ni; out->n_ins_letters = nl_out;
	// ---- the consensus of every block after: the part's pointer, or letters this call owns (every sequence at a multiple of 16) ----
	const bool copy_all = (flags & PGA_JOIN_COPY_CONSENSUS) != 0;
	std::vector<const char*> src(na, nullptr); std::vector<uint64_t> at(na, ~0ULL);
	for (int32_t p = 0; p < n_parts; ++p) for (int64_t b = 0; b < parts[p].n_blocks; ++b) {
		const uint32_t i = out->block_map[J.blk_off[p] + (uint64_t)b];
		if (i != TP_NONE) src[i] = parts[p].rc_blocks[b].consensus;
	}
	uint64_t n_cons = 0;
	if (copy_all) for (uint64_t i = 0; i < na; ++i) { at[i] = n_cons; n_cons += ((uint64_t)out->blocks[i].cons_len + 15) / 16 * 16; }
	out->cons = host_array<char>(n_cons + 1, me); out->n_cons_letters = n_cons;
	thread_ranges(na, range_threads(), [&](int, uint64_t i0, uint64_t i1) {
		for (uint64_t i = i0; i < i1; ++i) {
			const uint32_t len = out->blocks[i].cons_len;
			if (copy_all && len) memcpy(out->cons + at[i], src[i], len);
			out->rc_blocks[i] = pga_rc_block_t{copy_all ? out->cons + at[i] : src[i], len, out->blocks[i].depth};
		}
	});
}

} // namespace pga
