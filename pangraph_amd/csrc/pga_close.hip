// pga_close.hip -- the tail of a self-merge round folded back into the two flat layouts: what self_merge (graph_merging.rs:153-169) and
// reconsensus_graph (reconsensus.rs:46-91) do with the results of detach_unaligned_nodes, reconsensus and the second detach_unaligned_nodes.
// The reference removes and inserts blocks and nodes in BTreeMaps, one orphan at a time; here a MERGED MEMBER, a BLOCK AFTER, an OUTPUT
// MEMBER, a path POSITION, a LIST ELEMENT and a LETTER are the units of work.
//   host               validation (all of it before anything is launched), the per-block first places of the two stages, the alive ids,
//                      the orphan records of both stages behind each other; one upload
//   k_topo_keys / _check   pga_topo_idx.h: every (block, member) slot of the graph named exactly once
//   k_ts_* (pga_tile_scan.h)   before: where a survivor's lists start; second: where the lists of the second detach's members start;
//                      kept1 / kept2: the rank of a kept member in its stage
//   k_close_stage<1|2> the two member_maps against what they must be, the per-block counts, the kind of an orphan's block
//   k_close_chain      one thread per merged member: which final place or which orphan it became
//   rocPRIM            the singleton ids, sorted with their orphan numbers
//   k_close_rank       singletons and alive blocks: their index after, the block table, block_map, the duplicate ids
//   k_ts_*, blocks     the first output member of every block after
//   k_close_desc       one thread per output member: descriptor, origin, who, the orphan record after, the place of its origin
//   k_close_nodes      one thread per position: block, member and an orphan's strand
//   k_ts_*, out        where the lists start in the output
//   host               the first wait: the checks, the three list totals
//   k_assemble_copy<list>, k_ts_* letters   pga_assemble_idx.h: one thread per element of an output list; the insertion lengths
//   host               the second wait: the bounds of every insertion, the letter total
//   k_assemble_letters / _seq_off   one thread per letter
//   host               the third wait: the output; then the consensus pointers and the letters this call owns (host copies on thread_ranges)
// The call waits for the device three times.  No consensus letter goes to the device.
// All arithmetic is integer; atomics feed only counts and minima, so the result does not depend on the launch geometry.
#include "pga_common.h"
#include "pga_graph_host.h"
#include "../../include/pga_align.h"
#include "pga_close_idx.h"
#include "pga_runs.h"

namespace pga {

static unsigned cl_grid(uint64_t items) { return grid_for(items, CL_THREADS, 2048); }
static unsigned cl_tile_grid(uint64_t items) { return grid_for(items, CL_TILE, 1u << 16); }

// the stream's clock at four places of the last call of this thread: upload, kernels (their waits included), download, in ms
static thread_local double g_cl_ms[3] = {0, 0, 0};
void close_last_ms(double *ms) { for (int i = 0; i < 3; ++i) ms[i] = g_cl_ms[i]; }

void rc_detach_args_host(int64_t n_upd, const pga_detach_out_t *detached, const pga_detach_member_t *who_merged, const pga_rc_out_t *rc,
                         pga_rc_block_t *blocks, pga_rc_member_t *members, pga_detach_member_t *who2)
{
	cl_detach_args(n_upd, detached, who_merged, rc, blocks, members, who2);
}

void close_round_host(int64_t n_blocks, const pga_topo_block_t *blocks, int64_t n_paths, const pga_topo_path_t *paths, int64_t n_nodes, const pga_topo_node_t *nodes,
                      const pga_rc_block_t *rc_blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss,
                      const char *ins_seq, uint64_t ins_seq_len, const pga_detach_member_t *who, int64_t n_upd, const uint32_t *upd,
                      const pga_detach_out_t *detached, const pga_rc_out_t *rc, uint64_t rc_ins_seq_len, const pga_detach_out_t *redetached,
                      uint32_t flags, pga_close_out_t *out)
{
	const char *me = "pga_close_round";
	ClTables C;
	cl_validate(n_blocks, blocks, n_paths, paths, n_nodes, nodes, rc_blocks, members, subs, dels, inss, who, n_upd, upd, detached, rc, redetached, flags, C);
	if (!ins_seq) ins_seq_len = 0;                                            // (a NULL buffer holds no letter: an insertion with letters is refused by its range)
	if (!n_upd || !rc->ins_seq) rc_ins_seq_len = 0;
	const uint64_t nb = (uint64_t)n_blocks, np = (uint64_t)n_paths, nn = (uint64_t)n_nodes, nu = (uint64_t)n_upd, nm = C.n_before, nm1 = C.n_merged, k1 = C.n_k1, k2 = C.n_k2;
	const uint64_t no = C.n_o1 + C.n_o2, na = C.alive_id.size(), nbo = C.n_out_blocks, nmo = C.n_out_members;
	out->n_blocks = (int64_t)nbo; out->n_paths = n_paths; out->n_nodes = n_nodes; out->n_members = (int64_t)nmo; out->n_orphans = (int64_t)no;
	out->blocks = host_array<pga_topo_block_t>(nbo, me); out->paths = host_array<pga_topo_path_t>(np, me); out->nodes = host_array<pga_topo_node_t>(nn, me);
	out->rc_blocks = host_array<pga_rc_block_t>(nbo, me); out->members = host_array<pga_rc_member_t>(nmo, me);
	out->who = host_array<pga_detach_member_t>(nmo, me); out->origin = host_array<int64_t>(nmo, me); out->block_map = host_array<uint32_t>(nb, me);
	out->kinds = host_array<int32_t>(nu, me); out->orphans = host_array<pga_detach_orphan_t>(no, me);
	if (np) std::copy(paths, paths + np, out->paths);
	std::copy(C.kinds.begin(), C.kinds.end(), out->kinds);
	if (nb == 0) {                                                            // no block, so no member and no node (cl_validate): nothing to launch
		out->subs = host_array<pga_sub_t>(0, me); out->dels = host_array<pga_del_t>(0, me); out->inss = host_array<pga_ins_t>(0, me);
		out->ins_seq = host_array<char>(0, me); out->cons = host_array<char>(0, me);
		return;
	}
	StreamLease stream;
	hipStream_t st = stream.s;
	StageClock clock(st);
	clock.at(0);
	// ---- the uploads (every buffer one entry longer than its count: none is empty) ----
	DBuf<pga_topo_node_t> d_nodes(nn + 1), d_onodes(nn + 1); DBuf<pga_topo_path_t> d_paths(np + 1); DBuf<pga_topo_block_t> d_blocks(nb + 1), d_oblocks(nbo + 1);
	DBuf<uint32_t> d_depth(nb + 1), d_first(nb + 1), d_upd(nu + 1), d_rclen(nu + 1), d_ablock(na + 1), d_aupd(na + 1), d_map(nb + 1), d_sorph(no + 1), d_iota(no + 1);
	DBuf<int32_t> d_kinds(nu + 1);
	DBuf<cl_u64> d_mfirst(nu + 1), d_r1first(nu + 1), d_r2first(nu + 1), d_aid(na + 1), d_oid(no + 1), d_sid(no + 1), d_fin(k2 + 1), d_osrc(no + 1), d_err(CL_ERRS), d_aerr(AS_ERRS);
	DBuf<long long> d_map1(nm1 + 1), d_map2(k1 + 1), d_origin(nmo + 1);
	DBuf<pga_rc_member_t> d_members(nm + 1), d_members2(k2 + 1), d_omembers(nmo + 1);
	DBuf<pga_sub_t> d_subs(C.before_tot[0] + 1), d_subs2(C.second_tot[0] + 1); DBuf<pga_del_t> d_dels(C.before_tot[1] + 1), d_dels2(C.second_tot[1] + 1);
	DBuf<pga_ins_t> d_inss(C.before_tot[2] + 1), d_inss2(C.second_tot[2] + 1);
	DBuf<char> d_letters(ins_seq_len + rc_ins_seq_len + 1);
	DBuf<pga_detach_orphan_t> d_orph(no + 1), d_oorph(no + 1); DBuf<pga_detach_member_t> d_who(nm + 1), d_owho(nmo + 1);
	DBuf<ClBlock> d_rec(nbo + 1); DBuf<ClWhere> d_where(nm + 1); DBuf<AsDesc> d_desc(nmo + 1);
	std::vector<cl_u64> oid(no); std::vector<uint32_t> iota(no);
	for (uint64_t k = 0; k < no; ++k) { oid[k] = C.orphans[k].block_id; iota[k] = (uint32_t)k; }
	upload(d_nodes, nodes, nn, st); upload(d_paths, paths, np, st); upload(d_blocks, blocks, nb, st);
	upload(d_depth, C.T.depth.data(), nb, st); upload(d_first, C.T.slot_first.data(), nb + 1, st);
	upload(d_upd, upd, nu, st); upload(d_rclen, C.rc_len.data(), nu, st); upload(d_kinds, C.kinds.data(), nu, st);
	upload(d_mfirst, (const cl_u64*)C.mfirst.data(), nu + 1, st); upload(d_r1first, (const cl_u64*)C.r1first.data(), nu + 1, st); upload(d_r2first, (const cl_u64*)C.r2first.data(), nu + 1, st);
	upload(d_aid, (const cl_u64*)C.alive_id.data(), na, st); upload(d_ablock, C.alive_block.data(), na, st); upload(d_aupd, C.alive_upd.data(), na, st);
	upload(d_oid, (const cl_u64*)oid.data(), no, st); upload(d_iota, iota.data(), no, st); upload(d_orph, C.orphans.data(), no, st);
	upload(d_members, members, nm, st); upload(d_subs, subs, C.before_tot[0], st); upload(d_dels, dels, C.before_tot[1], st); upload(d_inss, inss, C.before_tot[2], st);
	upload(d_who, who, nm, st);
	if (ins_seq_len) PGA_HIP(hipMemcpyAsync(d_letters.p, ins_seq, ins_seq_len, hipMemcpyHostToDevice, st));
	if (nu) {
		upload(d_map1, (const long long*)detached->member_map, nm1, st); upload(d_map2, (const long long*)redetached->member_map, k1, st);
		upload(d_members2, redetached->members, k2, st);
		upload(d_subs2, redetached->subs, C.second_tot[0], st); upload(d_dels2, redetached->dels, C.second_tot[1], st); upload(d_inss2, redetached->inss, C.second_tot[2], st);
		if (rc_ins_seq_len) PGA_HIP(hipMemcpyAsync(d_letters.p + ins_seq_len, rc->ins_seq, rc_ins_seq_len, hipMemcpyHostToDevice, st));
	}
	clock.at(1);
	// ---- the checks of the graph, the two stages, the chain ----
	DBuf<uint32_t> d_pathof(nn + 1), d_cnts(nm + nb + 1), d_terr(TP_ERRS);
	DBuf<tp_u64> d_key(nn + 1);
	d_cnts.zero(st);
	PGA_HIP(hipMemsetAsync(d_terr.p, 0xff, TP_ERRS * sizeof(uint32_t), st));
	PGA_HIP(hipMemsetAsync(d_err.p, 0xff, CL_ERRS * sizeof(cl_u64), st));
	PGA_HIP(hipMemsetAsync(d_aerr.p, 0xff, AS_ERRS * sizeof(as_u64), st));
	PGA_HIP(hipMemsetAsync(d_fin.p, 0xff, (k2 + 1) * sizeof(cl_u64), st));
	PGA_HIP(hipMemsetAsync(d_osrc.p, 0xff, (no + 1) * sizeof(cl_u64), st));
	PGA_HIP(hipMemsetAsync(d_rec.p, 0xff, (nbo + 1) * sizeof(ClBlock), st));
	PGA_HIP(hipMemsetAsync(d_where.p, 0xff, (nm + 1) * sizeof(ClWhere), st));
	PGA_HIP(hipMemsetAsync(d_map.p, 0xff, (nb + 1) * sizeof(uint32_t), st));
	d_oorph.zero(st); d_owho.zero(st);
	TpDev T;
	memset(&T, 0, sizeof(T));
	T.n_nodes = nn; T.n_paths = np; T.n_blocks = nb; T.n_slots = nm;
	T.nodes = d_nodes.p; T.paths = d_paths.p; T.depth = d_depth.p; T.slot_first = d_first.p; T.path_of = d_pathof.p; T.key = d_key.p;
	T.slot_cnt = d_cnts.p; T.blk_cnt = d_cnts.p + nm; T.err = d_terr.p;
	TileScanBufs<cl_u64> b_before, b_second, b_kept1, b_kept2, b_blocks, b_out, b_let;
	ClDev V;
	memset(&V, 0, sizeof(V));
	V.n_upd = nu; V.n_merged = nm1; V.n_k1 = k1; V.n_k2 = k2; V.n_o1 = C.n_o1; V.n_orphans = no; V.n_alive = na; V.n_blocks = nb; V.n_out_blocks = nbo; V.n_nodes = nn;
	V.blocks = d_blocks.p; V.nodes = d_nodes.p; V.first_member = d_first.p; V.upd = d_upd.p; V.mfirst = d_mfirst.p; V.r1first = d_r1first.p; V.r2first = d_r2first.p;
	V.rc_len = d_rclen.p; V.kinds = d_kinds.p; V.map1 = d_map1.p; V.map2 = d_map2.p; V.members2 = d_members2.p; V.orphans = d_orph.p; V.who = d_who.p;
	V.alive_id = d_aid.p; V.alive_block = d_ablock.p; V.alive_upd = d_aupd.p; V.sing_id = d_sid.p; V.sing_orphan = d_sorph.p; V.fin_src = d_fin.p; V.orph_src = d_osrc.p;
	V.o_rec = d_rec.p; V.o_blocks = d_oblocks.p; V.block_map = d_map.p; V.where = d_where.p; V.o_who = d_owho.p; V.o_orphans = d_oorph.p; V.o_nodes = d_onodes.p; V.err = d_err.p;
	V.A.n_out_members = nmo; V.A.ins_seq_len = ins_seq_len; V.A.p_ins_seq_len = rc_ins_seq_len;
	V.A.members = d_members.p; V.A.subs = d_subs.p; V.A.dels = d_dels.p; V.A.inss = d_inss.p;
	V.A.p_subs = d_subs2.p; V.A.p_dels = d_dels2.p; V.A.p_inss = d_inss2.p; V.A.letters = d_letters.p;
	V.A.desc = d_desc.p; V.A.o_members = d_omembers.p; V.A.origin = d_origin.p; V.A.err = d_aerr.p;
	V.scan[CL_SCAN_BEFORE] = b_before.make(nm, 3); V.scan[CL_SCAN_SECOND] = b_second.make(k2, 3);
	V.scan[CL_SCAN_KEPT1] = b_kept1.make(nm1, 1); V.scan[CL_SCAN_KEPT2] = b_kept2.make(k1, 1);
	V.scan[CL_SCAN_BLOCKS] = b_blocks.make(nbo, 1); V.A.scan[AS_SCAN_OUT] = b_out.make(nmo, 3);
	hipLaunchKernelGGL(k_topo_keys, dim3(cl_grid(nn)), dim3(TP_THREADS), 0, st, T);
	hipLaunchKernelGGL(k_topo_check, dim3(cl_grid(std::max(nm, nb))), dim3(TP_THREADS), 0, st, T);
	tile_scan_launch(V.scan[CL_SCAN_BEFORE], AsBeforeValue{V.A}, st);
	tile_scan_launch(V.scan[CL_SCAN_SECOND], ClSecondValue{V}, st);
	tile_scan_launch(V.scan[CL_SCAN_KEPT1], ClKeptValue{V.map1, k1}, st);
	tile_scan_launch(V.scan[CL_SCAN_KEPT2], ClKeptValue{V.map2, k2}, st);
	hipLaunchKernelGGL(k_close_stage<1>, dim3(cl_grid(std::max(nm1, nu))), dim3(CL_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_close_stage<2>, dim3(cl_grid(std::max(k1, nu))), dim3(CL_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_close_chain, dim3(cl_grid(nm1)), dim3(CL_THREADS), 0, st, V);
	// ---- the block table after, the descriptors, the nodes ----
	radix_sort_pairs<cl_u64>(d_oid.p, d_sid.p, d_iota.p, d_sorph.p, no, 64, st);
	hipLaunchKernelGGL(k_close_rank, dim3(cl_grid(std::max(no, na))), dim3(CL_THREADS), 0, st, V);
	tile_scan_launch(V.scan[CL_SCAN_BLOCKS], ClDepthValue{V}, st);
	hipLaunchKernelGGL(k_close_desc, dim3(cl_grid(nmo)), dim3(CL_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_close_nodes, dim3(cl_grid(nn)), dim3(CL_THREADS), 0, st, V);
	tile_scan_launch(V.A.scan[AS_SCAN_OUT], AsOutValue{V.A}, st);
	PGA_HIP(hipGetLastError());
	// ---- the first wait: nothing behind it runs on input that was not checked ----
	uint32_t terr[TP_ERRS];
	cl_u64 err[CL_ERRS], tot[3], n_mem_dev = 0;
	as_u64 aerr[AS_ERRS];
	fetch(terr, (const uint32_t*)d_terr.p, TP_ERRS, st); fetch(err, (const cl_u64*)d_err.p, CL_ERRS, st);
	for (int q = 0; q < 3; ++q) fetch(&tot[q], ts_off(V.A.scan[AS_SCAN_OUT], q) + nmo, 1, st);
	fetch(&n_mem_dev, ts_off(V.scan[CL_SCAN_BLOCKS], 0) + nbo, 1, st);
	PGA_HIP(sync_stream(st));
	cl_report(terr, err, C);
	const uint64_t ns_out = tot[0], nd_out = tot[1], ni_out = tot[2];
	if (n_mem_dev != nmo || ns_out > C.before_tot[0] + C.second_tot[0] || nd_out > C.before_tot[1] + C.second_tot[1] || ni_out > C.before_tot[2] + C.second_tot[2])
		cl_fail("internal: the device and the host disagree on the totals");
	// ---- the three lists, the letter scan ----
	DBuf<pga_sub_t> d_osubs(ns_out + 1); DBuf<pga_del_t> d_odels(nd_out + 1); DBuf<pga_ins_t> d_oinss(ni_out + 1);
	V.A.o_subs = d_osubs.p; V.A.o_dels = d_odels.p; V.A.o_inss = d_oinss.p;
	if (ns_out) hipLaunchKernelGGL(k_assemble_copy<RM_LIST_SUB>, dim3(cl_tile_grid(ns_out)), dim3(AS_THREADS), 0, st, V.A);
	if (nd_out) hipLaunchKernelGGL(k_assemble_copy<RM_LIST_DEL>, dim3(cl_tile_grid(nd_out)), dim3(AS_THREADS), 0, st, V.A);
	if (ni_out) hipLaunchKernelGGL(k_assemble_copy<RM_LIST_INS>, dim3(cl_tile_grid(ni_out)), dim3(AS_THREADS), 0, st, V.A);
	V.A.scan[AS_SCAN_LETTERS] = b_let.make(ni_out, 1);
	tile_scan_launch(V.A.scan[AS_SCAN_LETTERS], AsLetterValue{V.A}, st);
	PGA_HIP(hipGetLastError());
	// ---- the second wait: every insertion lies inside its buffer before a letter is read ----
	as_u64 n_let = 0;
	fetch(aerr, (const as_u64*)d_aerr.p, AS_ERRS, st); fetch(&n_let, ts_off(V.A.scan[AS_SCAN_LETTERS], 0) + ni_out, 1, st);
	PGA_HIP(sync_stream(st));
	cl_report_letters(aerr);
	const uint64_t nl_out = n_let;
	DBuf<char> d_oseq(nl_out + 1);
	V.A.o_ins_seq = d_oseq.p;
	if (nl_out) hipLaunchKernelGGL(k_assemble_letters, dim3(cl_tile_grid(nl_out)), dim3(AS_THREADS), 0, st, V.A);
	if (ni_out) hipLaunchKernelGGL(k_assemble_seq_off, dim3(cl_grid(ni_out)), dim3(AS_THREADS), 0, st, V.A);
	PGA_HIP(hipGetLastError());
	clock.at(2);
	// ---- the output ----
	std::vector<ClBlock> rec(nbo);
	out->subs = host_array<pga_sub_t>(ns_out, me); out->dels = host_array<pga_del_t>(nd_out, me); out->inss = host_array<pga_ins_t>(ni_out, me);
	out->ins_seq = host_array<char>(nl_out + 1, me);
	fetch(out->blocks, (const pga_topo_block_t*)d_oblocks.p, nbo, st); fetch(out->nodes, (const pga_topo_node_t*)d_onodes.p, nn, st);
	fetch(out->members, (const pga_rc_member_t*)d_omembers.p, nmo, st); fetch((long long*)out->origin, (const long long*)d_origin.p, nmo, st);
	fetch(out->who, (const pga_detach_member_t*)d_owho.p, nmo, st); fetch(out->block_map, (const uint32_t*)d_map.p, nb, st);
	fetch(out->orphans, (const pga_detach_orphan_t*)d_oorph.p, no, st); fetch(rec.data(), (const ClBlock*)d_rec.p, nbo, st);
	fetch(out->subs, (const pga_sub_t*)d_osubs.p, ns_out, st); fetch(out->dels, (const pga_del_t*)d_odels.p, nd_out, st);
	fetch(out->inss, (const pga_ins_t*)d_oinss.p, ni_out, st); fetch(out->ins_seq, (const char*)d_oseq.p, nl_out, st);
	clock.at(3);
	PGA_HIP(sync_stream(st));
	clock.read(g_cl_ms);
	out->n_subs = ns_out; out->n_dels = nd_out; out->n_inss = ni_out; out->n_ins_letters = nl_out;
	// ---- the consensus of every block after: a pointer that stays, or letters this call owns (every sequence at a multiple of 16) ----
	const bool copy_all = (flags & PGA_CLOSE_COPY_CONSENSUS) != 0;
	std::vector<const char*> src(nbo, nullptr); std::vector<uint64_t> at(nbo, ~0ULL);
	uint64_t n_cons = 0;
	for (uint64_t i = 0; i < nbo; ++i) {
		const ClBlock &R = rec[i];
		bool own = copy_all;
		if (R.kind == CL_K_SURVIVOR) src[i] = rc_blocks[R.src].consensus;
		else if (R.kind == CL_K_UPDATED) {
			const pga_rc_block_res_t &B = rc->blocks[R.src];
			if (B.kind == 0) src[i] = rc_blocks[upd[R.src]].consensus; else { src[i] = rc->cons ? rc->cons + B.cons_off : nullptr; own = true; }
		} else if (R.kind == CL_K_SINGLETON) { src[i] = R.src < C.n_o1 ? detached->blocks[nu + R.src].consensus : redetached->blocks[nu + (R.src - C.n_o1)].consensus; own = true; }
		else cl_fail("internal: a block after was left unwritten");
		if (out->blocks[i].cons_len && !src[i]) cl_fail("null consensus of a block with letters (block " + std::to_string(i) + " after)");
		if (own) { at[i] = n_cons; n_cons += ((uint64_t)out->blocks[i].cons_len + 15) / 16 * 16; }
	}
	out->cons = host_array<char>(n_cons + 1, me); out->n_cons_letters = n_cons;
	thread_ranges(nbo, range_threads(), [&](int, uint64_t i0, uint64_t i1) {
		for (uint64_t i = i0; i < i1; ++i) {
			const uint32_t len = out->blocks[i].cons_len;
			if (at[i] != ~0ULL && len) memcpy(out->cons + at[i], src[i], len);
			out->rc_blocks[i] = pga_rc_block_t{at[i] != ~0ULL ? out->cons + at[i] : src[i], len, out->blocks[i].depth};
		}
	});
}

} // namespace pga
