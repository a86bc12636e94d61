// pga_assemble.hip -- the block arrays behind a merge round: what pga_apply_merge's gather list (new_blocks[], member_src[]) stands for,
// executed.  solve_promise's tail (reweave.rs:88-93: alignment_insert of every re-aligned member into its anchor block), the insertion of
// the merged blocks (graph_merging.rs:156-165) and the blocks split_block leaves (reweave.rs:359-401), for the whole graph after in one call.
// The reference inserts member after member into a BTreeMap per block; here an output MEMBER, a LIST ELEMENT and a LETTER are the units of work.
//   host               validation (all of it before anything is launched), one record per output block, the consensus pointers; one upload
//   k_ts_sums / _scan / _offsets (pga_tile_scan.h), before   three exclusive sums over the members before: where a survivor's lists start
//   k_assemble_desc    one thread per output member: its source, its counts, its first elements there; member_src, res[].status and the
//                      offsets of the records are checked here
//   k_assemble_who / _who_check   one thread per node after, one per slot: who[], every slot named exactly once
//   k_ts_sums / _scan / _offsets, out      three exclusive sums over the descriptors: where the lists start in the output
//   host               the first wait: the checks, the three list totals
//   k_assemble_copy<list>   one thread per element of an output list (never one thread per member: a member has no edit or 10^4)
//   k_ts_sums / _scan / _offsets, letters  the lengths of the output insertions
//   host               the second wait: the bounds of every insertion (checked by the copy), the letter total
//   k_assemble_letters one thread per letter; k_assemble_seq_off
//   host               the third wait: the output
// The call waits for the device three times (a fourth time only to word the message of a failed promise result).
// The kernels and the host tables are pga_assemble_idx.h (no wave intrinsic: tests/emu/assemble_emu.cpp runs them on the host).
// All arithmetic is integer; atomics feed only marks and minima, so the result does not depend on the launch geometry.
#include "pga_common.h"
#include "pga_graph_host.h"
#include "../../include/pga_align.h"
#include "pga_assemble_idx.h"

namespace pga {

static unsigned as_grid(uint64_t items) { return grid_for(items, AS_THREADS, 2048); }
static unsigned as_tile_grid(uint64_t items) { return grid_for(items, AS_TILE, 1u << 16); }

// the stream's clock at four places of the last call of this thread: upload, kernels (their waits included), download, in ms
static thread_local double g_as_ms[3] = {0, 0, 0};
void assemble_last_ms(double *ms) { for (int i = 0; i < 3; ++i) ms[i] = g_as_ms[i]; }

void assemble_blocks_host(int64_t n_blocks, const pga_rc_block_t *rc_blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels,
                          const pga_ins_t *inss, const char *ins_seq, uint64_t ins_seq_len, int64_t n_cut, const pga_apply_cut_t *cut, const pga_plan_interval_t *intervals,
                          int64_t n_promises, const pga_plan_promise_t *promises, const pga_slice_out_t *slice, const pga_mapvar_res_t *res, const pga_sub_t *p_subs,
                          const pga_del_t *p_dels, const pga_ins_t *p_inss, const char *p_ins_seq, uint64_t p_ins_seq_len, const pga_apply_out_t *applied, uint32_t flags,
                          pga_assemble_out_t *out)
{
	AsTables A;
	as_validate(n_blocks, rc_blocks, members, subs, dels, inss, n_cut, cut, intervals, n_promises, promises, slice, res, p_subs, p_dels, p_inss, applied, flags, A);
	if (!ins_seq) ins_seq_len = 0;                                            // (a NULL buffer holds no letter: an insertion with letters is refused by its range)
	if (!p_ins_seq || A.identity) p_ins_seq_len = 0;
	const bool merged_only = (flags & PGA_ASSEMBLE_MERGED_ONLY) != 0;                  // no survivor in the output: the members and lists before stay on the host
	const uint64_t nbo = A.blocks.size(), nmo = A.n_out_members, nmb = merged_only ? 0 : A.n_before_members, ni = A.n_intervals, nk = A.n_slice_members, nr = A.n_res, nba = A.n_after_blocks;
	const uint64_t nbs = merged_only ? 0 : A.before_tot[0], nbd = merged_only ? 0 : A.before_tot[1], nbi = merged_only ? 0 : A.before_tot[2];
	const uint64_t nn = A.identity ? 0 : (uint64_t)applied->n_nodes;
	const bool who = !A.identity;
	out->n_blocks = (int64_t)nbo; out->n_members = (int64_t)nmo;
	out->blocks = host_array<pga_rc_block_t>(nbo, "pga_assemble_blocks");
	std::copy(A.o_blocks.begin(), A.o_blocks.end(), out->blocks);
	out->members = host_array<pga_rc_member_t>(nmo, "pga_assemble_blocks"); out->origin = host_array<int64_t>(nmo, "pga_assemble_blocks");
	if (who) out->who = host_array<pga_detach_member_t>(nmo, "pga_assemble_blocks");
	if (nmo == 0) {                                                           // no member after: nothing to gather, no slot to hold a node against, no device call
		out->subs = host_array<pga_sub_t>(0, "pga_assemble_blocks"); out->dels = host_array<pga_del_t>(0, "pga_assemble_blocks"); out->inss = host_array<pga_ins_t>(0, "pga_assemble_blocks"); out->ins_seq = host_array<char>(0, "pga_assemble_blocks");
		return;
	}
	StreamLease stream;
	hipStream_t st = stream.s;
	StageClock clock(st);
	clock.at(0);
	// ---- the uploads (every buffer one entry longer than its count: none is empty) ----
	DBuf<AsBlock> d_blocks(nbo + 1); DBuf<as_u64> d_first(nbo + 1), d_afirst(nba + 1), d_err(AS_ERRS); DBuf<uint32_t> d_adepth(nba + 1), d_used(nk + 1), d_slotcnt(nmo + 1);
	DBuf<pga_rc_member_t> d_members(nmb + 1), d_omembers(nmo + 1); DBuf<pga_sub_t> d_subs(nbs + 1), d_ssubs(A.slice_tot[0] + 1), d_psubs(A.p_tot[0] + 1);
	DBuf<pga_del_t> d_dels(nbd + 1), d_sdels(A.slice_tot[1] + 1), d_pdels(A.p_tot[1] + 1);
	DBuf<pga_ins_t> d_inss(nbi + 1), d_sinss(A.slice_tot[2] + 1), d_pinss(A.p_tot[2] + 1);
	DBuf<pga_slice_res_t> d_slices(ni + 1); DBuf<pga_slice_member_t> d_smembers(nk + 1); DBuf<pga_mapvar_res_t> d_res(nr + 1); DBuf<uint64_t> d_msrc(nk + 1);
	DBuf<char> d_letters(ins_seq_len + p_ins_seq_len + 1); DBuf<pga_topo_node_t> d_nodes(nn + 1);
	DBuf<AsDesc> d_desc(nmo + 1); DBuf<long long> d_origin(nmo + 1); DBuf<pga_detach_member_t> d_who(nmo + 1);
	upload(d_blocks, A.blocks.data(), nbo, st); upload(d_first, (const as_u64*)A.blk_first.data(), nbo + 1, st);
	upload(d_members, members, nmb, st); upload(d_subs, subs, nbs, st); upload(d_dels, dels, nbd, st); upload(d_inss, inss, nbi, st);
	if (ins_seq_len) PGA_HIP(hipMemcpyAsync(d_letters.p, ins_seq, ins_seq_len, hipMemcpyHostToDevice, st));
	if (!A.identity) {
		upload(d_afirst, (const as_u64*)A.after_first.data(), nba, st); upload(d_adepth, A.after_depth.data(), nba, st);
		upload(d_slices, slice->slices, ni, st); upload(d_smembers, slice->members, nk, st); upload(d_msrc, applied->member_src, nk, st);
		upload(d_ssubs, slice->subs, A.slice_tot[0], st); upload(d_sdels, slice->dels, A.slice_tot[1], st); upload(d_sinss, slice->inss, A.slice_tot[2], st);
		upload(d_res, res, nr, st); upload(d_psubs, p_subs, A.p_tot[0], st); upload(d_pdels, p_dels, A.p_tot[1], st); upload(d_pinss, p_inss, A.p_tot[2], st);
		if (p_ins_seq_len) PGA_HIP(hipMemcpyAsync(d_letters.p + ins_seq_len, p_ins_seq, p_ins_seq_len, hipMemcpyHostToDevice, st));
		upload(d_nodes, applied->nodes, nn, st);
	}
	clock.at(1);
	// ---- the descriptors, who, the two member scans ----
	d_used.zero(st); d_slotcnt.zero(st);
	PGA_HIP(hipMemsetAsync(d_err.p, 0xff, AS_ERRS * sizeof(as_u64), st));
	TileScanBufs<as_u64> b_before, b_out, b_let;
	AsDev V;
	memset(&V, 0, sizeof(V));
	V.n_out_blocks = nbo; V.n_out_members = nmo; V.n_before_members = nmb; V.n_nodes = nn; V.n_after_blocks = nba; V.ins_seq_len = ins_seq_len; V.p_ins_seq_len = p_ins_seq_len;
	for (int q = 0; q < 3; ++q) { V.slice_tot[q] = A.slice_tot[q]; V.p_tot[q] = A.p_tot[q]; }
	V.blocks = d_blocks.p; V.blk_first = d_first.p; V.members = d_members.p; V.subs = d_subs.p; V.dels = d_dels.p; V.inss = d_inss.p;
	V.slices = d_slices.p; V.s_members = d_smembers.p; V.s_subs = d_ssubs.p; V.s_dels = d_sdels.p; V.s_inss = d_sinss.p;
	V.res = d_res.p; V.p_subs = d_psubs.p; V.p_dels = d_pdels.p; V.p_inss = d_pinss.p; V.letters = d_letters.p; V.member_src = d_msrc.p; V.used = d_used.p;
	V.desc = d_desc.p; V.o_members = d_omembers.p; V.origin = d_origin.p;
	V.nodes = d_nodes.p; V.after_first = d_afirst.p; V.after_depth = d_adepth.p; V.who = d_who.p; V.slot_cnt = d_slotcnt.p; V.err = d_err.p;
	V.scan[AS_SCAN_BEFORE] = b_before.make(nmb, 3); V.scan[AS_SCAN_OUT] = b_out.make(nmo, 3);
	tile_scan_launch(V.scan[AS_SCAN_BEFORE], AsBeforeValue{V}, st);
	hipLaunchKernelGGL(k_assemble_desc, dim3(as_grid(nmo)), dim3(AS_THREADS), 0, st, V);
	if (who) {
		hipLaunchKernelGGL(k_assemble_who, dim3(as_grid(nn)), dim3(AS_THREADS), 0, st, V);
		hipLaunchKernelGGL(k_assemble_who_check, dim3(as_grid(nmo)), dim3(AS_THREADS), 0, st, V);
	}
	tile_scan_launch(V.scan[AS_SCAN_OUT], AsOutValue{V}, st);
	PGA_HIP(hipGetLastError());
	// ---- the first wait: nothing behind it runs on input that was not checked ----
	as_u64 err[AS_ERRS], tot[3];
	fetch(err, (const as_u64*)d_err.p, AS_ERRS, st);
	for (int q = 0; q < 3; ++q) fetch(&tot[q], ts_off(V.scan[AS_SCAN_OUT], q) + nmo, 1, st);
	PGA_HIP(sync_stream(st));
	as_u64 status_k = 0;
	if (err[AS_E_STATUS] != AS_NONE) {                                        // (the failing path only: which slice member it was)
		long long o = 0;
		fetch(&o, (const long long*)d_origin.p + err[AS_E_STATUS], 1, st);
		PGA_HIP(sync_stream(st));
		status_k = (as_u64)(-(o + 1));
	}
	as_report(err, A, status_k, A.identity ? nullptr : slice->slices);
	const uint64_t ns_out = tot[0], nd_out = tot[1], ni_out = tot[2];
	if (ns_out > nbs + A.slice_tot[0] + A.p_tot[0] || nd_out > nbd + A.slice_tot[1] + A.p_tot[1] || ni_out > nbi + A.slice_tot[2] + A.p_tot[2])
		as_fail("internal: the device and the host disagree on the list totals");
	// ---- the three lists, the letter scan ----
	DBuf<pga_sub_t> d_osubs(ns_out + 1); DBuf<pga_del_t> d_odels(nd_out + 1); DBuf<pga_ins_t> d_oinss(ni_out + 1);
	V.o_subs = d_osubs.p; V.o_dels = d_odels.p; V.o_inss = d_oinss.p;
	if (ns_out) hipLaunchKernelGGL(k_assemble_copy<RM_LIST_SUB>, dim3(as_tile_grid(ns_out)), dim3(AS_THREADS), 0, st, V);
	if (nd_out) hipLaunchKernelGGL(k_assemble_copy<RM_LIST_DEL>, dim3(as_tile_grid(nd_out)), dim3(AS_THREADS), 0, st, V);
	if (ni_out) hipLaunchKernelGGL(k_assemble_copy<RM_LIST_INS>, dim3(as_tile_grid(ni_out)), dim3(AS_THREADS), 0, st, V);
	V.scan[AS_SCAN_LETTERS] = b_let.make(ni_out, 1);
	tile_scan_launch(V.scan[AS_SCAN_LETTERS], AsLetterValue{V}, st);
	PGA_HIP(hipGetLastError());
	// ---- the second wait: every insertion lies inside its buffer before a letter is read ----
	as_u64 n_let = 0;
	fetch(err, (const as_u64*)d_err.p, AS_ERRS, st); fetch(&n_let, ts_off(V.scan[AS_SCAN_LETTERS], 0) + ni_out, 1, st);
	PGA_HIP(sync_stream(st));
	as_report_letters(err);
	const uint64_t nl_out = n_let;
	DBuf<char> d_oseq(nl_out + 1);
	V.o_ins_seq = d_oseq.p;
	if (nl_out) hipLaunchKernelGGL(k_assemble_letters, dim3(as_tile_grid(nl_out)), dim3(AS_THREADS), 0, st, V);
	if (ni_out) hipLaunchKernelGGL(k_assemble_seq_off, dim3(as_grid(ni_out)), dim3(AS_THREADS), 0, st, V);
	PGA_HIP(hipGetLastError());
	clock.at(2);
	// ---- the output ----
	out->subs = host_array<pga_sub_t>(ns_out, "pga_assemble_blocks"); out->dels = host_array<pga_del_t>(nd_out, "pga_assemble_blocks"); out->inss = host_array<pga_ins_t>(ni_out, "pga_assemble_blocks");
	out->ins_seq = host_array<char>(nl_out + 1, "pga_assemble_blocks");
	fetch(out->members, (const pga_rc_member_t*)d_omembers.p, nmo, st); fetch((long long*)out->origin, (const long long*)d_origin.p, nmo, st);
	if (who) fetch(out->who, (const pga_detach_member_t*)d_who.p, nmo, st);
	fetch(out->subs, (const pga_sub_t*)d_osubs.p, ns_out, st); fetch(out->dels, (const pga_del_t*)d_odels.p, nd_out, st);
	fetch(out->inss, (const pga_ins_t*)d_oinss.p, ni_out, st); fetch(out->ins_seq, (const char*)d_oseq.p, nl_out, st);
	clock.at(3);
	PGA_HIP(sync_stream(st));
	clock.read(g_as_ms);
	out->n_subs = ns_out; out->n_dels = nd_out; out->n_inss = ni_out; out->n_ins_letters = nl_out;
}

} // namespace pga
