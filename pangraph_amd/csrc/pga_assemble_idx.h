// pga_assemble_idx.h -- the kernels and host tables of pga_assemble.hip (the block arrays behind a merge round: solve_promise's tail,
// reweave.rs:88-93 alignment_insert; the insertion of the merged blocks, graph_merging.rs:156-165; the blocks split_block leaves,
// reweave.rs:359-401).  No wave intrinsic, atomicAdd / atomicMin only: all of this compiles under hipcc and, with dev/emu/hip_emu.h
// included first, under g++ -std=c++17 -DPGA_EMU (tests/emu/assemble_emu.cpp runs it against a direct scalar construction).
// The scans are the tile scan of pga_tile_scan.h (k_ts_sums / _scan / _offsets, ts_last_le) with the value functors below.
//
// A MEMBER is a member of the output, m.  Its DESCRIPTOR says where its three lists come from: the SOURCE (the caller's arrays of the graph
// before, the sliced lists, the promise results), the three counts and the three first elements there.  A survivor's first elements are the
// exclusive sums over the members before (the BEFORE scan, three quantities), a slice member's and a promise result's are written in their
// records.  The OUT scan (three quantities over the descriptors) says where the lists of a member start in the output; the LETTER scan (one
// quantity over the output insertions) gives the new seq_off.
// A LIST COPY is spread over the elements of the OUTPUT list in tiles of AS_TILE: the members of a tile's first and last element are looked up
// once per workgroup, every thread then finds the member of its element between the two, so one member with thousands of edits beside
// thousands without does not serialise.  The letter gather is spread over the bytes of the output in the same way.
// The two letter buffers lie behind each other on the device (the caller's, then the promises'): a copied insertion of a promise result has
// its seq_off moved up by ins_seq_len until the gather has read it.
#pragma once
#include "pga_remove_idx.h"

namespace pga {

typedef rm_u64 as_u64;
constexpr int AS_THREADS = TS_THREADS, AS_TILE = TS_TILE;
static_assert(AS_TILE == PGA_ASSEMBLE_TILE, "the header exports the tile of the scans");
enum { AS_SCAN_BEFORE = 0, AS_SCAN_OUT = 1, AS_SCAN_LETTERS = 2, AS_SCANS = 3 };
enum { AS_SRC_BEFORE = 0, AS_SRC_SLICE = 1, AS_SRC_PROMISE = 2 };
enum { AS_K_SURVIVOR = 0, AS_K_UNALIGNED = 1, AS_K_MERGED = 2 };
// err[]: the lowest offender (output member; output member; output member; output member; output insertion; node; slot; node), all-ones = none
enum { AS_E_SRC_RANGE = 0, AS_E_SRC_TWICE = 1, AS_E_STATUS = 2, AS_E_LIST_RANGE = 3, AS_E_SEQ_RANGE = 4, AS_E_SLOT_TWICE = 5, AS_E_SLOT_EMPTY = 6, AS_E_SLOT_RANGE = 7, AS_ERRS = 8 };
constexpr as_u64 AS_NONE = ~0ULL;

// one block of the output.  src: a survivor's first member before; otherwise its member_off in member_src[]
struct AsBlock { as_u64 src, first_res; uint32_t kind, ia, ib, promise; };
struct AsDesc { as_u64 off[3]; uint32_t n[3], src; };
struct AsDev {
	uint64_t n_out_blocks, n_out_members, n_before_members, n_nodes, n_after_blocks, ins_seq_len, p_ins_seq_len;
	uint64_t slice_tot[3], p_tot[3];                        // the lengths of the sliced lists and of the promise results' lists
	const AsBlock *blocks; const as_u64 *blk_first;        // per output block; blk_first: n_out_blocks + 1 entries, the last one n_out_members
	const pga_rc_member_t *members; const pga_sub_t *subs; const pga_del_t *dels; const pga_ins_t *inss;         // the graph before
	const pga_slice_res_t *slices; const pga_slice_member_t *s_members; const pga_sub_t *s_subs; const pga_del_t *s_dels; const pga_ins_t *s_inss;
	const pga_mapvar_res_t *res; const pga_sub_t *p_subs; const pga_del_t *p_dels; const pga_ins_t *p_inss;
	const char *letters;                                   // ins_seq_len letters of the caller, then p_ins_seq_len of the promises
	const uint64_t *member_src;
	uint32_t *used;                                        // per slice member (zeroed before)
	AsDesc *desc; pga_rc_member_t *o_members; long long *origin;   // per output member
	RmScan scan[AS_SCANS];
	pga_sub_t *o_subs; pga_del_t *o_dels; pga_ins_t *o_inss; char *o_ins_seq;
	// who
	const pga_topo_node_t *nodes; const as_u64 *after_first; const uint32_t *after_depth;   // per block after: its first output member or AS_NONE; its depth
	pga_detach_member_t *who; uint32_t *slot_cnt;          // per output member (slot_cnt zeroed before)
	as_u64 *err;                                           // AS_ERRS words
};

// what a member before, a descriptor and an output insertion are worth in their scans
struct AsBeforeValue {
	AsDev V;
	__host__ __device__ as_u64 operator()(int q, uint64_t i) const
	{
		const pga_rc_member_t M = V.members[i];
		return q == RM_LIST_SUB ? M.n_subs : q == RM_LIST_DEL ? M.n_dels : M.n_inss;
	}
};
struct AsOutValue { AsDev V; __host__ __device__ as_u64 operator()(int q, uint64_t i) const { return V.desc[i].n[q]; } };
struct AsLetterValue { AsDev V; __host__ __device__ as_u64 operator()(int, uint64_t i) const { return V.o_inss[i].len; } };
// off + n <= tot, without wrapping
__host__ __device__ inline bool as_inside(as_u64 off, as_u64 n, as_u64 tot) { return off <= tot && n <= tot - off; }

// ---------------------------------------------------------------- 1. the scans: pga_tile_scan.h (64 bits, two levels)

// ---------------------------------------------------------------- 2. behind the BEFORE scan: one thread per output member, its descriptor
// A descriptor that fails a check keeps three empty lists: nothing behind it reads through a value that was refused.
static __global__ __launch_bounds__(AS_THREADS) void k_assemble_desc(AsDev V)
{
	const RmScan S = V.scan[AS_SCAN_BEFORE];
	for (as_u64 m = (as_u64)blockIdx.x * AS_THREADS + threadIdx.x; m < V.n_out_members; m += (as_u64)gridDim.x * AS_THREADS) {
		const as_u64 b = ts_last_le(V.blk_first, 0, V.n_out_blocks, m), s = m - V.blk_first[b];
		const AsBlock B = V.blocks[b];
		AsDesc D = {{0, 0, 0}, {0, 0, 0}, AS_SRC_BEFORE};
		long long origin = 0;
		if (B.kind == AS_K_SURVIVOR) {
			const as_u64 g = B.src + s;                                            // (below n_before_members: the host held n_members against the depth after)
			const pga_rc_member_t M = V.members[g];
			D.n[0] = M.n_subs; D.n[1] = M.n_dels; D.n[2] = M.n_inss;
			for (int q = 0; q < 3; ++q) D.off[q] = ts_off(S, q)[g];
			origin = (long long)g;
		} else {
			const as_u64 k = V.member_src[B.src + s];
			const pga_slice_res_t A = V.slices[B.ia], Q = V.slices[B.ib];
			const bool anchor = k >= A.member_off && k - A.member_off < A.n_kept;
			const bool append = !anchor && B.kind == AS_K_MERGED && k >= Q.member_off && k - Q.member_off < Q.n_kept;
			if (!anchor && !append) atomicMin(&V.err[AS_E_SRC_RANGE], m);
			else {
				origin = -(1LL + (long long)k);                                     // (k lies inside a slice, so below 2^31)
				if (atomicAdd(&V.used[k], 1u) != 0u) atomicMin(&V.err[AS_E_SRC_TWICE], m);
				else if (anchor) {
					const pga_slice_member_t X = V.s_members[k];
					if (!as_inside(X.sub_off, X.counts.n_subs, V.slice_tot[0]) || !as_inside(X.del_off, X.counts.n_dels, V.slice_tot[1]) || !as_inside(X.ins_off, X.counts.n_inss, V.slice_tot[2]))
						atomicMin(&V.err[AS_E_LIST_RANGE], m);
					else { D = AsDesc{{X.sub_off, X.del_off, X.ins_off}, {X.counts.n_subs, X.counts.n_dels, X.counts.n_inss}, AS_SRC_SLICE}; }
				} else {
					const pga_mapvar_res_t R = V.res[B.first_res + (k - Q.member_off)];
					if (R.status != 0) atomicMin(&V.err[AS_E_STATUS], m);
					else if (!as_inside(R.sub_off, R.n_subs, V.p_tot[0]) || !as_inside(R.del_off, R.n_dels, V.p_tot[1]) || !as_inside(R.ins_off, R.n_inss, V.p_tot[2]))
						atomicMin(&V.err[AS_E_LIST_RANGE], m);
					else { D = AsDesc{{R.sub_off, R.del_off, R.ins_off}, {R.n_subs, R.n_dels, R.n_inss}, AS_SRC_PROMISE}; }
				}
			}
		}
		V.desc[m] = D; V.origin[m] = origin;
		V.o_members[m] = pga_rc_member_t{D.n[0], D.n[1], D.n[2]};
	}
}

// ---------------------------------------------------------------- 3. who: one thread per node of the graph after, then one per slot
static __global__ __launch_bounds__(AS_THREADS) void k_assemble_who(AsDev V)
{
	for (as_u64 i = (as_u64)blockIdx.x * AS_THREADS + threadIdx.x; i < V.n_nodes; i += (as_u64)gridDim.x * AS_THREADS) {
		const pga_topo_node_t A = V.nodes[i];
		if (A.block >= V.n_after_blocks || A.member >= V.after_depth[A.block]) { atomicMin(&V.err[AS_E_SLOT_RANGE], i); continue; }
		const as_u64 first = V.after_first[A.block];
		if (first == AS_NONE) continue;                                             // (merged-only: a block that is not in the output)
		if (atomicAdd(&V.slot_cnt[first + A.member], 1u) != 0u) atomicMin(&V.err[AS_E_SLOT_TWICE], i);
		else V.who[first + A.member] = pga_detach_member_t{A.node_id, A.reverse ? 1 : 0, 0};
	}
}
static __global__ __launch_bounds__(AS_THREADS) void k_assemble_who_check(AsDev V)
{
	for (as_u64 m = (as_u64)blockIdx.x * AS_THREADS + threadIdx.x; m < V.n_out_members; m += (as_u64)gridDim.x * AS_THREADS)
		if (V.slot_cnt[m] == 0u) atomicMin(&V.err[AS_E_SLOT_EMPTY], m);
}

// ---------------------------------------------------------------- 4. behind the checks: the three lists, one thread per element of the output
template <int LIST> __device__ inline void as_copy_one(const AsDev &V, as_u64 j, uint32_t src, as_u64 at);
template <> __device__ inline void as_copy_one<RM_LIST_SUB>(const AsDev &V, as_u64 j, uint32_t src, as_u64 at) { V.o_subs[j] = (src == AS_SRC_BEFORE ? V.subs : src == AS_SRC_SLICE ? V.s_subs : V.p_subs)[at]; }
template <> __device__ inline void as_copy_one<RM_LIST_DEL>(const AsDev &V, as_u64 j, uint32_t src, as_u64 at) { V.o_dels[j] = (src == AS_SRC_BEFORE ? V.dels : src == AS_SRC_SLICE ? V.s_dels : V.p_dels)[at]; }
template <> __device__ inline void as_copy_one<RM_LIST_INS>(const AsDev &V, as_u64 j, uint32_t src, as_u64 at)
{
	pga_ins_t I = (src == AS_SRC_BEFORE ? V.inss : src == AS_SRC_SLICE ? V.s_inss : V.p_inss)[at];
	const bool p = src == AS_SRC_PROMISE;
	if (I.len && !as_inside(I.seq_off, I.len, p ? V.p_ins_seq_len : V.ins_seq_len)) atomicMin(&V.err[AS_E_SEQ_RANGE], j);   // (the letters are read only behind this check)
	else if (p) I.seq_off += V.ins_seq_len;
	V.o_inss[j] = I;
}
template <int LIST> static __global__ __launch_bounds__(AS_THREADS) void k_assemble_copy(AsDev V)
{
	__shared__ as_u64 s_rng[2];
	const RmScan S = V.scan[AS_SCAN_OUT];
	const as_u64 *out = ts_off(S, LIST);
	const as_u64 n = out[S.n], n_tiles = (n + AS_TILE - 1) / AS_TILE;
	for (as_u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const as_u64 j0 = t * AS_TILE, j1 = j0 + AS_TILE < n ? j0 + AS_TILE : n;
		if (threadIdx.x < 2) s_rng[threadIdx.x] = ts_last_le(out, 0, S.n, threadIdx.x ? j1 - 1 : j0);
		__syncthreads();
		const as_u64 lo = s_rng[0], hi = s_rng[1] + 1;
		for (as_u64 j = j0 + threadIdx.x; j < j1; j += AS_THREADS) {
			const as_u64 m = ts_last_le(out, lo, hi, j);
			as_copy_one<LIST>(V, j, V.desc[m].src, V.desc[m].off[LIST] + (j - out[m]));
		}
		__syncthreads();
	}
}

// ---------------------------------------------------------------- 5. behind the letter scan and the checks of as_copy_one: one thread per letter
static __global__ __launch_bounds__(AS_THREADS) void k_assemble_letters(AsDev V)
{
	__shared__ as_u64 s_rng[2];
	const RmScan S = V.scan[AS_SCAN_LETTERS];
	const as_u64 *out = ts_off(S, 0);
	const as_u64 n = out[S.n], n_tiles = (n + AS_TILE - 1) / AS_TILE;
	for (as_u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const as_u64 j0 = t * AS_TILE, j1 = j0 + AS_TILE < n ? j0 + AS_TILE : n;
		if (threadIdx.x < 2) s_rng[threadIdx.x] = ts_last_le(out, 0, S.n, threadIdx.x ? j1 - 1 : j0);
		__syncthreads();
		const as_u64 lo = s_rng[0], hi = s_rng[1] + 1;
		for (as_u64 j = j0 + threadIdx.x; j < j1; j += AS_THREADS) {
			const as_u64 k = ts_last_le(out, lo, hi, j);
			V.o_ins_seq[j] = V.letters[V.o_inss[k].seq_off + (j - out[k])];
		}
		__syncthreads();
	}
}
// behind the gather: seq_off becomes the running sum of len
static __global__ __launch_bounds__(AS_THREADS) void k_assemble_seq_off(AsDev V)
{
	const RmScan S = V.scan[AS_SCAN_LETTERS];
	const as_u64 *out = ts_off(S, 0);
	for (as_u64 k = (as_u64)blockIdx.x * AS_THREADS + threadIdx.x; k < S.n; k += (as_u64)gridDim.x * AS_THREADS) V.o_inss[k].seq_off = out[k];
}

// ---------------------------------------------------------------- host side: everything that is refused before a launch, and the tables
struct AsTables {
	std::vector<AsBlock> blocks; std::vector<as_u64> blk_first;           // per output block (blk_first: one more)
	std::vector<as_u64> after_first; std::vector<uint32_t> after_depth;   // per block after
	std::vector<pga_rc_block_t> o_blocks;
	uint64_t n_intervals = 0, n_slice_members = 0, n_res = 0, n_before_members = 0, n_out_members = 0, n_after_blocks = 0;
	uint64_t before_tot[3] = {0, 0, 0}, slice_tot[3] = {0, 0, 0}, p_tot[3] = {0, 0, 0};
	bool identity = false;                                                // n_cut == 0: every block as it is, no who
};
inline void as_fail(const std::string &what) { throw std::runtime_error("pga_assemble_blocks: " + what); }

static void as_validate(int64_t n_blocks, const pga_rc_block_t *rc_blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss,
                        int64_t n_cut, const pga_apply_cut_t *cut, const pga_plan_interval_t *intervals, int64_t n_promises, const pga_plan_promise_t *promises,
                        const pga_slice_out_t *slice, const pga_mapvar_res_t *res, const pga_sub_t *p_subs, const pga_del_t *p_dels, const pga_ins_t *p_inss,
                        const pga_apply_out_t *applied, uint32_t flags, AsTables &A)
{
	const char *null = "null argument or negative count";
	const uint64_t lim = 1ULL << 63, lim31 = 1ULL << 31;
	if (flags & ~PGA_ASSEMBLE_MERGED_ONLY) as_fail("unknown flag");
	if (n_blocks < 0 || n_cut < 0 || n_promises < 0 || (n_blocks && !rc_blocks)) as_fail(null);
	if ((uint64_t)n_blocks >= lim31 || (uint64_t)n_cut >= lim31 || (uint64_t)n_promises >= lim31) as_fail("2^31 or more blocks, cut blocks or promises");
	const bool merged_only = (flags & PGA_ASSEMBLE_MERGED_ONLY) != 0;
	// ---- the graph before
	std::vector<uint64_t> first_before((size_t)n_blocks + 1, 0);
	for (int64_t b = 0; b < n_blocks; ++b) first_before[b + 1] = first_before[b] + rc_blocks[b].n_members;
	A.n_before_members = first_before[n_blocks];
	if (A.n_before_members >= lim31) as_fail("2^31 or more members");
	if (A.n_before_members && !members) as_fail(null);
	// the list totals of the graph before size its upload; merged-only takes no survivor, so it neither walks nor uploads them
	for (uint64_t m = 0; m < (merged_only ? 0 : A.n_before_members); ++m) {
		A.before_tot[0] += members[m].n_subs; A.before_tot[1] += members[m].n_dels; A.before_tot[2] += members[m].n_inss;
		if (A.before_tot[0] >= lim || A.before_tot[1] >= lim || A.before_tot[2] >= lim) as_fail("the edit counts overflow 2^63");
	}
	if ((A.before_tot[0] && !subs) || (A.before_tot[1] && !dels) || (A.before_tot[2] && !inss)) as_fail(null);
	auto emit = [&](const AsBlock &B, const pga_rc_block_t &R) {
		A.blk_first.push_back(A.n_out_members); A.blocks.push_back(B); A.o_blocks.push_back(R);
		A.n_out_members += R.n_members;
		if (A.n_out_members >= lim31) as_fail("2^31 or more members after");
	};
	if (n_cut == 0) {
		A.identity = true;
		if (!merged_only) for (int64_t b = 0; b < n_blocks; ++b) emit(AsBlock{first_before[b], 0, AS_K_SURVIVOR, 0, 0, 0}, rc_blocks[b]);
		A.blk_first.push_back(A.n_out_members);
		return;
	}
	// ---- the cut, the intervals, the slices: as pga_apply_merge holds them against each other.  These refusals are ap_validate's
	// (pga_apply_idx.h), message for message; that function also needs the flat graph, which this entry does not take, so they are
	// restated here: a change to one of the two belongs in the other as well.
	if (!cut || !intervals || !slice || !slice->slices || !applied || !applied->blocks || !applied->block_map) as_fail(null);
	std::vector<uint32_t> cut_of((size_t)n_blocks, TP_NONE), iv_cut;
	for (int64_t c = 0; c < n_cut; ++c) {
		const pga_apply_cut_t &C = cut[c];
		const std::string who = " (cut " + std::to_string(c) + ")";
		if (C.block >= (uint64_t)n_blocks) as_fail("a cut block is out of range" + who);
		if (cut_of[C.block] != TP_NONE) as_fail("a cut block is named twice" + who);
		if (C.n_intervals == 0) as_fail("a cut block without intervals" + who);
		if (C.first_interval != A.n_intervals) as_fail("first_interval is not the running sum of n_intervals" + who);
		cut_of[C.block] = (uint32_t)c;
		A.n_intervals += C.n_intervals;
		if (A.n_intervals >= lim31) as_fail("2^31 or more intervals");
		iv_cut.insert(iv_cut.end(), C.n_intervals, (uint32_t)c);
	}
	const pga_slice_res_t *slices = slice->slices;
	for (int64_t c = 0; c < n_cut; ++c) for (uint32_t j = 0; j < cut[c].n_intervals; ++j) {
		const uint64_t s = cut[c].first_interval + j;
		const pga_plan_interval_t &I = intervals[s];
		const std::string who = " (cut " + std::to_string(c) + ", interval " + std::to_string(j) + ")";
		if (I.start >= I.end || (j && I.start < intervals[s - 1].end)) as_fail("the intervals of a block are not ascending and disjoint" + who);
		if (I.end > rc_blocks[cut[c].block].cons_len) as_fail("an interval lies beyond its block's consensus" + who);
		if (slices[s].member_off != A.n_slice_members || slices[s].n_kept > rc_blocks[cut[c].block].n_members) as_fail("the n_kept of the slices do not match members[]" + who);
		A.n_slice_members += slices[s].n_kept;
		if (A.n_slice_members >= lim31) as_fail("2^31 or more slice members");
	}
	const uint64_t nk = A.n_slice_members;
	if (nk && (!slice->members || !applied->member_src)) as_fail(null);
	if (nk) {
		const pga_slice_member_t &X = slice->members[nk - 1];
		A.slice_tot[0] = X.sub_off + X.counts.n_subs; A.slice_tot[1] = X.del_off + X.counts.n_dels; A.slice_tot[2] = X.ins_off + X.counts.n_inss;
		if (X.sub_off >= lim || X.del_off >= lim || X.ins_off >= lim || A.slice_tot[0] >= lim || A.slice_tot[1] >= lim || A.slice_tot[2] >= lim) as_fail("the edit counts overflow 2^63");
	}
	if ((A.slice_tot[0] && !slice->subs) || (A.slice_tot[1] && !slice->dels) || (A.slice_tot[2] && !slice->inss)) as_fail(null);
	// ---- the promises: each names an aligned pair; its results follow those of the promises before
	if (n_promises && !promises) as_fail(null);
	std::vector<int64_t> promise_of((size_t)A.n_intervals, -1);
	std::vector<uint64_t> first_res((size_t)n_promises + 1, 0);
	for (int64_t p = 0; p < n_promises; ++p) {
		const pga_plan_promise_t &P = promises[p];
		const std::string who = " (promise " + std::to_string(p) + ")";
		if (P.anchor_interval >= A.n_intervals || P.append_interval >= A.n_intervals) as_fail("a promise names an interval out of range" + who);
		const pga_plan_interval_t &Ia = intervals[P.anchor_interval], &Ib = intervals[P.append_interval];
		if (!Ia.aligned || !Ia.is_anchor || !Ib.aligned || Ib.is_anchor || Ia.new_block_id != Ib.new_block_id) as_fail("the intervals of a promise are not an anchor and its append" + who);
		if (promise_of[P.append_interval] >= 0) as_fail("two promises with one append_interval" + who);
		promise_of[P.append_interval] = p;
		first_res[p + 1] = first_res[p] + slices[P.append_interval].n_kept;
	}
	A.n_res = first_res[n_promises];
	if (A.n_res && !res) as_fail(null);
	if (A.n_res) {
		const pga_mapvar_res_t &R = res[A.n_res - 1];
		A.p_tot[0] = R.sub_off + R.n_subs; A.p_tot[1] = R.del_off + R.n_dels; A.p_tot[2] = R.ins_off + R.n_inss;
		if (R.sub_off >= lim || R.del_off >= lim || R.ins_off >= lim || A.p_tot[0] >= lim || A.p_tot[1] >= lim || A.p_tot[2] >= lim) as_fail("the edit counts overflow 2^63");
	}
	if ((A.p_tot[0] && !p_subs) || (A.p_tot[1] && !p_dels) || (A.p_tot[2] && !p_inss)) as_fail(null);
	// ---- the graph after: every block is a survivor or a new block, once
	if (applied->n_new_nodes != (int64_t)nk) as_fail("applied->n_new_nodes differs from the kept members of the slices");
	if (applied->n_blocks < 0 || applied->n_new_blocks < 0 || applied->n_nodes < 0 || (applied->n_new_blocks && !applied->new_blocks) || (applied->n_nodes && !applied->nodes)) as_fail(null);
	if ((uint64_t)applied->n_blocks >= lim31) as_fail("2^31 or more blocks after");
	A.n_after_blocks = (uint64_t)applied->n_blocks;
	const uint64_t nba = A.n_after_blocks;
	std::vector<AsBlock> after(nba, AsBlock{0, 0, TP_NONE, 0, 0, 0});
	std::vector<pga_rc_block_t> after_rc(nba);
	for (int64_t b = 0; b < n_blocks; ++b) {
		const uint32_t to = applied->block_map[b];
		const std::string who = " (block " + std::to_string(b) + ")";
		if (cut_of[b] != TP_NONE) { if (to != TP_NONE) as_fail("block_map keeps a cut block" + who); continue; }
		if (to == TP_NONE) { if (rc_blocks[b].n_members) as_fail("a block that is neither cut nor mapped has members" + who); continue; }
		if (to >= nba) as_fail("block_map is out of range" + who);
		if (after[to].kind != TP_NONE) as_fail("a block after is named twice" + who);
		if (rc_blocks[b].n_members != applied->blocks[to].depth) as_fail("n_members of a survivor differs from its depth after" + who);
		after[to] = AsBlock{first_before[b], 0, AS_K_SURVIVOR, 0, 0, 0};
		after_rc[to] = rc_blocks[b];
	}
	uint64_t member_off = 0, n_merged = 0;
	for (int64_t e = 0; e < applied->n_new_blocks; ++e) {
		const pga_apply_block_t &E = applied->new_blocks[e];
		const std::string who = " (new block " + std::to_string(e) + ")";
		if (E.block >= nba) as_fail("a new block is out of range" + who);
		if (after[E.block].kind != TP_NONE) as_fail("a block after is named twice" + who);
		if ((E.kind != 0 && E.kind != 1) || E.interval_a >= A.n_intervals || (E.kind && E.interval_b >= A.n_intervals)) as_fail("a new block names an interval out of range, or has an unknown kind" + who);
		const pga_plan_interval_t &Ia = intervals[E.interval_a];
		uint64_t depth = slices[E.interval_a].n_kept;
		int64_t p = 0;
		if (E.kind == 0) { if (Ia.aligned) as_fail("an unaligned block over an aligned interval" + who); }
		else {
			p = promise_of[E.interval_b];
			if (p < 0) as_fail("the interval_b of a merged block is no promise's append_interval" + who);
			if (promises[p].anchor_interval != E.interval_a) as_fail("a promise whose anchor_interval disagrees with new_blocks[] (promise " + std::to_string(p) + ")");
			depth += slices[E.interval_b].n_kept; ++n_merged;
		}
		if (E.member_off != member_off) as_fail("member_off of new_blocks[] is not the running sum of the depths" + who);
		if (applied->blocks[E.block].depth != depth) as_fail("the depth of a new block is not the kept members of its slices" + who);
		member_off += depth;
		const pga_rc_block_t &C = rc_blocks[cut[iv_cut[E.interval_a]].block];
		after[E.block] = AsBlock{E.member_off, E.kind ? first_res[p] : 0, E.kind ? (uint32_t)AS_K_MERGED : (uint32_t)AS_K_UNALIGNED, (uint32_t)E.interval_a, E.kind ? (uint32_t)E.interval_b : (uint32_t)E.interval_a, (uint32_t)p};
		after_rc[E.block] = pga_rc_block_t{C.consensus ? C.consensus + Ia.start : nullptr, Ia.end - Ia.start, (uint32_t)depth};
	}
	if (member_off != nk) as_fail("new_blocks[] do not cover member_src[]");
	if (n_merged != (uint64_t)n_promises) as_fail("a promise whose append_interval is no merged block's interval_b");
	for (uint64_t i = 0; i < nba; ++i) if (after[i].kind == TP_NONE) as_fail("applied->n_blocks is not the survivors plus the new blocks (block " + std::to_string(i) + " after)");
	// ---- the blocks of the output
	A.after_first.assign(nba, AS_NONE); A.after_depth.resize(nba);
	for (uint64_t i = 0; i < nba; ++i) A.after_depth[i] = applied->blocks[i].depth;
	if (!merged_only) for (uint64_t i = 0; i < nba; ++i) { A.after_first[i] = A.n_out_members; emit(after[i], after_rc[i]); }
	else for (int64_t e = 0; e < applied->n_new_blocks; ++e) if (applied->new_blocks[e].kind == 1) { const uint32_t i = applied->new_blocks[e].block; A.after_first[i] = A.n_out_members; emit(after[i], after_rc[i]); }
	A.blk_first.push_back(A.n_out_members);
}

// what the device found, lowest offender each; status_k: the slice member behind err[AS_E_STATUS] (from origin[]), to name the promise's member
static void as_report(const as_u64 *err, const AsTables &A, as_u64 status_k, const pga_slice_res_t *slices)
{
	auto at = [](as_u64 x) { return std::to_string(x); };
	if (err[AS_E_SRC_RANGE] != AS_NONE) as_fail("a member_src entry lies outside the slices of its block (member " + at(err[AS_E_SRC_RANGE]) + " after)");
	if (err[AS_E_SRC_TWICE] != AS_NONE) as_fail("a member_src entry is used twice (member " + at(err[AS_E_SRC_TWICE]) + " after)");
	if (err[AS_E_STATUS] != AS_NONE) {
		const as_u64 m = err[AS_E_STATUS], b = ts_last_le(A.blk_first.data(), 0, A.blocks.size(), m);
		const AsBlock &B = A.blocks[b];
		as_fail("solve_promise failed for a member that the merged block takes: its res[] entry has a status other than 0 (promise " + at(B.promise) + ", member " +
		        at(status_k - slices[B.ib].member_off) + "; member " + at(m) + " after)");
	}
	if (err[AS_E_LIST_RANGE] != AS_NONE) as_fail("a source offset + count lies beyond its list (member " + at(err[AS_E_LIST_RANGE]) + " after)");
	if (err[AS_E_SLOT_RANGE] != AS_NONE) as_fail("a node of the graph after names a slot outside its block (node " + at(err[AS_E_SLOT_RANGE]) + ")");
	if (err[AS_E_SLOT_TWICE] != AS_NONE) as_fail("a (block, member) slot after is named by two nodes (node " + at(err[AS_E_SLOT_TWICE]) + ")");
	if (err[AS_E_SLOT_EMPTY] != AS_NONE) as_fail("a (block, member) slot after is named by no node (member " + at(err[AS_E_SLOT_EMPTY]) + " after)");
}
static void as_report_letters(const as_u64 *err)
{
	if (err[AS_E_SEQ_RANGE] != AS_NONE) as_fail("seq_off + len of an insertion lies beyond its letter buffer (insertion " + std::to_string(err[AS_E_SEQ_RANGE]) + " of the output)");
}

} // namespace pga
