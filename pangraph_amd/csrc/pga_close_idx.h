// pga_close_idx.h -- the kernels and host tables of pga_close.hip (the tail of a self-merge round folded back into the flat graph and the
// block arrays: graph_merging.rs:153-169 self_merge, reconsensus.rs:46-91 reconsensus_graph, detach_unaligned.rs:24-114).
// No wave intrinsic, atomicAdd / atomicMin only: all of this compiles under hipcc and, with dev/emu/hip_emu.h included first, under
// g++ -std=c++17 -DPGA_EMU (tests/emu/close_emu.cpp runs it against a direct scalar construction).
// The scans are the tile scan of pga_tile_scan.h; the list copies, the letter gather and their value functors are pga_assemble_idx.h's
// (k_assemble_copy, k_assemble_letters, k_assemble_seq_off over an AsDev): this header only fills the descriptors they read, with the two
// sources AS_SRC_BEFORE (the caller's arrays) and AS_SRC_PROMISE (the second detach's lists, whose letters are the reconsensus').
//
// MERGED MEMBER m: member of the merged-only arrays, block j = the last one with mfirst[j] <= m, slot m - mfirst[j]; it is global member
// first_member[upd[j]] + slot of the arrays given.  STAGE 1 is the first detach (places: K1 kept, then n1 orphans), STAGE 2 the second (K1
// members in; K2 kept, then n2 orphans).  A stage's member_map is held against what it must be: a kept member's place is its block's first
// kept place plus its rank among the kept members of its block (the KEPT scan of the stage: one flag per member), an orphan's place names an
// orphan record that names the member back.  Together with the per-block kept counts and the host's totals that makes the map a bijection
// that keeps the order; nothing reads through a place that failed.
// An ORPHAN is numbered k: the first stage's records, then the second's.  The SINGLETON ids are sorted (rocPRIM on the device, std::sort
// under the emulation); a singleton's index after is its rank plus the survivors with a smaller id, a survivor's index its rank among the
// alive blocks plus the singletons with an id not above its own -- a permutation of the blocks after whatever the ids are, so a duplicate
// id is reported and nothing is written twice.
// An OUTPUT MEMBER's DESCRIPTOR (AsDesc) is made by one thread per output member: the block record after (ClBlock) says whether it is a
// survivor's, an updated block's or a singleton's; its origin is the global member before, where[origin] its (block, slot) after, read by
// the node rewrite.
#pragma once
#include "pga_assemble_idx.h"

namespace pga {

typedef as_u64 cl_u64;
constexpr int CL_THREADS = TS_THREADS, CL_TILE = TS_TILE;
enum { CL_SCAN_BEFORE = 0, CL_SCAN_SECOND = 1, CL_SCAN_KEPT1 = 2, CL_SCAN_KEPT2 = 3, CL_SCAN_BLOCKS = 4, CL_SCANS = 5 };
enum { CL_K_SURVIVOR = 0, CL_K_UPDATED = 1, CL_K_SINGLETON = 2 };
// err[]: the lowest offender (merged member; stage-2 member; updated block; updated block; orphan; orphan), all-ones = none
enum { CL_E_MAP1 = 0, CL_E_MAP2 = 1, CL_E_DEPTH1 = 2, CL_E_DEPTH2 = 3, CL_E_KIND = 4, CL_E_ID = 5, CL_ERRS = 6 };
constexpr cl_u64 CL_NONE = ~0ULL;
constexpr uint32_t CL_ORPHAN = 0x80000000u;                                // in ClWhere.block: the member became a singleton block

struct ClBlock { uint32_t kind, src, depth, pad; };                       // a block after.  src: graph block before; updated block j; orphan k
struct ClWhere { uint32_t block, slot; };                                 // per global member before: its place after (block: TP_NONE = unwritten)
struct ClDev {
	AsDev A;                                                           // descriptors, output lists, letters: the copies of pga_assemble_idx.h
	uint64_t n_upd, n_merged, n_k1, n_k2, n_o1, n_orphans, n_alive, n_blocks, n_out_blocks, n_nodes;
	const pga_topo_block_t *blocks; const pga_topo_node_t *nodes;
	const uint32_t *first_member;                                      // per graph block before (n_blocks + 1)
	const uint32_t *upd;                                               // per updated block: its graph block
	const cl_u64 *mfirst, *r1first, *r2first;                          // per updated block (n_upd + 1): first merged member, first kept place of stage 1, of stage 2
	const uint32_t *rc_len; const int32_t *kinds;                      // per updated block: cons_len and kind after the reconsensus
	const long long *map1, *map2;                                      // member_map of the two stages (n_merged, n_k1)
	const pga_rc_member_t *members2;                                   // the second detach's kept members (n_k2)
	const pga_detach_orphan_t *orphans;                                // n_orphans records as given: the first stage's, then the second's
	const pga_detach_member_t *who;                                    // per global member before
	const cl_u64 *alive_id; const uint32_t *alive_block, *alive_upd;   // per alive block in index order: id, graph block, updated block j or TP_NONE
	const cl_u64 *sing_id; const uint32_t *sing_orphan;                // the singleton ids ascending, and the orphan behind each
	cl_u64 *fin_src, *orph_src;                                        // per stage-2 kept place, per orphan: the global member before (all-ones before)
	RmScan scan[CL_SCANS];
	ClBlock *o_rec; pga_topo_block_t *o_blocks; uint32_t *block_map;   // per block after; block_map per graph block before (all-ones before)
	ClWhere *where;                                                    // per global member before (all-ones before)
	pga_detach_member_t *o_who; pga_detach_orphan_t *o_orphans; pga_topo_node_t *o_nodes;
	cl_u64 *err;                                                       // CL_ERRS words
};

// what the scans sum: the lists of the second detach's kept members, the kept flags of the two stages, the depths of the blocks after
struct ClSecondValue {
	ClDev V;
	__host__ __device__ cl_u64 operator()(int q, uint64_t i) const
	{
		const pga_rc_member_t M = V.members2[i];
		return q == RM_LIST_SUB ? M.n_subs : q == RM_LIST_DEL ? M.n_dels : M.n_inss;
	}
};
struct ClKeptValue {
	const long long *map; cl_u64 n_kept;
	__host__ __device__ cl_u64 operator()(int, uint64_t i) const { return map[i] >= 0 && (cl_u64)map[i] < n_kept ? 1ULL : 0ULL; }
};
struct ClDepthValue { ClDev V; __host__ __device__ cl_u64 operator()(int, uint64_t i) const { return V.o_rec[i].kind > (uint32_t)CL_K_SINGLETON ? 0ULL : V.o_rec[i].depth; } };

// the number of entries of the ascending a[0 .. n) below x (strict) or not above it
__host__ __device__ inline cl_u64 cl_count_below(const cl_u64 *a, cl_u64 n, cl_u64 x, bool or_equal)
{
	cl_u64 lo = 0, hi = n;
	while (lo < hi) { const cl_u64 mid = (lo + hi) >> 1; if (a[mid] < x || (or_equal && a[mid] == x)) lo = mid + 1; else hi = mid; }
	return lo;
}

// ---------------------------------------------------------------- 1. one stage's member_map held against what it must be
// x runs over the stage's members and over the updated blocks.  first_in: the first member of a block in this stage's input numbering;
// first_kept: its first kept place; n_kept_block: what the stage's output says it kept.
template <int STAGE> static __global__ __launch_bounds__(CL_THREADS) void k_close_stage(ClDev V)
{
	const cl_u64 n_in = STAGE == 1 ? V.n_merged : V.n_k1, n_kept = STAGE == 1 ? V.n_k1 : V.n_k2, n_orph = STAGE == 1 ? V.n_o1 : V.n_orphans - V.n_o1;
	const cl_u64 *first_in = STAGE == 1 ? V.mfirst : V.r1first, *first_kept = STAGE == 1 ? V.r1first : V.r2first;
	const long long *map = STAGE == 1 ? V.map1 : V.map2;
	const pga_detach_orphan_t *orph = V.orphans + (STAGE == 1 ? 0 : V.n_o1);
	const cl_u64 *kept = ts_off(V.scan[STAGE == 1 ? CL_SCAN_KEPT1 : CL_SCAN_KEPT2], 0);
	const int e_map = STAGE == 1 ? CL_E_MAP1 : CL_E_MAP2, e_depth = STAGE == 1 ? CL_E_DEPTH1 : CL_E_DEPTH2;
	const cl_u64 n = n_in > V.n_upd ? n_in : V.n_upd;
	for (cl_u64 x = (cl_u64)blockIdx.x * CL_THREADS + threadIdx.x; x < n; x += (cl_u64)gridDim.x * CL_THREADS) {
		if (x < V.n_upd && kept[first_in[x + 1]] - kept[first_in[x]] != first_kept[x + 1] - first_kept[x]) atomicMin(&V.err[e_depth], x);
		if (x >= n_in) continue;
		const cl_u64 j = ts_last_le(first_in, 0, V.n_upd, x);
		const long long v = map[x];
		if (v < 0 || (cl_u64)v >= n_kept + n_orph) { atomicMin(&V.err[e_map], x); continue; }
		if ((cl_u64)v < n_kept) { if ((cl_u64)v != first_kept[j] + (kept[x] - kept[first_in[j]])) atomicMin(&V.err[e_map], x); continue; }
		if (orph[(cl_u64)v - n_kept].member != x) atomicMin(&V.err[e_map], x);
		else if (STAGE == 2 && V.kinds[j] != 2) atomicMin(&V.err[CL_E_KIND], V.n_o1 + ((cl_u64)v - n_kept));
	}
}

// ---------------------------------------------------------------- 2. the member chain, one thread per merged member
// Every place is held against its range here as well: this kernel runs beside k_close_stage, not behind a wait.
static __global__ __launch_bounds__(CL_THREADS) void k_close_chain(ClDev V)
{
	const cl_u64 n_o2 = V.n_orphans - V.n_o1;
	for (cl_u64 m = (cl_u64)blockIdx.x * CL_THREADS + threadIdx.x; m < V.n_merged; m += (cl_u64)gridDim.x * CL_THREADS) {
		const cl_u64 j = ts_last_le(V.mfirst, 0, V.n_upd, m), a = V.first_member[V.upd[j]] + (m - V.mfirst[j]);
		const long long v1 = V.map1[m];
		if (v1 < 0 || (cl_u64)v1 >= V.n_k1 + V.n_o1) continue;
		if ((cl_u64)v1 >= V.n_k1) { V.orph_src[(cl_u64)v1 - V.n_k1] = a; continue; }
		const long long v2 = V.map2[v1];
		if (v2 < 0 || (cl_u64)v2 >= V.n_k2 + n_o2) continue;
		if ((cl_u64)v2 >= V.n_k2) V.orph_src[V.n_o1 + ((cl_u64)v2 - V.n_k2)] = a;
		else V.fin_src[v2] = a;
	}
}

// ---------------------------------------------------------------- 3. the block table after: behind the sort of the singleton ids
// x runs over the singletons in id order and over the alive blocks in index order
static __global__ __launch_bounds__(CL_THREADS) void k_close_rank(ClDev V)
{
	const cl_u64 n = V.n_orphans > V.n_alive ? V.n_orphans : V.n_alive;
	for (cl_u64 x = (cl_u64)blockIdx.x * CL_THREADS + threadIdx.x; x < n; x += (cl_u64)gridDim.x * CL_THREADS) {
		if (x < V.n_orphans) {
			const cl_u64 id = V.sing_id[x], below = cl_count_below(V.alive_id, V.n_alive, id, false);
			const uint32_t k = V.sing_orphan[x];
			if ((below < V.n_alive && V.alive_id[below] == id) || (x && V.sing_id[x - 1] == id)) atomicMin(&V.err[CL_E_ID], (cl_u64)k);
			V.o_rec[x + below] = ClBlock{CL_K_SINGLETON, k, 1u, 0u};
			V.o_blocks[x + below] = pga_topo_block_t{id, V.orphans[k].len, 1u, 1, 0};
		}
		if (x < V.n_alive) {
			const uint32_t b = V.alive_block[x], j = V.alive_upd[x];
			const cl_u64 i = x + cl_count_below(V.sing_id, V.n_orphans, V.alive_id[x], true);
			const pga_topo_block_t B = V.blocks[b];
			const uint32_t depth = j == TP_NONE ? B.depth : (uint32_t)(V.r2first[j + 1] - V.r2first[j]);
			V.o_rec[i] = j == TP_NONE ? ClBlock{CL_K_SURVIVOR, b, depth, 0u} : ClBlock{CL_K_UPDATED, j, depth, 0u};
			V.o_blocks[i] = pga_topo_block_t{B.block_id, j == TP_NONE ? B.cons_len : V.rc_len[j], depth, 1, 0};
			V.block_map[b] = (uint32_t)i;
		}
	}
}

// ---------------------------------------------------------------- 4. behind the BLOCKS scan: one thread per output member, its descriptor
// A member whose chain was refused keeps three empty lists and writes no place.
static __global__ __launch_bounds__(CL_THREADS) void k_close_desc(ClDev V)
{
	const cl_u64 *first = ts_off(V.scan[CL_SCAN_BLOCKS], 0);
	const RmScan SB = V.scan[CL_SCAN_BEFORE], S2 = V.scan[CL_SCAN_SECOND];
	for (cl_u64 m = (cl_u64)blockIdx.x * CL_THREADS + threadIdx.x; m < V.A.n_out_members; m += (cl_u64)gridDim.x * CL_THREADS) {
		const cl_u64 i = ts_last_le(first, 0, V.n_out_blocks, m), s = m - first[i];
		const ClBlock B = V.o_rec[i];
		AsDesc D = {{0, 0, 0}, {0, 0, 0}, AS_SRC_BEFORE};
		cl_u64 origin = CL_NONE;
		if (B.kind <= (uint32_t)CL_K_SINGLETON && s < B.depth) {
			if (B.kind == CL_K_SURVIVOR) {
				origin = V.first_member[B.src] + s;
				const pga_rc_member_t M = V.A.members[origin];
				D.n[0] = M.n_subs; D.n[1] = M.n_dels; D.n[2] = M.n_inss;
				for (int q = 0; q < 3; ++q) D.off[q] = ts_off(SB, q)[origin];
			} else if (B.kind == CL_K_UPDATED) {
				const cl_u64 f = V.r2first[B.src] + s;
				origin = V.fin_src[f];
				if (origin != CL_NONE) {
					const pga_rc_member_t M = V.members2[f];
					D.n[0] = M.n_subs; D.n[1] = M.n_dels; D.n[2] = M.n_inss; D.src = AS_SRC_PROMISE;
					for (int q = 0; q < 3; ++q) D.off[q] = ts_off(S2, q)[f];
				}
			} else {
				origin = V.orph_src[B.src];
				if (origin != CL_NONE) {
					pga_detach_orphan_t O = V.orphans[B.src];
					O.member = origin; O.block = (uint32_t)i; O.pad = 0;
					V.o_orphans[B.src] = O;
				}
			}
		}
		V.A.desc[m] = D; V.A.o_members[m] = pga_rc_member_t{D.n[0], D.n[1], D.n[2]};
		V.A.origin[m] = origin == CL_NONE ? -1LL : (long long)origin;
		if (origin == CL_NONE) continue;
		const pga_detach_member_t W = V.who[origin];
		V.o_who[m] = pga_detach_member_t{W.node_id, B.kind == CL_K_SINGLETON ? 0 : (W.reverse ? 1 : 0), 0};
		V.where[origin] = ClWhere{(uint32_t)i | (B.kind == CL_K_SINGLETON ? CL_ORPHAN : 0u), (uint32_t)s};
	}
}

// ---------------------------------------------------------------- 5. the node rewrite, one thread per position
static __global__ __launch_bounds__(CL_THREADS) void k_close_nodes(ClDev V)
{
	for (cl_u64 i = (cl_u64)blockIdx.x * CL_THREADS + threadIdx.x; i < V.n_nodes; i += (cl_u64)gridDim.x * CL_THREADS) {
		pga_topo_node_t N = V.nodes[i];
		const ClWhere W = V.where[V.first_member[N.block] + N.member];       // (block and member were checked on the host)
		if (W.block != TP_NONE) {
			N.block = W.block & ~CL_ORPHAN; N.member = W.slot; N.pad = 0;
			if (W.block & CL_ORPHAN) N.reverse = 0;
		}
		V.o_nodes[i] = N;
	}
}

// ---------------------------------------------------------------- host side: everything that is refused before a launch, and the tables
struct ClTables {
	TpTables T;
	std::vector<uint32_t> upd_of;                                      // per graph block: its updated block or TP_NONE
	std::vector<cl_u64> mfirst, r1first, r2first;                      // n_upd + 1 each
	std::vector<uint32_t> rc_len; std::vector<int32_t> kinds;
	std::vector<cl_u64> alive_id; std::vector<uint32_t> alive_block, alive_upd;
	std::vector<pga_detach_orphan_t> orphans;
	uint64_t n_before = 0, n_merged = 0, n_k1 = 0, n_k2 = 0, n_o1 = 0, n_o2 = 0, n_out_blocks = 0, n_out_members = 0;
	uint64_t before_tot[3] = {0, 0, 0}, second_tot[3] = {0, 0, 0};
};
inline void cl_fail(const std::string &what) { throw std::runtime_error("pga_close_round: " + what); }

static void cl_validate(int64_t n_blocks, const pga_topo_block_t *blocks, int64_t n_paths, const pga_topo_path_t *paths, int64_t n_nodes, const pga_topo_node_t *nodes,
                        const pga_rc_block_t *rc_blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss,
                        const pga_detach_member_t *who, int64_t n_upd, const uint32_t *upd, const pga_detach_out_t *detached, const pga_rc_out_t *rc,
                        const pga_detach_out_t *redetached, uint32_t flags, ClTables &C)
{
	const char *null = "null argument or negative count";
	const uint64_t lim = 1ULL << 63, lim31 = 1ULL << 31;
	try { tp_validate(n_blocks, blocks, n_paths, paths, n_nodes, nodes, 0, nullptr, 0, C.T); }
	catch (std::runtime_error &e) { const std::string w = e.what(); const size_t at = w.find(": "); cl_fail(at == std::string::npos ? w : w.substr(at + 2)); }
	if (flags & ~PGA_CLOSE_COPY_CONSENSUS) cl_fail("unknown flag");
	if (n_upd < 0 || (n_blocks && !rc_blocks) || (n_upd && (!upd || !detached || !rc || !redetached))) cl_fail(null);
	for (int64_t b = 0; b < n_blocks; ++b) {
		if (rc_blocks[b].n_members != C.T.depth[b]) cl_fail(std::string(blocks[b].alive ? "n_members of a block differs from its depth" : "a dead block with members") + " (block " + std::to_string(b) + ")");
		// (the consensus copies of the host read blocks[b].cons_len letters through rc_blocks[b].consensus)
		if (blocks[b].alive && rc_blocks[b].cons_len != blocks[b].cons_len) cl_fail("cons_len of a block differs between the graph and the block arrays (block " + std::to_string(b) + ")");
	}
	C.n_before = C.T.n_slots;
	if (C.n_before && (!members || !who)) cl_fail(null);
	for (uint64_t m = 0; m < C.n_before; ++m) {
		C.before_tot[0] += members[m].n_subs; C.before_tot[1] += members[m].n_dels; C.before_tot[2] += members[m].n_inss;
		if (C.before_tot[0] >= lim || C.before_tot[1] >= lim || C.before_tot[2] >= lim) cl_fail("the edit counts overflow 2^63");
	}
	if ((C.before_tot[0] && !subs) || (C.before_tot[1] && !dels) || (C.before_tot[2] && !inss)) cl_fail(null);
	// ---- the updated blocks
	C.upd_of.assign((size_t)n_blocks, TP_NONE);
	C.mfirst.assign((size_t)n_upd + 1, 0); C.r1first.assign((size_t)n_upd + 1, 0); C.r2first.assign((size_t)n_upd + 1, 0);
	C.rc_len.assign((size_t)n_upd, 0); C.kinds.assign((size_t)n_upd, 0);
	for (int64_t j = 0; j < n_upd; ++j) {
		const std::string at = " (updated block " + std::to_string(j) + ")";
		if (upd[j] >= (uint64_t)n_blocks) cl_fail("an updated block is out of range" + at);
		if (!blocks[upd[j]].alive) cl_fail("an updated block is dead" + at);
		if (C.upd_of[upd[j]] != TP_NONE) cl_fail("an updated block is named twice" + at);
		C.upd_of[upd[j]] = (uint32_t)j;
		C.mfirst[j + 1] = C.mfirst[j] + C.T.depth[upd[j]];
	}
	C.n_merged = C.mfirst[n_upd];
	if (n_upd) {
		// ---- the two detach outputs and the reconsensus between them
		if (detached->n_orphans < 0 || redetached->n_orphans < 0 || !detached->blocks || !redetached->blocks || !rc->blocks) cl_fail(null);
		if (detached->n_blocks != n_upd + detached->n_orphans) cl_fail("detached->n_blocks is not n_upd + its orphans");
		if (redetached->n_blocks != n_upd + redetached->n_orphans) cl_fail("redetached->n_blocks is not n_upd + its orphans");
		C.n_o1 = (uint64_t)detached->n_orphans; C.n_o2 = (uint64_t)redetached->n_orphans;
		if ((C.n_o1 && !detached->orphans) || (C.n_o2 && !redetached->orphans) || (C.n_merged && !detached->member_map)) cl_fail(null);
		for (int64_t j = 0; j < n_upd; ++j) {
			C.r1first[j + 1] = C.r1first[j] + detached->blocks[j].n_members; C.r2first[j + 1] = C.r2first[j] + redetached->blocks[j].n_members;
			const pga_rc_block_res_t &R = rc->blocks[j];
			if (R.kind < 0) cl_fail("the reconsensus failed for a block (updated block " + std::to_string(j) + ", kind " + std::to_string(R.kind) + ")");
			if (R.kind > 2) cl_fail("an unknown reconsensus kind (updated block " + std::to_string(j) + ", kind " + std::to_string(R.kind) + ")");
			if (R.kind && R.cons_len && !rc->cons) cl_fail(null);
			if (R.kind == 0 && R.cons_len != rc_blocks[upd[j]].cons_len) cl_fail("a kind-0 block whose cons_len changed (updated block " + std::to_string(j) + ")");
			C.rc_len[j] = R.cons_len; C.kinds[j] = R.kind;
		}
		C.n_k1 = C.r1first[n_upd]; C.n_k2 = C.r2first[n_upd];
		if (C.n_k1 + C.n_o1 != C.n_merged) cl_fail("the kept members and the orphans of the first detach are not the members of the updated blocks");
		if (C.n_k2 + C.n_o2 != C.n_k1) cl_fail("the kept members and the orphans of the second detach are not the members the first one kept");
		if (C.n_k1 && (!rc->members || !redetached->member_map)) cl_fail(null);
		if (C.n_k2 && !redetached->members) cl_fail(null);
		for (int64_t j = 0; j < n_upd; ++j) for (cl_u64 m1 = C.r1first[j]; m1 < C.r1first[j + 1]; ++m1)
			if (rc->members[m1].status != 0) cl_fail("the realignment of a member failed: its rc->members[] entry has a status other than 0 (updated block " + std::to_string(j) + ", member " + std::to_string(m1 - C.r1first[j]) + ", status " + std::to_string(rc->members[m1].status) + ")");
		for (uint64_t f = 0; f < C.n_k2; ++f) {
			const pga_rc_member_t &M = redetached->members[f];
			C.second_tot[0] += M.n_subs; C.second_tot[1] += M.n_dels; C.second_tot[2] += M.n_inss;
			if (C.second_tot[0] >= lim || C.second_tot[1] >= lim || C.second_tot[2] >= lim) cl_fail("the edit counts overflow 2^63");
		}
		if ((C.second_tot[0] && !redetached->subs) || (C.second_tot[1] && !redetached->dels) || (C.second_tot[2] && !redetached->inss)) cl_fail(null);
		for (int stage = 0; stage < 2; ++stage) {
			const pga_detach_out_t *D = stage ? redetached : detached;
			for (int64_t k = 0; k < D->n_orphans; ++k) {
				const pga_detach_orphan_t &O = D->orphans[k];
				if (O.status != 0) cl_fail("an orphan's sequence was not built: its record has a status other than 0 (" + std::string(stage ? "second" : "first") + " detach, orphan " + std::to_string(k) + ", status " + std::to_string(O.status) + ")");
				// (the letters of orphan k are read at blocks[n_upd + k], as pga_detach_unaligned lays them out)
				if (O.block != (uint64_t)(n_upd + k) || D->blocks[n_upd + k].cons_len != O.len) cl_fail("an orphan record does not name its singleton block (" + std::string(stage ? "second" : "first") + " detach, orphan " + std::to_string(k) + ")");
				if (O.len && !D->blocks[n_upd + k].consensus) cl_fail(null);
				C.orphans.push_back(O);
			}
		}
	}
	// ---- the alive blocks in index order; the counts after
	for (int64_t b = 0; b < n_blocks; ++b) if (blocks[b].alive) { C.alive_id.push_back(blocks[b].block_id); C.alive_block.push_back((uint32_t)b); C.alive_upd.push_back(C.upd_of[b]); }
	C.n_out_blocks = C.alive_id.size() + C.n_o1 + C.n_o2;
	C.n_out_members = C.n_before - C.n_merged + C.n_k2 + C.n_o1 + C.n_o2;
	if (C.n_out_blocks >= lim31 || C.n_out_members >= lim31) cl_fail("2^31 or more blocks or members after");
}

// what the device found before the first wait, lowest offender each
static void cl_report(const uint32_t *topo_err, const cl_u64 *err, const ClTables &C)
{
	auto at = [](cl_u64 x) { return std::to_string(x); };
	if (topo_err[TP_E_DEPTH] != TP_NONE) cl_fail("the nodes of a block do not sum to its depth (block " + at(topo_err[TP_E_DEPTH]) + ")");
	if (topo_err[TP_E_SLOT] != TP_NONE) cl_fail(std::string("a (block, member) slot is named by ") + ((topo_err[TP_E_SLOT] & 1u) ? "two nodes" : "no node") + " (slot " + at(topo_err[TP_E_SLOT] >> 1) + ")");
	if (err[CL_E_DEPTH1] != CL_NONE) cl_fail("the kept members and the orphans of a block do not sum to its depth (first detach, updated block " + at(err[CL_E_DEPTH1]) + ")");
	if (err[CL_E_MAP1] != CL_NONE) cl_fail("member_map is no bijection onto the kept places and the orphans (first detach, member " + at(err[CL_E_MAP1]) + ")");
	if (err[CL_E_DEPTH2] != CL_NONE) cl_fail("the kept members and the orphans of a block do not sum to its depth (second detach, updated block " + at(err[CL_E_DEPTH2]) + ")");
	if (err[CL_E_MAP2] != CL_NONE) cl_fail("member_map is no bijection onto the kept places and the orphans (second detach, member " + at(err[CL_E_MAP2]) + ")");
	if (err[CL_E_KIND] != CL_NONE) cl_fail("the second detach took a member out of a block that was not realigned (orphan " + at(err[CL_E_KIND] - C.n_o1) + " of the second detach)");
	if (err[CL_E_ID] != CL_NONE) cl_fail("Conflicting key: a singleton block_id equals a surviving block's or another singleton's (orphan " + at(err[CL_E_ID]) + ")");
}
static void cl_report_letters(const as_u64 *err)
{
	if (err[AS_E_SEQ_RANGE] != AS_NONE) cl_fail("seq_off + len of an insertion lies beyond its letter buffer (insertion " + std::to_string(err[AS_E_SEQ_RANGE]) + " of the output)");
}

// pga_rc_detach_args: the first arguments of the second pga_detach_unaligned from a pga_rc_out_t (host only)
static void cl_detach_args(int64_t n_upd, const pga_detach_out_t *detached, const pga_detach_member_t *who_merged, const pga_rc_out_t *rc,
                           pga_rc_block_t *blocks, pga_rc_member_t *members, pga_detach_member_t *who2)
{
	auto fail = [](const std::string &what) { throw std::runtime_error("pga_rc_detach_args: " + what); };
	if (n_upd < 0 || (n_upd && (!detached || !rc || !blocks || !detached->blocks || !rc->blocks))) fail("null argument or negative count");
	if (n_upd == 0) return;
	if (detached->n_orphans < 0 || detached->n_blocks != n_upd + detached->n_orphans) fail("detached->n_blocks is not n_upd + its orphans");
	uint64_t n_kept = 0;
	for (int64_t j = 0; j < n_upd; ++j) {
		const pga_rc_block_res_t &R = rc->blocks[j];
		if (R.cons_len && !rc->cons) fail("null argument or negative count");
		blocks[j] = pga_rc_block_t{rc->cons ? rc->cons + R.cons_off : nullptr, R.cons_len, detached->blocks[j].n_members};
		n_kept += detached->blocks[j].n_members;
	}
	const uint64_t n_all = n_kept + (uint64_t)detached->n_orphans;
	if (n_kept && (!members || !who2 || !rc->members)) fail("null argument or negative count");
	if (n_all && (!detached->member_map || !who_merged)) fail("null argument or negative count");
	for (uint64_t m1 = 0; m1 < n_kept; ++m1) members[m1] = pga_rc_member_t{rc->members[m1].n_subs, rc->members[m1].n_dels, rc->members[m1].n_inss};
	for (uint64_t m = 0; m < n_all; ++m) {
		const int64_t v = detached->member_map[m];
		if (v < 0 || (uint64_t)v >= n_all) fail("member_map is out of range (member " + std::to_string(m) + ")");
		if ((uint64_t)v < n_kept) who2[v] = who_merged[m];
	}
}

} // namespace pga
