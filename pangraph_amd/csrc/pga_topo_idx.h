// pga_topo_idx.h -- the kernels and host tables of pga_topo.hip (the path side of a round of remove_transitive_edges: circularize.rs:11-76
// find_transitive_edges / count_edges, merge_blocks.rs:33-89 orient_merging_edge / find_node_pairings, :196-234 graph_merging_update_paths /
// _nodes).  None of it uses a wave intrinsic -- the block scan goes through LDS and barriers -- so all of this compiles under hipcc and, with
// dev/emu/hip_emu.h included first, under g++ -std=c++17 -DPGA_EMU (tests/emu/topo_emu.cpp runs it against a direct scalar construction).
// The radix sort of the keys and the two scans over run heads are rocPRIM's (pga_topo.hip) and are not in here; the workgroup scan of the
// splice is ts_block_excl of pga_tile_scan.h over 32 bits, the node hash is xxh64_words of pga_xxh64.h.
// pga_apply_idx.h includes this header for the path lookup, the node hash and the splice: the kernels are static, one copy per translation unit.
//
// A POSITION is an index into nodes[] (path after path).  Its SUCCESSOR is the next position of its path, the path's first position behind
// the last one of a circular path, or none; its EDGE is the pair (block, strand) -> (block, strand) of the two in conventional orientation,
// packed as b1 << 33 | b2 << 2 | s1 << 1 | s2 (block indices below 2^31: the all-ones key is free and means "no successor").  Sorted keys are
// the output order (b1, b2, s1, s2); a RUN of equal keys is an edge with its count.
// A SLOT is (block, member) numbered slot_first[block] + member; every slot is named by exactly one position (checked before any list is built).
// For a chosen transitive edge every node of the two blocks lies in exactly one matching pair, and only on the side its strand allows, so
// every partner slot, new node and mark is written by one thread: the pairing needs no atomics.
// The SPLICE is general: position i is replaced by cnt[i] nodes (0 .. k) -- its own node when repl[i] is TP_NONE (cnt[i] == 1), else
// new_nodes[repl[i] .. repl[i] + cnt[i]) -- in tiles of TP_TILE positions: block scan per tile, one workgroup over the tile sums, scatter.
#pragma once
#ifndef PGA_EMU
#include "pga_common.h"
#endif
#include "../../include/pga_align.h"
#include "pga_tile_scan.h"
#include "pga_xxh64.h"
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace pga {

typedef unsigned long long tp_u64;
constexpr int TP_THREADS = TS_THREADS, TP_ITEMS = TS_ITEMS, TP_TILE = TS_TILE;
static_assert(TP_TILE == PGA_TOPO_TILE, "the header exports the tile of the splice");
constexpr uint32_t TP_NONE = 0xffffffffu;
constexpr tp_u64 TP_NOKEY = ~0ULL;
enum { TP_E_DEPTH = 0, TP_E_SLOT = 1, TP_ERRS = 2 };                  // err[]: lowest offending block; lowest offending slot << 1 | named twice

struct TpPick { tp_u64 key, partner_off, anchor_id; uint32_t anchor, left; };   // a chosen edge: its key, where its lists start, the oriented blocks
struct TpDev {
	uint64_t n_nodes, n_paths, n_blocks, n_slots;
	const pga_topo_node_t *nodes; const pga_topo_path_t *paths;
	const uint32_t *depth, *slot_first;      // per block (0 for a dead one); first slot
	uint32_t *path_of;                       // per position
	tp_u64 *key;                             // per position: its edge
	uint32_t *slot_cnt, *blk_cnt, *err;      // positions per slot and per block; TP_ERRS words, all-ones = none
	// the sorted list
	const tp_u64 *skey;                      // n_nodes sorted keys
	uint32_t *head; const uint32_t *head_off;   // n_nodes + 1 entries: a run starts here; exclusive sums (the last: the number of runs)
	uint32_t *run_start;                     // per run, and one behind the last: where the keyed positions end
	uint32_t *keep; const uint32_t *keep_off;   // n_nodes + 1 entries: the run is transitive; exclusive sums (the last: their number)
	pga_topo_edge_t *o_trans, *o_counts;     // o_counts: NULL unless asked for
	// the round
	const uint32_t *choice; const TpPick *pick;   // per block: its edge of the round or TP_NONE
	uint32_t *o_partner; pga_topo_node_t *o_new; uint64_t *o_left, *o_right;
	uint32_t *cnt, *repl;                    // per position (cnt: n_nodes + 1 entries, the last 0)
	// the splice
	uint32_t n_tiles, pad;
	uint32_t *tile_sum, *tile_off;           // tile_off: n_tiles + 1 entries
	uint32_t *pos_off;                       // n_nodes + 1 entries: nodes written before position i
	pga_topo_node_t *o_nodes; pga_topo_path_t *o_paths;
};

__host__ __device__ inline tp_u64 tp_key(uint32_t bi, uint32_t si, uint32_t bj, uint32_t sj)
{
	const bool as_is = bi < bj || (bi == bj && si == 0u);
	const uint32_t b1 = as_is ? bi : bj, s1 = as_is ? si : sj ^ 1u, b2 = as_is ? bj : bi, s2 = as_is ? sj : si ^ 1u;
	return (tp_u64)b1 << 33 | (tp_u64)b2 << 2 | (tp_u64)(s1 << 1 | s2);
}
__host__ __device__ inline pga_topo_edge_t tp_edge(tp_u64 key, uint32_t count)
{
	return pga_topo_edge_t{(uint32_t)(key >> 33), (uint32_t)(key >> 2) & 0x7fffffffu, (int32_t)((key >> 1) & 1u), (int32_t)(key & 1u), count, 0u};
}
// the last path whose node_off is <= i: the one that holds position i (empty paths share their offset with the path behind them)
__host__ __device__ inline uint32_t tp_path_of(const pga_topo_path_t *paths, uint64_t n_paths, uint64_t i)
{
	uint64_t lo = 0, hi = n_paths;                                       // paths[lo].node_off <= i < paths[hi].node_off
	while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (paths[mid].node_off <= i) lo = mid; else hi = mid; }
	return (uint32_t)lo;
}
__host__ __device__ inline uint32_t tp_succ(const pga_topo_path_t &P, uint64_t i)
{
	if (i + 1 < P.node_off + P.n_nodes) return (uint32_t)(i + 1);
	return P.circular ? (uint32_t)P.node_off : TP_NONE;
}
__host__ __device__ inline uint32_t tp_pred(const pga_topo_path_t &P, uint64_t i)
{
	if (i > P.node_off) return (uint32_t)(i - 1);
	return P.circular ? (uint32_t)(P.node_off + P.n_nodes - 1) : TP_NONE;
}

// PangraphNode::new(None, block, path, strand, position): XXH64, seed 0, of five little-endian u64 words
__host__ __device__ inline uint64_t tp_node_id(uint64_t block_id, uint64_t path_id, uint64_t reverse, uint64_t pos0, uint64_t pos1)
{
	const uint64_t w[5] = {block_id, path_id, reverse, pos0, pos1};
	return xxh64_words(w, 5);
}

// ---------------------------------------------------------------- 1. edge keys and the slot counts, one thread per position
static __global__ __launch_bounds__(TP_THREADS) void k_topo_keys(TpDev V)
{
	for (uint64_t i = (uint64_t)blockIdx.x * TP_THREADS + threadIdx.x; i < V.n_nodes; i += (uint64_t)gridDim.x * TP_THREADS) {
		const uint32_t p = tp_path_of(V.paths, V.n_paths, i);
		const pga_topo_node_t A = V.nodes[i];
		const uint32_t j = tp_succ(V.paths[p], i);
		V.path_of[i] = p;
		tp_u64 key = TP_NOKEY;
		if (j != TP_NONE) { const pga_topo_node_t B = V.nodes[j]; key = tp_key(A.block, A.reverse ? 1u : 0u, B.block, B.reverse ? 1u : 0u); }
		V.key[i] = key;
		atomicAdd(&V.slot_cnt[V.slot_first[A.block] + A.member], 1u);     // (block and member were checked on the host)
		atomicAdd(&V.blk_cnt[A.block], 1u);
	}
}
// one thread per slot and per block: a slot named by no position or by two, a block whose positions do not sum to its depth
static __global__ __launch_bounds__(TP_THREADS) void k_topo_check(TpDev V)
{
	const uint64_t n = V.n_slots > V.n_blocks ? V.n_slots : V.n_blocks;
	for (uint64_t x = (uint64_t)blockIdx.x * TP_THREADS + threadIdx.x; x < n; x += (uint64_t)gridDim.x * TP_THREADS) {
		if (x < V.n_slots && V.slot_cnt[x] != 1u) atomicMin(&V.err[TP_E_SLOT], (uint32_t)x << 1 | (V.slot_cnt[x] ? 1u : 0u));
		if (x < V.n_blocks && V.blk_cnt[x] != V.depth[x]) atomicMin(&V.err[TP_E_DEPTH], (uint32_t)x);
	}
}

// ---------------------------------------------------------------- 2. runs of the sorted keys
static __global__ __launch_bounds__(TP_THREADS) void k_topo_heads(TpDev V)
{
	for (uint64_t i = (uint64_t)blockIdx.x * TP_THREADS + threadIdx.x; i <= V.n_nodes; i += (uint64_t)gridDim.x * TP_THREADS)
		V.head[i] = (i < V.n_nodes && V.skey[i] != TP_NOKEY && (i == 0 || V.skey[i] != V.skey[i - 1])) ? 1u : 0u;
}
// behind the scan of head[]: where every run starts; the first position without a key (or n_nodes) closes the last run
static __global__ __launch_bounds__(TP_THREADS) void k_topo_runs(TpDev V)
{
	for (uint64_t i = (uint64_t)blockIdx.x * TP_THREADS + threadIdx.x; i <= V.n_nodes; i += (uint64_t)gridDim.x * TP_THREADS) {
		const bool keyed = i < V.n_nodes && V.skey[i] != TP_NOKEY;
		if (keyed ? V.head[i] != 0u : (i == 0 || V.skey[i - 1] != TP_NOKEY)) V.run_start[V.head_off[i]] = (uint32_t)i;
	}
}
// one thread per run: transitive when the two blocks differ and count == depth of both; every run's record when asked for
static __global__ __launch_bounds__(TP_THREADS) void k_topo_keep(TpDev V)
{
	const uint64_t n_runs = V.head_off[V.n_nodes];
	for (uint64_t r = (uint64_t)blockIdx.x * TP_THREADS + threadIdx.x; r <= V.n_nodes; r += (uint64_t)gridDim.x * TP_THREADS) {
		uint32_t keep = 0;
		if (r < n_runs) {
			const pga_topo_edge_t E = tp_edge(V.skey[V.run_start[r]], V.run_start[r + 1] - V.run_start[r]);
			keep = (E.b1 != E.b2 && E.count == V.depth[E.b1] && E.count == V.depth[E.b2]) ? 1u : 0u;
			if (V.o_counts) V.o_counts[r] = E;
		}
		V.keep[r] = keep;
	}
}
static __global__ __launch_bounds__(TP_THREADS) void k_topo_compact(TpDev V)
{
	const uint64_t n_runs = V.head_off[V.n_nodes];
	for (uint64_t r = (uint64_t)blockIdx.x * TP_THREADS + threadIdx.x; r < n_runs; r += (uint64_t)gridDim.x * TP_THREADS)
		if (V.keep[r]) V.o_trans[V.keep_off[r]] = tp_edge(V.skey[V.run_start[r]], V.run_start[r + 1] - V.run_start[r]);
}

// ---------------------------------------------------------------- 4. the pairing, one thread per position
// whether the pair (position x, its successor y) is an occurrence of a chosen edge; r: the edge
__device__ inline bool tp_matched(const TpDev &V, uint32_t bx, uint32_t by, tp_u64 key, uint32_t &r)
{
	if (key == TP_NOKEY || bx == by) return false;
	r = V.choice[bx];
	return r != TP_NONE && r == V.choice[by] && V.pick[r].key == key;
}
static __global__ __launch_bounds__(TP_THREADS) void k_topo_pair(TpDev V)
{
	for (uint64_t i = (uint64_t)blockIdx.x * TP_THREADS + threadIdx.x; i <= V.n_nodes; i += (uint64_t)gridDim.x * TP_THREADS) {
		if (i == V.n_nodes) { V.cnt[i] = 0; continue; }
		const uint32_t p = V.path_of[i];
		const pga_topo_path_t P = V.paths[p];
		const pga_topo_node_t A = V.nodes[i];
		uint32_t cnt = 1, repl = TP_NONE, r = TP_NONE;
		const uint32_t j = tp_succ(P, i);
		if (j != TP_NONE) {
			const pga_topo_node_t B = V.nodes[j];
			if (tp_matched(V, A.block, B.block, V.key[i], r)) {
				// this thread owns the pair: A is its first node in path order, B its second
				const TpPick K = V.pick[r];
				const bool a_left = A.block == K.left, a_anchor = A.block == K.anchor;
				const pga_topo_node_t &L = a_left ? A : B, &R = a_left ? B : A, &N = a_anchor ? A : B;
				const uint64_t at = K.partner_off + L.member;
				V.o_partner[at] = R.member;
				V.o_new[at] = pga_topo_node_t{tp_node_id(K.anchor_id, P.path_id, N.reverse ? 1u : 0u, A.pos0, B.pos1), A.pos0, B.pos1, K.anchor, L.member, N.reverse ? 1 : 0, 0};
				V.o_left[at] = L.node_id; V.o_right[at] = R.node_id;
				if (a_anchor) repl = (uint32_t)at; else cnt = 0;
			}
		}
		const uint32_t h = repl == TP_NONE && cnt == 1 ? tp_pred(P, i) : TP_NONE;   // (not matched forward: the pair with the predecessor)
		if (h != TP_NONE) {
			const pga_topo_node_t Z = V.nodes[h];
			if (tp_matched(V, Z.block, A.block, V.key[h], r)) {
				const TpPick K = V.pick[r];
				if (A.block == K.anchor) repl = (uint32_t)(K.partner_off + (A.block == K.left ? A.member : Z.member)); else cnt = 0;
			}
		}
		V.cnt[i] = cnt; V.repl[i] = repl;
	}
}

// ---------------------------------------------------------------- 5. the splice
// the workgroup scan is ts_block_excl of pga_tile_scan.h, over 32 bits (the buffers are part of TpDev)
static __global__ __launch_bounds__(TP_THREADS) void k_topo_tile_sums(TpDev V)
{
	__shared__ uint32_t s[TP_THREADS];
	for (uint32_t t = blockIdx.x; t < V.n_tiles; t += gridDim.x) {
		const uint64_t i0 = (uint64_t)t * TP_TILE + (uint64_t)threadIdx.x * TP_ITEMS;
		uint32_t v = 0, total;
		for (int q = 0; q < TP_ITEMS; ++q) if (i0 + q < V.n_nodes) v += V.cnt[i0 + q];
		ts_block_excl(v, s, total);
		if (threadIdx.x == 0) V.tile_sum[t] = total;
	}
}
// ONE workgroup: tile_off[t] = the nodes written by the tiles before t; tile_off[n_tiles] = all of them
static __global__ __launch_bounds__(TP_THREADS) void k_topo_tile_scan(TpDev V)
{
	__shared__ uint32_t s[TP_THREADS];
	uint32_t run = 0;
	for (uint32_t t0 = 0; t0 < V.n_tiles; t0 += TP_THREADS) {
		const uint32_t t = t0 + threadIdx.x, v = t < V.n_tiles ? V.tile_sum[t] : 0u;
		uint32_t total;
		const uint32_t before = ts_block_excl(v, s, total);
		if (t < V.n_tiles) V.tile_off[t] = run + before;
		run += total;
	}
	if (threadIdx.x == 0) V.tile_off[V.n_tiles] = run;
}
static __global__ __launch_bounds__(TP_THREADS) void k_topo_splice(TpDev V)
{
	__shared__ uint32_t s[TP_THREADS];
	for (uint32_t t = blockIdx.x; t < V.n_tiles; t += gridDim.x) {
		const uint64_t i0 = (uint64_t)t * TP_TILE + (uint64_t)threadIdx.x * TP_ITEMS;
		uint32_t c[TP_ITEMS], v = 0, total;
		for (int q = 0; q < TP_ITEMS; ++q) { c[q] = i0 + q < V.n_nodes ? V.cnt[i0 + q] : 0u; v += c[q]; }
		uint32_t at = V.tile_off[t] + ts_block_excl(v, s, total);
		for (int q = 0; q < TP_ITEMS; ++q) {
			const uint64_t i = i0 + q;
			if (i >= V.n_nodes) break;
			V.pos_off[i] = at;
			const uint32_t from = V.repl[i];
			for (uint32_t k = 0; k < c[q]; ++k) V.o_nodes[at + k] = from == TP_NONE ? V.nodes[i] : V.o_new[from + k];
			at += c[q];
			if (i + 1 == V.n_nodes) V.pos_off[V.n_nodes] = at;
		}
	}
}
// a path's new node_off is the scanned value at its old node_off
static __global__ __launch_bounds__(TP_THREADS) void k_topo_paths(TpDev V)
{
	for (uint64_t p = (uint64_t)blockIdx.x * TP_THREADS + threadIdx.x; p < V.n_paths; p += (uint64_t)gridDim.x * TP_THREADS) {
		const pga_topo_path_t P = V.paths[p];
		const uint32_t a = V.pos_off[P.node_off], b = V.pos_off[P.node_off + P.n_nodes];
		V.o_paths[p] = pga_topo_path_t{P.path_id, a, b - a, P.circular};
	}
}

// ---------------------------------------------------------------- host side: validation, the choice of the round, the blocks behind it
struct TpTables {
	std::vector<uint32_t> depth, slot_first;     // per block
	uint64_t n_slots = 0;
};
struct TpRound {
	std::vector<pga_topo_round_t> round; std::vector<TpPick> pick; std::vector<uint32_t> choice;
	uint64_t n_partner = 0;
};
inline void tp_fail(const std::string &what) { throw std::runtime_error("pga_plan_simplify: " + what); }

// everything the host can refuse, before anything is launched
static void tp_validate(int64_t n_blocks, const pga_topo_block_t *blocks, int64_t n_paths, const pga_topo_path_t *paths, int64_t n_nodes, const pga_topo_node_t *nodes,
                        int64_t n_sched, const pga_topo_sched_t *sched, uint32_t flags, TpTables &T)
{
	if (n_blocks < 0 || n_paths < 0 || n_nodes < 0 || n_sched < 0 || (n_blocks && !blocks) || (n_paths && !paths) || (n_nodes && !nodes)) tp_fail("null argument or negative count");
	if (flags & ~(PGA_TOPO_EDGES_ONLY | PGA_TOPO_COUNTS)) tp_fail("unknown flag");
	if (sched ? n_sched == 0 : n_sched != 0) tp_fail("an empty schedule, or a count without a schedule");
	if (n_blocks >= (1LL << 31) || n_paths >= (1LL << 31) || n_nodes >= (1LL << 31)) tp_fail("2^31 or more blocks, paths or nodes");
	T.depth.assign((size_t)n_blocks, 0); T.slot_first.assign((size_t)n_blocks + 1, 0);
	bool any = false; uint64_t last = 0;
	for (int64_t b = 0; b < n_blocks; ++b) {
		T.slot_first[b] = (uint32_t)T.n_slots;
		if (!blocks[b].alive) continue;
		if (any && blocks[b].block_id <= last) tp_fail("the ids of the alive blocks are not strictly ascending (block " + std::to_string(b) + ")");
		any = true; last = blocks[b].block_id;
		T.depth[b] = blocks[b].depth;
		T.n_slots += blocks[b].depth;
		if (T.n_slots >= (1ULL << 31)) tp_fail("2^31 or more members");
	}
	T.slot_first[n_blocks] = (uint32_t)T.n_slots;
	uint64_t run = 0;
	for (int64_t p = 0; p < n_paths; ++p) {
		if (p && paths[p].path_id <= paths[p - 1].path_id) tp_fail("the path ids are not ascending (path " + std::to_string(p) + ")");
		if (paths[p].node_off != run) tp_fail("node_off is not the running sum of n_nodes (path " + std::to_string(p) + ")");
		run += paths[p].n_nodes;
	}
	if (run != (uint64_t)n_nodes) tp_fail("the n_nodes of the paths do not sum to the node count");
	for (int64_t i = 0; i < n_nodes; ++i) {
		const pga_topo_node_t &N = nodes[i];
		if (N.block >= (uint64_t)n_blocks) tp_fail("a node names a block out of range (node " + std::to_string(i) + ")");
		if (!blocks[N.block].alive) tp_fail("a node names a dead block (node " + std::to_string(i) + ")");
		if (N.member >= blocks[N.block].depth) tp_fail("member >= depth (node " + std::to_string(i) + ")");
	}
}

// the round: the greedy walk over the sorted transitive list, or the schedule checked against it; every edge oriented anchor first
static void tp_choose(int64_t n_blocks, const pga_topo_block_t *blocks, const pga_topo_edge_t *trans, uint64_t n_trans, int64_t n_sched, const pga_topo_sched_t *sched, TpRound &R)
{
	R.choice.assign((size_t)n_blocks, TP_NONE);
	std::vector<uint32_t> picked;
	auto key_of = [](const pga_topo_edge_t &E) { return (tp_u64)E.b1 << 33 | (tp_u64)E.b2 << 2 | (tp_u64)((uint32_t)E.s1 << 1 | (uint32_t)E.s2); };
	if (!sched) {
		for (uint64_t t = 0; t < n_trans; ++t) if (R.choice[trans[t].b1] == TP_NONE && R.choice[trans[t].b2] == TP_NONE) {
			R.choice[trans[t].b1] = R.choice[trans[t].b2] = (uint32_t)picked.size();
			picked.push_back((uint32_t)t);
		}
	} else {
		for (int64_t e = 0; e < n_sched; ++e) {
			const pga_topo_sched_t &S = sched[e];
			const std::string who = " (schedule entry " + std::to_string(e) + ")";
			if (S.b1 >= (uint64_t)n_blocks || S.b2 >= (uint64_t)n_blocks) tp_fail("a scheduled edge is not transitive: it names a block out of range" + who);
			const tp_u64 key = tp_key(S.b1, S.s1 ? 1u : 0u, S.b2, S.s2 ? 1u : 0u);
			const pga_topo_edge_t *at = std::lower_bound(trans, trans + n_trans, key, [&](const pga_topo_edge_t &E, tp_u64 k) { return key_of(E) < k; });
			if (at == trans + n_trans || key_of(*at) != key) tp_fail("a scheduled edge is not transitive" + who);
			if (R.choice[at->b1] != TP_NONE || R.choice[at->b2] != TP_NONE) tp_fail("the schedule names a block twice" + who);
			R.choice[at->b1] = R.choice[at->b2] = (uint32_t)picked.size();
			picked.push_back((uint32_t)(at - trans));
		}
	}
	for (uint32_t t : picked) {
		const pga_topo_edge_t &E = trans[t];
		const pga_topo_block_t &B1 = blocks[E.b1], &B2 = blocks[E.b2];
		const bool first = B1.cons_len > B2.cons_len || (B1.cons_len == B2.cons_len && B1.block_id < B2.block_id);
		pga_topo_round_t O;
		memset(&O, 0, sizeof(O));
		O.anchor = first ? E.b1 : E.b2; O.other = first ? E.b2 : E.b1;
		O.anchor_rev = first ? E.s1 : E.s2 ^ 1; O.other_rev = first ? E.s2 : E.s1 ^ 1;
		O.transitive = t;
		const int32_t rc = O.anchor_rev != O.other_rev ? 1 : 0;
		O.merge = O.anchor_rev == 0 ? pga_merge_edge_t{O.anchor, O.other, 0, rc} : pga_merge_edge_t{O.other, O.anchor, rc, 0};
		O.partner_off = R.n_partner;
		if ((uint64_t)B1.cons_len + B2.cons_len >= (1ULL << 32)) tp_fail("a merged consensus of 2^32 letters or more (blocks " + std::to_string(E.b1) + " and " + std::to_string(E.b2) + ")");
		R.pick.push_back(TpPick{key_of(E), R.n_partner, blocks[O.anchor].block_id, O.anchor, O.merge.left});
		R.round.push_back(O);
		R.n_partner += E.count;
	}
}
// the anchor block takes both lengths and keeps its depth, the other block dies
static void tp_blocks_after(int64_t n_blocks, const pga_topo_block_t *blocks, const TpRound &R, pga_topo_block_t *o)
{
	for (int64_t b = 0; b < n_blocks; ++b) { o[b] = blocks[b]; o[b].pad = 0; if (!o[b].alive) { o[b].depth = 0; o[b].cons_len = 0; } }
	for (const pga_topo_round_t &O : R.round) {
		o[O.anchor].cons_len = blocks[O.anchor].cons_len + blocks[O.other].cons_len;
		o[O.other].alive = 0; o[O.other].depth = 0; o[O.other].cons_len = 0;
	}
}

} // namespace pga
