// pga_remove_idx.h -- the kernels and host tables of pga_remove.hip (the first step of `pangraph simplify`: Pangraph::remove_path,
// pangraph/pangraph.rs:110-132, for every path that is not kept, on the flat graph of pga_plan_simplify and the block arrays of pga_merge_blocks).
// No wave intrinsic, atomicAdd / atomicMin only: all of this compiles under hipcc and, with dev/emu/hip_emu.h included first, under
// g++ -std=c++17 -DPGA_EMU (tests/emu/remove_emu.cpp runs it against a direct scalar construction).
// The path lookup and the graph checks are pga_topo_idx.h's; the scans are the tile scan of pga_tile_scan.h over 64-bit values, several
// quantities side by side, with the value functors below.
//
// A MEMBER is a global member, first_member[block] + member: the SLOT of pga_topo_idx.h under another name (a dead block has no member, so
// slot_first[] is first_member[]).  It is KEPT when the path of the node that names it is.  A path is kept or removed as a whole, so a kept
// node's place after is (its path's new node_off) + (its place inside the path): the path table after is the host's (O(paths)), the nodes
// need no scan of their own.
// The MEMBER SCAN has seven quantities (RM_Q_*): the kept flag, the three list lengths of every member (where its lists start in the input)
// and the three list lengths of the kept members (where they start in the output).  The LETTER SCAN (PGA_REMOVE_COMPACT_LETTERS) has one:
// the length of every insertion in the output, whose sums are the new seq_off.
// A LIST COPY is spread over the elements of the OUTPUT list in tiles of RM_TILE: the members of a tile's first and last element are looked
// up once per workgroup, every thread then finds the member of its element between the two (no step at all inside a long list).
#pragma once
#include "pga_topo_idx.h"

namespace pga {

typedef unsigned long long rm_u64;
constexpr int RM_THREADS = TS_THREADS, RM_TILE = TS_TILE;
enum { RM_Q_KEPT = 0, RM_Q_IN_SUB = 1, RM_Q_IN_DEL = 2, RM_Q_IN_INS = 3, RM_Q_OUT_SUB = 4, RM_Q_OUT_DEL = 5, RM_Q_OUT_INS = 6, RM_QS = 7 };
enum { RM_SCAN_MEMBERS = 0, RM_SCAN_LETTERS = 1, RM_SCANS = 2 };
enum { RM_LIST_SUB = 0, RM_LIST_DEL = 1, RM_LIST_INS = 2 };
enum { RM_E_INS_NULL = 0, RM_E_INS_RANGE = 1, RM_ERRS = 2 };              // err[]: the lowest offending insertion of the output, all-ones = none
constexpr rm_u64 RM_NONE = ~0ULL;

typedef TileScan<rm_u64> RmScan;                                           // pga_tile_scan.h: n_q quantities side by side
struct RmDev {
	uint64_t n_nodes, n_paths, n_blocks, n_members, ins_seq_len;
	uint32_t flags, pad;
	const pga_topo_node_t *nodes; const pga_topo_path_t *paths; const pga_topo_block_t *blocks;
	const uint32_t *slot_first, *path_of;                  // as in TpDev (path_of: behind k_topo_keys)
	const uint8_t *keep;                                   // per path
	const rm_u64 *path_new_off;                            // per path: its node_off after (a removed path: anything)
	const pga_rc_member_t *members; const pga_sub_t *subs; const pga_del_t *dels; const pga_ins_t *inss; const char *ins_seq;
	uint32_t *mkeep;                                       // per member: kept (zeroed before)
	RmScan scan[RM_SCANS];
	pga_topo_block_t *o_blocks; pga_topo_node_t *o_nodes;
	pga_rc_member_t *o_members; pga_sub_t *o_subs; pga_del_t *o_dels; pga_ins_t *o_inss; char *o_ins_seq;
	long long *member_map;
	rm_u64 *err;                                           // RM_ERRS words
};

// what a member is worth in the member scan, an output insertion in the letter scan
struct RmMemberValue {
	RmDev V;
	__host__ __device__ rm_u64 operator()(int q, uint64_t i) const
	{
		const rm_u64 kept = V.mkeep[i] ? 1ULL : 0ULL;
		if (q == RM_Q_KEPT) return kept;
		const pga_rc_member_t M = V.members[i];
		const int list = (q - 1) % 3;
		const rm_u64 n = list == RM_LIST_SUB ? M.n_subs : list == RM_LIST_DEL ? M.n_dels : M.n_inss;
		return q >= RM_Q_OUT_SUB ? n * kept : n;
	}
};
struct RmLetterValue { RmDev V; __host__ __device__ rm_u64 operator()(int, uint64_t i) const { return V.o_inss[i].len; } };

// ---------------------------------------------------------------- 1. which members stay, one thread per position
static __global__ __launch_bounds__(RM_THREADS) void k_remove_mark(RmDev V)
{
	for (uint64_t i = (uint64_t)blockIdx.x * RM_THREADS + threadIdx.x; i < V.n_nodes; i += (uint64_t)gridDim.x * RM_THREADS)
		if (V.keep[V.path_of[i]]) V.mkeep[V.slot_first[V.nodes[i].block] + V.nodes[i].member] = 1u;   // (block and member were checked on the host)
}

// ---------------------------------------------------------------- 2. the scans: k_ts_sums / _scan / _offsets of pga_tile_scan.h

// ---------------------------------------------------------------- 3. behind the member scan: blocks, members, nodes
// a block keeps its index and its id; without a kept member it is dead as pga_plan_simplify leaves a dead block
static __global__ __launch_bounds__(RM_THREADS) void k_remove_blocks(RmDev V)
{
	const rm_u64 *kept = ts_off(V.scan[RM_SCAN_MEMBERS], RM_Q_KEPT);
	for (uint64_t b = (uint64_t)blockIdx.x * RM_THREADS + threadIdx.x; b < V.n_blocks; b += (uint64_t)gridDim.x * RM_THREADS) {
		const pga_topo_block_t B = V.blocks[b];
		const uint32_t n = (uint32_t)(kept[V.slot_first[b + 1]] - kept[V.slot_first[b]]);
		const bool alive = B.alive && (n != 0u || B.depth == 0u);
		V.o_blocks[b] = alive ? pga_topo_block_t{B.block_id, B.cons_len, n, 1, 0} : pga_topo_block_t{B.block_id, 0u, 0u, 0, 0};
	}
}
static __global__ __launch_bounds__(RM_THREADS) void k_remove_members(RmDev V)
{
	const rm_u64 *kept = ts_off(V.scan[RM_SCAN_MEMBERS], RM_Q_KEPT);
	for (uint64_t m = (uint64_t)blockIdx.x * RM_THREADS + threadIdx.x; m < V.n_members; m += (uint64_t)gridDim.x * RM_THREADS) {
		if (V.mkeep[m]) V.o_members[kept[m]] = V.members[m];
		V.member_map[m] = V.mkeep[m] ? (long long)kept[m] : -1LL;
	}
}
// one thread per position: a node of a kept path goes to its place; its member is its rank among the kept members of its block
static __global__ __launch_bounds__(RM_THREADS) void k_remove_nodes(RmDev V)
{
	const rm_u64 *kept = ts_off(V.scan[RM_SCAN_MEMBERS], RM_Q_KEPT);
	for (uint64_t i = (uint64_t)blockIdx.x * RM_THREADS + threadIdx.x; i < V.n_nodes; i += (uint64_t)gridDim.x * RM_THREADS) {
		const uint32_t p = V.path_of[i];
		if (!V.keep[p]) continue;
		pga_topo_node_t A = V.nodes[i];
		const uint32_t first = V.slot_first[A.block];
		A.member = (uint32_t)(kept[first + A.member] - kept[first]); A.pad = 0;
		V.o_nodes[V.path_new_off[p] + (i - V.paths[p].node_off)] = A;
	}
}

// ---------------------------------------------------------------- 4. the three lists, one thread per element of the output
template <int LIST> __device__ inline void rm_copy_one(const RmDev &V, rm_u64 j, rm_u64 src);
template <> __device__ inline void rm_copy_one<RM_LIST_SUB>(const RmDev &V, rm_u64 j, rm_u64 src) { V.o_subs[j] = V.subs[src]; }
template <> __device__ inline void rm_copy_one<RM_LIST_DEL>(const RmDev &V, rm_u64 j, rm_u64 src) { V.o_dels[j] = V.dels[src]; }
template <> __device__ inline void rm_copy_one<RM_LIST_INS>(const RmDev &V, rm_u64 j, rm_u64 src)
{
	const pga_ins_t I = V.inss[src];
	if ((V.flags & PGA_REMOVE_COMPACT_LETTERS) && I.len) {                     // (the letters are read only behind this check)
		if (!V.ins_seq) atomicMin(&V.err[RM_E_INS_NULL], j);
		else if (I.seq_off > V.ins_seq_len || I.len > V.ins_seq_len - I.seq_off) atomicMin(&V.err[RM_E_INS_RANGE], j);
	}
	V.o_inss[j] = I;
}
template <int LIST> static __global__ __launch_bounds__(RM_THREADS) void k_remove_copy(RmDev V)
{
	__shared__ rm_u64 s_rng[2];
	const RmScan S = V.scan[RM_SCAN_MEMBERS];
	const rm_u64 *in = ts_off(S, RM_Q_IN_SUB + LIST), *out = ts_off(S, RM_Q_OUT_SUB + LIST);
	const rm_u64 n = out[S.n], n_tiles = (n + RM_TILE - 1) / RM_TILE;
	for (rm_u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const rm_u64 j0 = t * RM_TILE, j1 = j0 + RM_TILE < n ? j0 + RM_TILE : n;
		if (threadIdx.x < 2) s_rng[threadIdx.x] = ts_last_le(out, 0, S.n, threadIdx.x ? j1 - 1 : j0);
		__syncthreads();
		const rm_u64 lo = s_rng[0], hi = s_rng[1] + 1;
		for (rm_u64 j = j0 + threadIdx.x; j < j1; j += RM_THREADS) {
			const rm_u64 m = ts_last_le(out, lo, hi, j);
			rm_copy_one<LIST>(V, j, in[m] + (j - out[m]));
		}
		__syncthreads();
	}
}

// ---------------------------------------------------------------- 5. PGA_REMOVE_COMPACT_LETTERS, behind the letter scan and the checks of rm_copy_one
// one thread per letter of the output; the insertion of a letter is found as the member of a list element is
static __global__ __launch_bounds__(RM_THREADS) void k_remove_letters(RmDev V)
{
	__shared__ rm_u64 s_rng[2];
	const RmScan S = V.scan[RM_SCAN_LETTERS];
	const rm_u64 *out = ts_off(S, 0);
	const rm_u64 n = out[S.n], n_tiles = (n + RM_TILE - 1) / RM_TILE;
	for (rm_u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const rm_u64 j0 = t * RM_TILE, j1 = j0 + RM_TILE < n ? j0 + RM_TILE : n;
		if (threadIdx.x < 2) s_rng[threadIdx.x] = ts_last_le(out, 0, S.n, threadIdx.x ? j1 - 1 : j0);
		__syncthreads();
		const rm_u64 lo = s_rng[0], hi = s_rng[1] + 1;
		for (rm_u64 j = j0 + threadIdx.x; j < j1; j += RM_THREADS) {
			const rm_u64 k = ts_last_le(out, lo, hi, j);
			V.o_ins_seq[j] = V.ins_seq[V.o_inss[k].seq_off + (j - out[k])];
		}
		__syncthreads();
	}
}
// behind the gather: seq_off becomes the running sum of len
static __global__ __launch_bounds__(RM_THREADS) void k_remove_seq_off(RmDev V)
{
	const RmScan S = V.scan[RM_SCAN_LETTERS];
	const rm_u64 *out = ts_off(S, 0);
	for (rm_u64 k = (rm_u64)blockIdx.x * RM_THREADS + threadIdx.x; k < S.n; k += (rm_u64)gridDim.x * RM_THREADS) V.o_inss[k].seq_off = out[k];
}

// ---------------------------------------------------------------- host side: everything that is refused before a launch, and the tables
struct RmTables {
	TpTables T;
	std::vector<rm_u64> path_new_off;            // per path
	std::vector<int32_t> path_map;               // per path: its place after or -1
	std::vector<pga_topo_path_t> o_paths;
	uint64_t n_members = 0, n_subs = 0, n_dels = 0, n_inss = 0, n_out_nodes = 0;
};
inline void rm_fail(const std::string &what) { throw std::runtime_error("pga_remove_paths: " + what); }

static void rm_validate(int64_t n_blocks, const pga_topo_block_t *blocks, int64_t n_paths, const pga_topo_path_t *paths, int64_t n_nodes, const pga_topo_node_t *nodes,
                        const pga_rc_block_t *rc_blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss,
                        const uint8_t *keep, uint32_t flags, RmTables &R)
{
	try { tp_validate(n_blocks, blocks, n_paths, paths, n_nodes, nodes, 0, nullptr, 0, R.T); }
	catch (std::runtime_error &e) { const std::string w = e.what(); const size_t at = w.find(": "); rm_fail(at == std::string::npos ? w : w.substr(at + 2)); }
	if (flags & ~PGA_REMOVE_COMPACT_LETTERS) rm_fail("unknown flag");
	if (n_paths && !keep) rm_fail("null keep with paths present");
	if (n_blocks && !rc_blocks) rm_fail("null argument or negative count");
	for (int64_t b = 0; b < n_blocks; ++b)
		if (rc_blocks[b].n_members != R.T.depth[b]) rm_fail(std::string(blocks[b].alive ? "n_members of a block differs from its depth" : "a dead block with members") + " (block " + std::to_string(b) + ")");
	R.n_members = R.T.n_slots;
	if (R.n_members && !members) rm_fail("null argument or negative count");
	const uint64_t lim = 1ULL << 63;
	for (uint64_t m = 0; m < R.n_members; ++m) {
		R.n_subs += members[m].n_subs; R.n_dels += members[m].n_dels; R.n_inss += members[m].n_inss;
		if (R.n_subs >= lim || R.n_dels >= lim || R.n_inss >= lim) rm_fail("the edit counts overflow 2^63");
	}
	if ((R.n_subs && !subs) || (R.n_dels && !dels) || (R.n_inss && !inss)) rm_fail("null argument or negative count");
	if (n_paths == 0 && R.n_members) rm_fail("a (block, member) slot is named by no node (slot 0)");   // (no node at all: no launch to find it)
	R.path_new_off.assign((size_t)n_paths, 0); R.path_map.assign((size_t)n_paths, -1);
	for (int64_t p = 0; p < n_paths; ++p) {
		R.path_new_off[p] = R.n_out_nodes;
		if (!keep[p]) continue;
		R.path_map[p] = (int32_t)R.o_paths.size();
		R.o_paths.push_back(pga_topo_path_t{paths[p].path_id, R.n_out_nodes, paths[p].n_nodes, paths[p].circular});
		R.n_out_nodes += paths[p].n_nodes;
	}
}

// what the device found before the first wait
static void rm_report(const uint32_t *topo_err)
{
	if (topo_err[TP_E_DEPTH] != TP_NONE) rm_fail("the nodes of a block do not sum to its depth (block " + std::to_string(topo_err[TP_E_DEPTH]) + ")");
	if (topo_err[TP_E_SLOT] != TP_NONE) rm_fail(std::string("a (block, member) slot is named by ") + ((topo_err[TP_E_SLOT] & 1u) ? "two nodes" : "no node") + " (slot " + std::to_string(topo_err[TP_E_SLOT] >> 1) + ")");
}
static void rm_report_letters(const rm_u64 *err)
{
	if (err[RM_E_INS_NULL] != RM_NONE) rm_fail("null insertion letters while a kept insertion has some (insertion " + std::to_string(err[RM_E_INS_NULL]) + " of the output)");
	if (err[RM_E_INS_RANGE] != RM_NONE) rm_fail("seq_off + len of a kept insertion lies beyond ins_seq_len (insertion " + std::to_string(err[RM_E_INS_RANGE]) + " of the output)");
}

} // namespace pga
