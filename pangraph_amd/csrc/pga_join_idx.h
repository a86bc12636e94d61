// pga_join_idx.h -- the kernels and host tables of pga_join.hip (graph_join, graph_merging.rs:74-93: the union of the blocks, paths and
// nodes of the child graphs at an internal node of the guide tree, a panic "Conflicting key" on a shared id).
// No wave intrinsic, atomicAdd / atomicMin only: all of this compiles under hipcc and, with dev/emu/hip_emu.h included first, under
// g++ -std=c++17 -DPGA_EMU (tests/emu/join_emu.cpp runs it against a direct scalar construction).
// The scans are the tile scan of pga_tile_scan.h; the list copies, the letter gather and their value functors are pga_assemble_idx.h's
// (k_assemble_copy, k_assemble_letters, k_assemble_seq_off over an AsDev): this header only fills the descriptors they read, all of them
// with the source AS_SRC_BEFORE (the parts' arrays, behind each other).
//
// The PARTS lie behind each other in every device buffer: part p's blocks at blk_off[p], its paths at path_off[p], its nodes at node_off[p],
// its members (and who) at mem_off[p], its insertions at ins_off[p], its letters at let_off[p].  A CONCATENATED index is an index into such a
// buffer; inside the records every index is still the part's own (a node's block, a path's node_off, an insertion's seq_off).  The lists of
// a part are dense in its member order, so the BEFORE scan over all members gives a member's first elements in the concatenated lists.
// The ORDER comes from three sorts (rocPRIM on the device, std::stable_sort under the emulation): the alive block ids with their
// concatenated index, the path ids with theirs, the node ids alone.  An entry's index after is its sorted position -- a permutation of
// the entries after whatever the ids are, so a duplicate id is reported (equal neighbours) and nothing is written twice.
// An INSERTION's range is held against its own part's letters before it is rebased (k_join_ins): the gather never reads another part's.
#pragma once
#include "pga_assemble_idx.h"

namespace pga {

typedef as_u64 jn_u64;
constexpr int JN_THREADS = TS_THREADS, JN_TILE = TS_TILE;
enum { JN_SCAN_BEFORE = 0, JN_SCAN_BLOCKS = 1, JN_SCAN_PATHS = 2, JN_SCANS = 3 };
// err[]: the lowest offender (block id; path id; node id; concatenated slot << 1 | named twice; concatenated insertion).  An id may be
// all-ones, so hit[] says whether an entry of err[] was written at all
enum { JN_E_BLOCK = 0, JN_E_PATH = 1, JN_E_NODE = 2, JN_E_SLOT = 3, JN_E_SEQ = 4, JN_ERRS = 5 };
constexpr jn_u64 JN_NONE = ~0ULL;

struct JnDev {
	AsDev A;                                                           // descriptors, output lists, letters: the copies of pga_assemble_idx.h
	uint64_t n_parts, n_blocks, n_paths, n_nodes, n_members, n_alive, n_inss;   // concatenated counts; n_alive blocks, n_paths, n_nodes, n_members after
	const jn_u64 *blk_off, *path_off, *node_off, *mem_off, *ins_off, *let_off;   // n_parts + 1 entries each
	const pga_topo_block_t *blocks; const pga_topo_path_t *paths; const pga_topo_node_t *nodes;
	const uint32_t *first_member;                                      // per concatenated block (n_blocks + 1): its first concatenated member
	const pga_detach_member_t *who;                                    // per concatenated member
	pga_ins_t *inss;                                                   // the concatenated insertions (A.inss): seq_off is rebased in place
	jn_u64 *path_id, *node_id; uint32_t *path_idx;                     // the keys of the path and node sorts, written by k_join_keys
	const jn_u64 *s_block_id; const uint32_t *s_block;                 // the alive block ids ascending, the concatenated block behind each
	const jn_u64 *s_path_id; const uint32_t *s_path;                   // the path ids ascending, the concatenated path behind each
	const jn_u64 *s_node_id;                                           // the node ids ascending
	RmScan scan[JN_SCANS];
	pga_topo_block_t *o_blocks; uint32_t *o_src;                       // per block after; o_src: its concatenated block
	pga_topo_path_t *o_paths; pga_topo_node_t *o_nodes;
	uint32_t *block_map, *path_map;                                    // per concatenated block / path (all-ones before)
	pga_detach_member_t *o_who; int32_t *o_part;                       // per member after
	uint32_t *slot_cnt;                                                // per concatenated member (zeroed before)
	jn_u64 *err; uint32_t *hit;                                        // JN_ERRS words each (all-ones / zeroed before)
};

// what the scans sum: the depths of the blocks after, the node counts of the paths after
struct JnDepthValue { JnDev V; __host__ __device__ jn_u64 operator()(int, uint64_t i) const { return V.o_blocks[i].depth; } };
struct JnPathValue { JnDev V; __host__ __device__ jn_u64 operator()(int, uint64_t i) const { return V.o_paths[i].n_nodes; } };

__device__ inline void jn_report(const JnDev &V, int e, jn_u64 what) { atomicMin(&V.err[e], what); atomicAdd(&V.hit[e], 1u); }

// ---------------------------------------------------------------- 1. the sort keys of the paths and the nodes, one thread per entry
static __global__ __launch_bounds__(JN_THREADS) void k_join_keys(JnDev V)
{
	const jn_u64 n = V.n_paths > V.n_nodes ? V.n_paths : V.n_nodes;
	for (jn_u64 x = (jn_u64)blockIdx.x * JN_THREADS + threadIdx.x; x < n; x += (jn_u64)gridDim.x * JN_THREADS) {
		if (x < V.n_paths) { V.path_id[x] = V.paths[x].path_id; V.path_idx[x] = (uint32_t)x; }
		if (x < V.n_nodes) V.node_id[x] = V.nodes[x].node_id;
	}
}

// ---------------------------------------------------------------- 2. an insertion inside its own part's letters, then rebased
// An insertion that fails keeps an offset that k_assemble_copy refuses as well: no letter is read through it.
static __global__ __launch_bounds__(JN_THREADS) void k_join_ins(JnDev V)
{
	for (jn_u64 j = (jn_u64)blockIdx.x * JN_THREADS + threadIdx.x; j < V.n_inss; j += (jn_u64)gridDim.x * JN_THREADS) {
		const jn_u64 p = ts_last_le(V.ins_off, 0, V.n_parts, j);
		pga_ins_t I = V.inss[j];
		if (I.len && !as_inside(I.seq_off, I.len, V.let_off[p + 1] - V.let_off[p])) { jn_report(V, JN_E_SEQ, j); I.seq_off = JN_NONE; }
		else I.seq_off = I.len ? I.seq_off + V.let_off[p] : 0;
		V.inss[j] = I;
	}
}

// ---------------------------------------------------------------- 3. behind the sorts: the tables after, the maps, equal neighbours
// x runs over the alive blocks, the paths and the nodes in id order
static __global__ __launch_bounds__(JN_THREADS) void k_join_rank(JnDev V)
{
	jn_u64 n = V.n_alive > V.n_paths ? V.n_alive : V.n_paths;
	if (V.n_nodes > n) n = V.n_nodes;
	for (jn_u64 x = (jn_u64)blockIdx.x * JN_THREADS + threadIdx.x; x < n; x += (jn_u64)gridDim.x * JN_THREADS) {
		if (x < V.n_alive) {
			const uint32_t b = V.s_block[x];
			const pga_topo_block_t B = V.blocks[b];
			if (x && V.s_block_id[x - 1] == V.s_block_id[x]) jn_report(V, JN_E_BLOCK, V.s_block_id[x]);
			V.o_blocks[x] = pga_topo_block_t{B.block_id, B.cons_len, B.depth, 1, 0};
			V.o_src[x] = b; V.block_map[b] = (uint32_t)x;
		}
		if (x < V.n_paths) {
			const uint32_t p = V.s_path[x];
			const pga_topo_path_t P = V.paths[p];
			if (x && V.s_path_id[x - 1] == V.s_path_id[x]) jn_report(V, JN_E_PATH, V.s_path_id[x]);
			V.o_paths[x] = pga_topo_path_t{P.path_id, 0, P.n_nodes, P.circular};   // (node_off: behind the PATHS scan)
			V.path_map[p] = (uint32_t)x;
		}
		if (x && x < V.n_nodes && V.s_node_id[x - 1] == V.s_node_id[x]) jn_report(V, JN_E_NODE, V.s_node_id[x]);
	}
}

// ---------------------------------------------------------------- 4. behind the BLOCKS and BEFORE scans: one thread per member after
static __global__ __launch_bounds__(JN_THREADS) void k_join_desc(JnDev V)
{
	const jn_u64 *first = ts_off(V.scan[JN_SCAN_BLOCKS], 0);
	const RmScan SB = V.scan[JN_SCAN_BEFORE];
	for (jn_u64 m = (jn_u64)blockIdx.x * JN_THREADS + threadIdx.x; m < V.n_members; m += (jn_u64)gridDim.x * JN_THREADS) {
		const jn_u64 i = ts_last_le(first, 0, V.n_alive, m), g = V.first_member[V.o_src[i]] + (m - first[i]);
		const jn_u64 p = ts_last_le(V.mem_off, 0, V.n_parts, g);
		const pga_rc_member_t M = V.A.members[g];
		AsDesc D = {{0, 0, 0}, {M.n_subs, M.n_dels, M.n_inss}, AS_SRC_BEFORE};
		for (int q = 0; q < 3; ++q) D.off[q] = ts_off(SB, q)[g];
		V.A.desc[m] = D; V.A.o_members[m] = M;
		V.A.origin[m] = (long long)(g - V.mem_off[p]); V.o_part[m] = (int32_t)p;
		const pga_detach_member_t W = V.who[g];
		V.o_who[m] = pga_detach_member_t{W.node_id, W.reverse ? 1 : 0, 0};
	}
}

// ---------------------------------------------------------------- 5. behind the PATHS scan: one thread per node, and per path its node_off
// (a node's block and member were checked on the host against its own part)
static __global__ __launch_bounds__(JN_THREADS) void k_join_nodes(JnDev V)
{
	const jn_u64 *at = ts_off(V.scan[JN_SCAN_PATHS], 0);
	const jn_u64 n = V.n_paths > V.n_nodes ? V.n_paths : V.n_nodes;
	for (jn_u64 x = (jn_u64)blockIdx.x * JN_THREADS + threadIdx.x; x < n; x += (jn_u64)gridDim.x * JN_THREADS) {
		if (x < V.n_paths) V.o_paths[x].node_off = at[x];
		if (x >= V.n_nodes) continue;
		const jn_u64 p = ts_last_le(V.node_off, 0, V.n_parts, x), i = x - V.node_off[p];   // part, position inside the part
		const jn_u64 path = V.path_off[p] + tp_path_of(V.paths + V.path_off[p], V.path_off[p + 1] - V.path_off[p], i);
		pga_topo_node_t N = V.nodes[x];
		const jn_u64 b = V.blk_off[p] + N.block;
		atomicAdd(&V.slot_cnt[V.first_member[b] + N.member], 1u);
		N.block = V.block_map[b]; N.pad = 0;
		V.o_nodes[at[V.path_map[path]] + (i - V.paths[path].node_off)] = N;
	}
}
// one thread per concatenated member: a slot named by no node or by two
static __global__ __launch_bounds__(JN_THREADS) void k_join_check(JnDev V)
{
	for (jn_u64 g = (jn_u64)blockIdx.x * JN_THREADS + threadIdx.x; g < V.n_members; g += (jn_u64)gridDim.x * JN_THREADS)
		if (V.slot_cnt[g] != 1u) jn_report(V, JN_E_SLOT, g << 1 | (V.slot_cnt[g] ? 1u : 0u));
}

// ---------------------------------------------------------------- host side: everything that is refused before a launch, and the tables
struct JnTables {
	std::vector<jn_u64> blk_off, path_off, node_off, mem_off, ins_off, let_off, list_off[2];   // n_parts + 1 each (list_off: subs, dels)
	std::vector<uint32_t> first_member;                                // per concatenated block, one more
	std::vector<jn_u64> alive_id; std::vector<uint32_t> alive_block;   // the alive blocks in concatenated order
};
inline void jn_fail(const std::string &what) { throw std::runtime_error("pga_join_graphs: " + what); }
inline void jn_fail(int64_t part, const std::string &what) { jn_fail("part " + std::to_string(part) + ": " + what); }

static void jn_validate(int32_t n_parts, const pga_join_part_t *parts, uint32_t flags, JnTables &J)
{
	const char *null = "null argument or negative count";
	const uint64_t lim = 1ULL << 63, lim31 = 1ULL << 31;
	if (flags & ~PGA_JOIN_COPY_CONSENSUS) jn_fail("unknown flag");
	if (n_parts < 1) jn_fail("n_parts < 1");
	if (!parts) jn_fail(null);
	const size_t np1 = (size_t)n_parts + 1;
	for (auto *v : {&J.blk_off, &J.path_off, &J.node_off, &J.mem_off, &J.ins_off, &J.let_off, &J.list_off[0], &J.list_off[1]}) v->assign(np1, 0);
	J.first_member.assign(1, 0);
	for (int32_t p = 0; p < n_parts; ++p) {
		const pga_join_part_t &P = parts[p];
		TpTables T;
		try { tp_validate(P.n_blocks, P.blocks, P.n_paths, P.paths, P.n_nodes, P.nodes, 0, nullptr, 0, T); }
		catch (std::runtime_error &e) { const std::string w = e.what(); const size_t at = w.find(": "); jn_fail(p, at == std::string::npos ? w : w.substr(at + 2)); }
		if (P.n_blocks && !P.rc_blocks) jn_fail(p, null);
		for (int64_t b = 0; b < P.n_blocks; ++b) {
			if (P.rc_blocks[b].n_members != T.depth[b]) jn_fail(p, std::string(P.blocks[b].alive ? "n_members of a block differs from its depth" : "a dead block with members") + " (block " + std::to_string(b) + ")");
			if (P.blocks[b].alive && P.rc_blocks[b].cons_len != P.blocks[b].cons_len) jn_fail(p, "cons_len of a block differs between the graph and the block arrays (block " + std::to_string(b) + ")");
			if (P.blocks[b].alive && P.blocks[b].cons_len && !P.rc_blocks[b].consensus) jn_fail(p, "null consensus of a block with letters (block " + std::to_string(b) + ")");
			if (P.blocks[b].alive) { J.alive_id.push_back(P.blocks[b].block_id); J.alive_block.push_back((uint32_t)(J.blk_off[p] + (uint64_t)b)); }
			J.first_member.push_back((uint32_t)(J.mem_off[p] + T.slot_first[b + 1]));
		}
		if (T.n_slots && (!P.members || !P.who)) jn_fail(p, null);
		uint64_t tot[3] = {0, 0, 0};
		for (uint64_t m = 0; m < T.n_slots; ++m) {
			tot[0] += P.members[m].n_subs; tot[1] += P.members[m].n_dels; tot[2] += P.members[m].n_inss;
			if (J.list_off[0][p] + tot[0] >= lim || J.list_off[1][p] + tot[1] >= lim || J.ins_off[p] + tot[2] >= lim) jn_fail(p, "the edit counts overflow 2^63");
		}
		if ((tot[0] && !P.subs) || (tot[1] && !P.dels) || (tot[2] && !P.inss)) jn_fail(p, null);
		const uint64_t n_let = P.ins_seq ? P.ins_seq_len : 0;              // (a NULL buffer holds no letter: an insertion with letters is refused by its range)
		if (J.let_off[p] + n_let >= lim || J.let_off[p] + n_let < n_let) jn_fail(p, "the letter counts overflow 2^63");
		J.blk_off[p + 1] = J.blk_off[p] + (uint64_t)P.n_blocks; J.path_off[p + 1] = J.path_off[p] + (uint64_t)P.n_paths; J.node_off[p + 1] = J.node_off[p] + (uint64_t)P.n_nodes;
		J.mem_off[p + 1] = J.mem_off[p] + T.n_slots; J.list_off[0][p + 1] = J.list_off[0][p] + tot[0]; J.list_off[1][p + 1] = J.list_off[1][p] + tot[1];
		J.ins_off[p + 1] = J.ins_off[p] + tot[2]; J.let_off[p + 1] = J.let_off[p] + n_let;
		if (J.blk_off[p + 1] >= lim31 || J.mem_off[p + 1] >= lim31 || J.node_off[p + 1] >= lim31 || J.path_off[p + 1] >= lim31)
			jn_fail(p, "2^31 or more blocks, members, nodes or paths after");
	}
}

// which parts hold an id (the first two, in part order): for the message of a conflict
template <class Has> static std::string jn_parts_with(int32_t n_parts, Has has)
{
	std::string s;
	int found = 0;
	for (int32_t p = 0; p < n_parts && found < 2; ++p) for (int k = has(p); k > 0 && found < 2; --k) s += (found++ ? " and " : "") + std::to_string(p);
	return s;
}
// what the device found before the first wait, lowest offender each
static void jn_report_host(int32_t n_parts, const pga_join_part_t *parts, const jn_u64 *err, const uint32_t *hit, const JnTables &J)
{
	auto at = [](jn_u64 x) { return std::to_string(x); };
	if (hit[JN_E_BLOCK]) {
		const jn_u64 id = err[JN_E_BLOCK];
		jn_fail("Conflicting key: block id " + at(id) + " is present twice (parts " + jn_parts_with(n_parts, [&](int32_t p) {
			int k = 0; for (int64_t b = 0; b < parts[p].n_blocks; ++b) k += parts[p].blocks[b].alive && parts[p].blocks[b].block_id == id; return k; }) + ")");
	}
	if (hit[JN_E_PATH]) {
		const jn_u64 id = err[JN_E_PATH];
		jn_fail("Conflicting key: path id " + at(id) + " is present twice (parts " + jn_parts_with(n_parts, [&](int32_t p) {
			int k = 0; for (int64_t i = 0; i < parts[p].n_paths; ++i) k += parts[p].paths[i].path_id == id; return k; }) + ")");
	}
	if (hit[JN_E_NODE]) {
		const jn_u64 id = err[JN_E_NODE];
		jn_fail("Conflicting key: node id " + at(id) + " is present twice (parts " + jn_parts_with(n_parts, [&](int32_t p) {
			int k = 0; for (int64_t i = 0; i < parts[p].n_nodes && k < 2; ++i) k += parts[p].nodes[i].node_id == id; return k; }) + ")");
	}
	if (hit[JN_E_SLOT]) {
		const jn_u64 g = err[JN_E_SLOT] >> 1, p = ts_last_le(J.mem_off.data(), 0, (jn_u64)n_parts, g);
		jn_fail((int64_t)p, std::string("a (block, member) slot is named by ") + ((err[JN_E_SLOT] & 1u) ? "two nodes" : "no node") + " (slot " + at(g - J.mem_off[p]) + ")");
	}
	if (hit[JN_E_SEQ]) {
		const jn_u64 j = err[JN_E_SEQ], p = ts_last_le(J.ins_off.data(), 0, (jn_u64)n_parts, j);
		jn_fail((int64_t)p, "seq_off + len of an insertion lies beyond its part's letter buffer (insertion " + at(j - J.ins_off[p]) + ")");
	}
}

} // namespace pga
