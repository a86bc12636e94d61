// pga_apply_idx.h -- the kernels and host tables of pga_apply.hip (the graph update of a merge: split_block's n_new / b_new, reweave.rs:359-401,
// Pangraph::update, pangraph.rs:68-107, applied block after block, reweave.rs:445-450, and the insertion of the merged blocks,
// graph_merging.rs:156-165).  No wave intrinsic, atomicAdd / atomicMin only: all of this compiles under hipcc and, with dev/emu/hip_emu.h
// included first, under g++ -std=c++17 -DPGA_EMU (tests/emu/apply_emu.cpp runs it against a direct scalar construction).
// The path lookup, the node hash and the tiled splice (its workgroup scan: pga_tile_scan.h) are pga_topo_idx.h's; the sorts and scans are
// rocPRIM's (pga_apply.hip).
//
// A MEMBER here is a kept slice member, index k into slice.members[]; its SLOT is (cut block, member) of the graph, named by one position.
// The MATRIX has one word per (cut block, member, interval of that block), rows of n_intervals words, cut after cut: a kept member counts
// into its word, so the exclusive sums of the matrix number the new nodes by (block, member, interval) -- the order in which they replace
// the old nodes of forward strand; a row's sum is the count of its slot, a reverse old node mirrors the order inside its row at scatter.
// An ENTRY is a block that the call makes: one per unaligned interval, one per aligned pair (anchor, append).  Its RANK is its place among
// the entries by ascending id (unsigned); its index in the table after is rank + the survivors of smaller id, a survivor's its rank among
// the survivors + the entries of smaller id.
#pragma once
#include "pga_topo_idx.h"

namespace pga {

enum { AP_E_MEMBER = 0, AP_E_TWICE = 1, AP_E_NEWDUP = 2, AP_E_CONFLICT = 3, AP_E_NODEDUP = 4, AP_ERRS = 5 };   // err[]: the lowest offender (member, member, rank, rank, place)

struct ApEntry { tp_u64 block_id; uint32_t ia, ib; int32_t kind; uint32_t pad; };     // ia: the unaligned or the anchor interval; ib: the append interval
struct ApDev {
	uint64_t n_nodes, n_paths, n_blocks, n_intervals, n_members, n_mat, n_entries, n_surv;
	const pga_topo_node_t *nodes; const pga_topo_path_t *paths; const pga_topo_block_t *blocks;
	const uint32_t *depth, *slot_first, *path_of;          // as in TpDev (path_of: behind k_topo_keys)
	const uint32_t *cut_of;                                // per block: its cut or TP_NONE
	const pga_apply_cut_t *cut; const uint32_t *mat_off;   // per cut: where its rows start
	const uint32_t *iv_cut, *iv_entry;                     // per interval
	const pga_plan_interval_t *intervals; const pga_slice_res_t *slices; const pga_slice_member_t *members;
	uint32_t *slot_pos;                                    // per slot: its position (zeroed before)
	uint32_t *mat; const uint32_t *mat_scan;               // n_mat + 1 words each
	uint32_t *m_slice, *m_ent;                             // per member: its slice; its matrix word or TP_NONE
	pga_topo_node_t *o_new; uint64_t *o_old; tp_u64 *node_key;   // per member
	uint32_t *err;                                         // AP_ERRS words, all-ones = none
	// the block table
	const ApEntry *entries; const tp_u64 *sorted_ids; const uint32_t *sorted_entry;   // the entries' ids sorted, with the entry of each
	const tp_u64 *surv_ids; const uint32_t *surv_rank;     // the survivors' ids in index order; per block its rank among them
	uint32_t *entry_rank, *rank_index, *rank_depth; const uint32_t *rank_moff;   // rank_depth, rank_moff: n_entries + 1 words
	uint32_t *block_map; pga_topo_block_t *o_blocks; pga_apply_block_t *o_new_blocks;
	// the member slots
	const uint32_t *by_id; uint32_t *key2;                 // members by node id; the rank of each of them
	const uint32_t *key2_sorted, *by_slot;                 // both sorted by (rank, node id)
	uint64_t *member_src;
	// what the splice takes
	pga_topo_node_t *ordered, *nodes2; uint32_t *cnt, *repl;
};

// the last slice whose member_off is <= k: the one that holds member k (empty slices share their offset with the slice behind them)
__host__ __device__ inline uint32_t ap_slice_of(const pga_slice_res_t *slices, uint64_t n, uint64_t k)
{
	uint64_t lo = 0, hi = n;
	while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (slices[mid].member_off <= k) lo = mid; else hi = mid; }
	return (uint32_t)lo;
}
// how many of the n ascending ids are smaller than id
__host__ __device__ inline uint32_t ap_below(const tp_u64 *ids, uint64_t n, tp_u64 id)
{
	uint64_t lo = 0, hi = n;
	while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (ids[mid] < id) lo = mid + 1; else hi = mid; }
	return (uint32_t)lo;
}

// ---------------------------------------------------------------- 1. where every slot lies, one thread per position
static __global__ __launch_bounds__(TP_THREADS) void k_apply_slot_pos(ApDev V)
{
	for (uint64_t i = (uint64_t)blockIdx.x * TP_THREADS + threadIdx.x; i < V.n_nodes; i += (uint64_t)gridDim.x * TP_THREADS)
		V.slot_pos[V.slot_first[V.nodes[i].block] + V.nodes[i].member] = (uint32_t)i;      // (block and member were checked on the host)
}
// ---------------------------------------------------------------- 2. one thread per kept slice member: its word of the matrix, the new node
static __global__ __launch_bounds__(TP_THREADS) void k_apply_members(ApDev V)
{
	for (uint64_t k = (uint64_t)blockIdx.x * TP_THREADS + threadIdx.x; k < V.n_members; k += (uint64_t)gridDim.x * TP_THREADS) {
		const uint32_t s = ap_slice_of(V.slices, V.n_intervals, k), c = V.iv_cut[s];
		const pga_apply_cut_t C = V.cut[c];
		const pga_slice_member_t M = V.members[k];
		V.m_slice[k] = s; V.m_ent[k] = TP_NONE; V.node_key[k] = 0; V.o_old[k] = 0;
		V.o_new[k] = pga_topo_node_t{0, 0, 0, 0, 0, 0, 0};
		if (M.member >= V.depth[C.block]) { atomicMin(&V.err[AP_E_MEMBER], (uint32_t)k); continue; }
		const uint32_t e = V.mat_off[c] + M.member * C.n_intervals + (s - (uint32_t)C.first_interval);
		if (atomicAdd(&V.mat[e], 1u) != 0u) atomicMin(&V.err[AP_E_TWICE], (uint32_t)k);
		V.m_ent[k] = e;
		const uint32_t i = V.slot_pos[V.slot_first[C.block] + M.member];
		const uint64_t id = tp_node_id(V.intervals[s].new_block_id, V.paths[V.path_of[i]].path_id, M.reverse ? 1u : 0u, M.pos_start, M.pos_end);
		V.o_new[k] = pga_topo_node_t{id, M.pos_start, M.pos_end, 0, 0, M.reverse ? 1 : 0, 0};
		V.o_old[k] = V.nodes[i].node_id; V.node_key[k] = id;
	}
}
// ---------------------------------------------------------------- 3. the block table: one thread per entry in id order, one per old block
static __global__ __launch_bounds__(TP_THREADS) void k_apply_entries(ApDev V)
{
	for (uint64_t r = (uint64_t)blockIdx.x * TP_THREADS + threadIdx.x; r <= V.n_entries; r += (uint64_t)gridDim.x * TP_THREADS) {
		if (r == V.n_entries) { V.rank_depth[r] = 0; continue; }
		const tp_u64 id = V.sorted_ids[r];
		const uint32_t j = V.sorted_entry[r];
		const ApEntry E = V.entries[j];
		if (r && V.sorted_ids[r - 1] == id) atomicMin(&V.err[AP_E_NEWDUP], (uint32_t)r);
		const uint32_t below = ap_below(V.surv_ids, V.n_surv, id);
		if (below < V.n_surv && V.surv_ids[below] == id) atomicMin(&V.err[AP_E_CONFLICT], (uint32_t)r);
		const uint32_t depth = V.slices[E.ia].n_kept + (E.kind ? V.slices[E.ib].n_kept : 0u);
		V.entry_rank[j] = (uint32_t)r; V.rank_index[r] = (uint32_t)r + below; V.rank_depth[r] = depth;
		V.o_blocks[r + below] = pga_topo_block_t{id, V.intervals[E.ia].end - V.intervals[E.ia].start, depth, 1, 0};
	}
}
static __global__ __launch_bounds__(TP_THREADS) void k_apply_survivors(ApDev V)
{
	for (uint64_t b = (uint64_t)blockIdx.x * TP_THREADS + threadIdx.x; b < V.n_blocks; b += (uint64_t)gridDim.x * TP_THREADS) {
		const pga_topo_block_t B = V.blocks[b];
		uint32_t to = TP_NONE;
		if (B.alive && V.cut_of[b] == TP_NONE) {
			to = V.surv_rank[b] + ap_below(V.sorted_ids, V.n_entries, B.block_id);
			V.o_blocks[to] = pga_topo_block_t{B.block_id, B.cons_len, B.depth, 1, 0};
		}
		V.block_map[b] = to;
	}
}
// behind the scan of rank_depth[]
static __global__ __launch_bounds__(TP_THREADS) void k_apply_new_blocks(ApDev V)
{
	for (uint64_t r = (uint64_t)blockIdx.x * TP_THREADS + threadIdx.x; r < V.n_entries; r += (uint64_t)gridDim.x * TP_THREADS) {
		const ApEntry E = V.entries[V.sorted_entry[r]];
		V.o_new_blocks[r] = pga_apply_block_t{V.rank_index[r], E.kind, E.ia, E.kind ? E.ib : 0u, V.rank_moff[r]};
	}
}
// ---------------------------------------------------------------- 4. the member slots: members sorted by node id get their block's rank as the second key
static __global__ __launch_bounds__(TP_THREADS) void k_apply_key2(ApDev V)
{
	for (uint64_t x = (uint64_t)blockIdx.x * TP_THREADS + threadIdx.x; x < V.n_members; x += (uint64_t)gridDim.x * TP_THREADS)
		V.key2[x] = V.entry_rank[V.iv_entry[V.m_slice[V.by_id[x]]]];
}
// sorted by (rank, node id): place x is slot x - (the members of the ranks before)
static __global__ __launch_bounds__(TP_THREADS) void k_apply_slots(ApDev V)
{
	for (uint64_t x = (uint64_t)blockIdx.x * TP_THREADS + threadIdx.x; x < V.n_members; x += (uint64_t)gridDim.x * TP_THREADS) {
		const uint32_t k = V.by_slot[x], r = V.key2_sorted[x];
		if (x && V.key2_sorted[x - 1] == r && V.node_key[V.by_slot[x - 1]] == V.node_key[k]) atomicMin(&V.err[AP_E_NODEDUP], (uint32_t)x);
		V.member_src[x] = k;
		V.o_new[k].block = V.rank_index[r]; V.o_new[k].member = (uint32_t)x - V.rank_moff[r];
	}
}
// ---------------------------------------------------------------- 5. behind the checks and the scan of the matrix: the new nodes in path order, cnt[] / repl[]
static __global__ __launch_bounds__(TP_THREADS) void k_apply_order(ApDev V)
{
	for (uint64_t k = (uint64_t)blockIdx.x * TP_THREADS + threadIdx.x; k < V.n_members; k += (uint64_t)gridDim.x * TP_THREADS) {
		const uint32_t e = V.m_ent[k], s = V.m_slice[k];
		if (e == TP_NONE) continue;
		const pga_apply_cut_t C = V.cut[V.iv_cut[s]];
		const uint32_t row = e - (s - (uint32_t)C.first_interval), first = V.mat_scan[row], last = V.mat_scan[row + C.n_intervals], at = V.mat_scan[e];
		const bool rev = V.nodes[V.slot_pos[V.slot_first[C.block] + V.members[k].member]].reverse != 0;
		V.ordered[rev ? first + (last - 1u - at) : at] = V.o_new[k];
	}
}
static __global__ __launch_bounds__(TP_THREADS) void k_apply_positions(ApDev V)
{
	for (uint64_t i = (uint64_t)blockIdx.x * TP_THREADS + threadIdx.x; i < V.n_nodes; i += (uint64_t)gridDim.x * TP_THREADS) {
		pga_topo_node_t A = V.nodes[i];
		const uint32_t c = V.cut_of[A.block];
		uint32_t cnt = 1, repl = TP_NONE;
		if (c == TP_NONE) { A.block = V.block_map[A.block]; A.pad = 0; }
		else {
			const uint32_t row = V.mat_off[c] + A.member * V.cut[c].n_intervals;
			repl = V.mat_scan[row]; cnt = V.mat_scan[row + V.cut[c].n_intervals] - repl;
		}
		V.nodes2[i] = A; V.cnt[i] = cnt; V.repl[i] = repl;
	}
}

// ---------------------------------------------------------------- host side: everything that is refused before a launch, and the tables
struct ApTables {
	TpTables T;
	std::vector<uint32_t> cut_of, mat_off, iv_cut, iv_entry, surv_rank;
	std::vector<tp_u64> surv_ids, entry_ids;
	std::vector<ApEntry> entries;
	uint64_t n_intervals = 0, n_members = 0, n_mat = 0, n_out_nodes = 0;
};
inline void ap_fail(const std::string &what) { throw std::runtime_error("pga_apply_merge: " + what); }

static void ap_validate(int64_t n_blocks, const pga_topo_block_t *blocks, int64_t n_paths, const pga_topo_path_t *paths, int64_t n_nodes, const pga_topo_node_t *nodes,
                        int64_t n_cut, const pga_apply_cut_t *cut, const pga_plan_interval_t *intervals, const pga_slice_res_t *slices, const pga_slice_member_t *members, ApTables &A)
{
	try { tp_validate(n_blocks, blocks, n_paths, paths, n_nodes, nodes, 0, nullptr, 0, A.T); }
	catch (std::runtime_error &e) { const std::string w = e.what(); const size_t at = w.find(": "); ap_fail(at == std::string::npos ? w : w.substr(at + 2)); }
	if (n_cut < 0 || (n_cut && (!cut || !intervals || !slices))) ap_fail("null argument or negative count");
	if (n_cut >= (1LL << 31)) ap_fail("2^31 or more cut blocks");
	if (n_cut == 0) return;
	if (A.T.n_slots != (uint64_t)n_nodes) ap_fail("the nodes of the blocks do not sum to their depths");
	A.cut_of.assign((size_t)n_blocks, TP_NONE); A.mat_off.assign((size_t)n_cut + 1, 0);
	uint64_t cut_nodes = 0;
	for (int64_t c = 0; c < n_cut; ++c) {
		const pga_apply_cut_t &C = cut[c];
		const std::string who = " (cut " + std::to_string(c) + ")";
		if (C.block >= (uint64_t)n_blocks) ap_fail("a cut block is out of range" + who);
		if (!blocks[C.block].alive) ap_fail("a cut block is dead" + who);
		if (A.cut_of[C.block] != TP_NONE) ap_fail("a cut block is named twice" + who);
		if (C.n_intervals == 0) ap_fail("a cut block without intervals" + who);
		if (C.first_interval != A.n_intervals) ap_fail("first_interval is not the running sum of n_intervals" + who);
		A.cut_of[C.block] = (uint32_t)c; A.mat_off[c] = (uint32_t)A.n_mat;
		A.n_intervals += C.n_intervals; A.n_mat += (uint64_t)C.n_intervals * blocks[C.block].depth; cut_nodes += blocks[C.block].depth;
		if (A.n_intervals >= (1ULL << 31) || A.n_mat >= (1ULL << 31)) ap_fail("2^31 or more intervals, or members times intervals");
	}
	A.mat_off[n_cut] = (uint32_t)A.n_mat;
	A.iv_cut.assign((size_t)A.n_intervals, 0); A.iv_entry.assign((size_t)A.n_intervals, TP_NONE);
	struct Half { tp_u64 id; uint32_t anchor, s; };
	std::vector<Half> halves;
	for (int64_t c = 0; c < n_cut; ++c) for (uint32_t j = 0; j < cut[c].n_intervals; ++j) {
		const uint64_t s = cut[c].first_interval + j;
		const pga_plan_interval_t &I = intervals[s];
		const std::string who = " (cut " + std::to_string(c) + ", interval " + std::to_string(j) + ")";
		if (I.start >= I.end || (j && I.start < intervals[s - 1].end)) ap_fail("the intervals of a block are not ascending and disjoint" + who);
		if (slices[s].member_off != A.n_members || slices[s].n_kept > blocks[cut[c].block].depth) ap_fail("the n_kept of the slices do not match members[]" + who);
		A.n_members += slices[s].n_kept;
		A.iv_cut[s] = (uint32_t)c;
		if (I.aligned) halves.push_back(Half{I.new_block_id, I.is_anchor ? 1u : 0u, (uint32_t)s});
		else { A.iv_entry[s] = (uint32_t)A.entries.size(); A.entries.push_back(ApEntry{I.new_block_id, (uint32_t)s, 0, 0, 0}); }
	}
	if (A.n_members && !members) ap_fail("null argument or negative count");
	std::sort(halves.begin(), halves.end(), [](const Half &x, const Half &y) { return x.id != y.id ? x.id < y.id : x.anchor < y.anchor; });
	for (size_t h = 0; h < halves.size(); h += 2) {
		const bool pair = h + 1 < halves.size() && halves[h].id == halves[h + 1].id && !halves[h].anchor && halves[h + 1].anchor && (h + 2 >= halves.size() || halves[h + 2].id != halves[h].id);
		if (!pair) ap_fail("an aligned interval without its partner (interval " + std::to_string(halves[h].s) + ")");
		A.iv_entry[halves[h].s] = A.iv_entry[halves[h + 1].s] = (uint32_t)A.entries.size();
		A.entries.push_back(ApEntry{halves[h].id, halves[h + 1].s, halves[h].s, 1, 0});
	}
	for (const ApEntry &E : A.entries) A.entry_ids.push_back(E.block_id);
	A.surv_rank.assign((size_t)n_blocks, 0);
	for (int64_t b = 0; b < n_blocks; ++b) if (blocks[b].alive && A.cut_of[b] == TP_NONE) { A.surv_rank[b] = (uint32_t)A.surv_ids.size(); A.surv_ids.push_back(blocks[b].block_id); }
	A.n_out_nodes = (uint64_t)n_nodes - cut_nodes + A.n_members;
	if (A.n_out_nodes >= (1ULL << 31) || A.n_members >= (1ULL << 31) || A.surv_ids.size() + A.entries.size() >= (1ULL << 31)) ap_fail("2^31 or more nodes or blocks after");
}

// what the device found, lowest offender each
static void ap_report(const uint32_t *topo_err, const uint32_t *err)
{
	if (topo_err[TP_E_DEPTH] != TP_NONE) ap_fail("the nodes of a block do not sum to its depth (block " + std::to_string(topo_err[TP_E_DEPTH]) + ")");
	if (topo_err[TP_E_SLOT] != TP_NONE) ap_fail(std::string("a (block, member) slot is named by ") + ((topo_err[TP_E_SLOT] & 1u) ? "two nodes" : "no node") + " (slot " + std::to_string(topo_err[TP_E_SLOT] >> 1) + ")");
	if (err[AP_E_MEMBER] != TP_NONE) ap_fail("a slice member with member >= depth of its block (member " + std::to_string(err[AP_E_MEMBER]) + ")");
	if (err[AP_E_TWICE] != TP_NONE) ap_fail("a member is kept twice in one interval (member " + std::to_string(err[AP_E_TWICE]) + ")");
	if (err[AP_E_NEWDUP] != TP_NONE) ap_fail("two new blocks with the same id (Conflicting key; rank " + std::to_string(err[AP_E_NEWDUP]) + ")");
	if (err[AP_E_CONFLICT] != TP_NONE) ap_fail("a new block id equals a surviving one (Conflicting key; rank " + std::to_string(err[AP_E_CONFLICT]) + ")");
	if (err[AP_E_NODEDUP] != TP_NONE) ap_fail("two equal node ids inside one block after (place " + std::to_string(err[AP_E_NODEDUP]) + ")");
}

} // namespace pga
