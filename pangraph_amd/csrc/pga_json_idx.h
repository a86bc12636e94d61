// pga_json_idx.h -- the kernels and host tables of pga_json.hip (the pangraph JSON: serde_json::to_writer_pretty of Pangraph, written by
// build_run.rs:78 and simplify_run.rs:20, on the flat graph of pga_plan_simplify and the block arrays of pga_reconsensus).
// No wave intrinsic, plain stores and atomicMin only: all of this compiles under hipcc and, with dev/emu/hip_emu.h included first, under
// g++ -std=c++17 -DPGA_EMU (tests/emu/json_emu.cpp runs it against a direct scalar construction).  The window and the decimal
// writer are pga_gfa_idx.h's, the tile scan and the lookup in scanned offsets pga_tile_scan.h's, the path lookup and the graph checks
// pga_topo_idx.h's; the two radix sorts are rocPRIM's (pga_json.hip) and are not in here.
//
// A POSITION is an index into nodes[]; a SLOT is (block, member) numbered slot_first[block] + member: members[], and with it the edit
// lists, are in slot order.  The reference prints three BTreeMaps.  order[] holds the positions by ascending node_id (the "nodes" map);
// border[] is order[] stably sorted by block index: entry e is the e-th EMITTED MEMBER, and because every slot is named by exactly one
// position (checked before border[] is used) the emitted members of block b are e in [slot_first[b], slot_first[b + 1]).
// The file is a list of ITEMS in file order, each with a byte length:
//   0                     the opening: {\n  "paths": {
//   per path              a head (key, id, "nodes": [), one item per node id, a tail (tot_len, circular, name, desc): path p's head is
//                         path item node_off + 2 p
//   1                     the joint to "blocks"
//   per alive block k     a head (key, id, the consensus skipped by its length, "alignments": {), its emitted members, a tail: its head is
//                         block item bstart[k] = 2 k + moff[slot_first[block]]
//     per emitted member  a head (key, "subs": [), one item per sub, the joint to "dels", one per del, the joint to "inss", per insertion
//                         one item per JS_CHUNK letters (at least one; the first carries pos, the last the closing), a tail: moff[] is the
//                         64-bit scan of the members' item counts in emitted order, icoff[] that of the insertions' chunk counts in
//                         input order
//   1                     the joint to "nodes"
//   per node              one item, in order[]
//   1                     the closing
// An item number is resolved top level first, by binary search on node_off + 2 p, bstart[], moff[] and icoff[] (js_item).  js_emit()
// writes an item through a WINDOW of the file as gf_emit() does: with an empty window it gives the item's length (k_json_lens), so the
// layout and the text cannot disagree; k_json_tile writes the items that intersect a tile, one thread per item.
// Consensus letters, names and descriptions are skipped by their (escaped) lengths: the host copies them into the tile (js_host_fill).
#pragma once
#include "pga_gfa_idx.h"

namespace pga {

constexpr uint32_t JS_NULL = 0xffffffffu;                               // JsPath::name_len / desc_len of a JSON null
constexpr uint32_t JS_CHUNK = 64;                                       // letters of an insertion per item
constexpr gf_u64 JS_NONE = ~0ULL;
enum { JS_E_DUPID = 0, JS_E_ALT, JS_E_INS_RANGE, JS_E_INS_LETTER, JS_ERRS };   // err[]: the lowest offending sorted rank / sub / insertion; all-ones = none
enum { JS_K_OPEN = 0, JS_K_P_HEAD, JS_K_P_NODE, JS_K_P_TAIL, JS_K_BLOCKS, JS_K_B_HEAD, JS_K_M_HEAD, JS_K_SUB, JS_K_J_DELS, JS_K_DEL, JS_K_J_INSS, JS_K_INS,
       JS_K_M_TAIL, JS_K_B_TAIL, JS_K_NODES, JS_K_NODE, JS_K_CLOSE };

struct JsPath { uint64_t tot_len; uint32_t name_len, desc_len; };       // the escaped lengths, JS_NULL for null
struct JsDev {
	uint64_t n_nodes, n_paths, n_blocks, n_slots, n_alive, n_subs, n_dels, n_inss, n_ins_seq;
	const pga_topo_node_t *nodes; const pga_topo_path_t *paths; const pga_topo_block_t *blocks; const JsPath *meta;
	const uint32_t *slot_first, *path_of;    // per block (n_blocks + 1); per position (behind k_topo_keys)
	const pga_rc_member_t *members; const pga_sub_t *subs; const pga_del_t *dels; const pga_ins_t *inss; const char *ins_seq;
	uint32_t chunk, pad;
	// the two orders
	gf_u64 *id_key; uint32_t *pos; const gf_u64 *id_skey; const uint32_t *order;   // per position: node_id, the position; sorted by node_id
	uint32_t *blk_key; const uint32_t *border;                                      // the block of order[i]; order[] sorted stably by it
	gf_u64 *err;                             // JS_ERRS words
	// the edits, in slot (input) order
	gf_u64 *cnt_s, *cnt_d, *cnt_i; const gf_u64 *sub_off, *del_off, *ins_off;     // per slot; their scans (n_slots + 1)
	gf_u64 *chunks; const gf_u64 *icoff;     // per insertion: its items; the scan (n_inss + 1)
	// the hierarchy
	gf_u64 *mitems; const gf_u64 *moff;      // per emitted member: its items; the scan (n_slots + 1)
	const uint32_t *ablk; gf_u64 *bstart;    // per alive block: its index; its first block item (n_alive + 1, the last: all block items)
	// the layout
	uint64_t n_pitems, n_bitems, n_items;
	gf_u64 *len; const gf_u64 *off;          // per item; off: n_items + 1 entries
	gf_u64 *path_off, *tail_off, *block_off; // per path: where its key and its tail item start; per block: its key (all-ones before)
	// the tile
	char *tile; gf_u64 t0, t1;
};

__host__ __device__ inline gf_u64 js_chunks(uint32_t len, uint32_t chunk) { return len ? ((gf_u64)len + chunk - 1) / chunk : 1ULL; }
__host__ __device__ inline bool js_plain(uint32_t c) { return c >= 0x20u && c <= 0x7eu && c != (uint32_t)'"' && c != (uint32_t)'\\'; }
#define JS_LIT(O, s) gf_puts(O, s, (uint32_t)sizeof(s) - 1u)

// ---------------------------------------------------------------- the pieces the host measures too (through an empty window)
// a block's head up to the opening quote of its consensus
__host__ __device__ inline void js_block_head(GfOut &O, bool first, gf_u64 id)
{
	if (!first) gf_put(O, ',');
	JS_LIT(O, "\n    \""); gf_dec(O, id); JS_LIT(O, "\": {\n      \"id\": "); gf_dec(O, id); JS_LIT(O, ",\n      \"consensus\": \"");
}
// a path's tail up to the value of "name"
__host__ __device__ inline void js_path_tail(GfOut &O, bool any_node, gf_u64 tot_len, bool circular)
{
	if (any_node) JS_LIT(O, "\n      ]"); else gf_put(O, ']');
	JS_LIT(O, ",\n      \"tot_len\": "); gf_dec(O, tot_len); JS_LIT(O, ",\n      \"circular\": ");
	if (circular) JS_LIT(O, "true"); else JS_LIT(O, "false");
	JS_LIT(O, ",\n      \"name\": ");
}
__host__ __device__ inline void js_string_or_null(GfOut &O, uint32_t len)   // (the bytes are the host's)
{
	if (len == JS_NULL) { JS_LIT(O, "null"); return; }
	gf_put(O, '"'); O.at += len; gf_put(O, '"');
}
#define JS_DESC_KEY ",\n      \"desc\": "
// the closing of a map or a list: on a line of its own unless it is empty
__host__ __device__ inline void js_close(GfOut &O, bool any, const char *full, uint32_t n, char c) { if (any) gf_puts(O, full, n); else gf_put(O, c); }

// ---------------------------------------------------------------- an item number -> what it is
// (js_item and js_emit are force-inlined: out of line they take the kernel's by-value argument by reference, which puts it into scratch)
struct JsItem { int kind; bool first; uint32_t c; gf_u64 a; };         // a: the path, position, block, emitted member, edit or sorted rank; c: the chunk
__host__ __device__ __forceinline__ JsItem js_item(const JsDev &V, gf_u64 x)
{
	if (x == 0) return JsItem{JS_K_OPEN, false, 0, 0};
	x -= 1;
	if (x < V.n_pitems) {
		gf_u64 lo = 0, hi = V.n_paths;                                       // paths[lo].node_off + 2 lo <= x < the same of hi
		while (hi - lo > 1) { const gf_u64 mid = (lo + hi) >> 1; if (V.paths[mid].node_off + 2 * mid <= x) lo = mid; else hi = mid; }
		const pga_topo_path_t P = V.paths[lo];
		const gf_u64 j = x - (P.node_off + 2 * lo);
		if (j == 0) return JsItem{JS_K_P_HEAD, lo == 0, 0, lo};
		if (j == (gf_u64)P.n_nodes + 1) return JsItem{JS_K_P_TAIL, P.n_nodes == 0, 0, lo};
		return JsItem{JS_K_P_NODE, j == 1, 0, P.node_off + j - 1};
	}
	x -= V.n_pitems;
	if (x == 0) return JsItem{JS_K_BLOCKS, V.n_paths == 0, 0, 0};
	x -= 1;
	if (x < V.n_bitems) {
		const gf_u64 k = ts_last_le(V.bstart, 0, V.n_alive, x);
		const uint32_t b = V.ablk[k];
		const gf_u64 e0 = V.slot_first[b], e1 = V.slot_first[b + 1], j = x - V.bstart[k];
		if (j == 0) return JsItem{JS_K_B_HEAD, k == 0, 0, b};
		if (j == 1 + (V.moff[e1] - V.moff[e0])) return JsItem{JS_K_B_TAIL, e0 == e1, 0, b};
		const gf_u64 y = V.moff[e0] + j - 1, e = ts_last_le(V.moff, e0, e1, y);
		gf_u64 r = y - V.moff[e];
		if (r == 0) return JsItem{JS_K_M_HEAD, e == e0, 0, e};
		const pga_topo_node_t N = V.nodes[V.border[e]];
		const gf_u64 s = (gf_u64)V.slot_first[N.block] + N.member;
		const pga_rc_member_t M = V.members[s];
		r -= 1;
		if (r < M.n_subs) return JsItem{JS_K_SUB, r == 0, 0, V.sub_off[s] + r};
		r -= M.n_subs;
		if (r == 0) return JsItem{JS_K_J_DELS, M.n_subs == 0, 0, 0};
		r -= 1;
		if (r < M.n_dels) return JsItem{JS_K_DEL, r == 0, 0, V.del_off[s] + r};
		r -= M.n_dels;
		if (r == 0) return JsItem{JS_K_J_INSS, M.n_dels == 0, 0, 0};
		r -= 1;
		const gf_u64 i0 = V.ins_off[s], i1 = i0 + M.n_inss;
		if (r < V.icoff[i1] - V.icoff[i0]) {
			const gf_u64 i = ts_last_le(V.icoff, i0, i1, V.icoff[i0] + r);
			return JsItem{JS_K_INS, i == i0, (uint32_t)(V.icoff[i0] + r - V.icoff[i]), i};
		}
		return JsItem{JS_K_M_TAIL, M.n_inss == 0, 0, 0};
	}
	x -= V.n_bitems;
	if (x == 0) return JsItem{JS_K_NODES, V.n_alive == 0, 0, 0};
	x -= 1;
	if (x < V.n_nodes) return JsItem{JS_K_NODE, x == 0, 0, x};
	return JsItem{JS_K_CLOSE, V.n_nodes == 0, 0, 0};
}

// item x through the window; O.at: where the item starts, behind the call where it ends.  `first` of a closing item: the list before it is empty
__host__ __device__ __forceinline__ void js_emit(const JsDev &V, gf_u64 x, GfOut &O)
{
	const JsItem I = js_item(V, x);
	switch (I.kind) {
	case JS_K_OPEN: JS_LIT(O, "{\n  \"paths\": {"); break;
	case JS_K_P_HEAD: {
		const gf_u64 id = V.paths[I.a].path_id;
		if (!I.first) gf_put(O, ',');
		JS_LIT(O, "\n    \""); gf_dec(O, id); JS_LIT(O, "\": {\n      \"id\": "); gf_dec(O, id); JS_LIT(O, ",\n      \"nodes\": [");
		break; }
	case JS_K_P_NODE: if (!I.first) gf_put(O, ','); JS_LIT(O, "\n        "); gf_dec(O, V.nodes[I.a].node_id); break;
	case JS_K_P_TAIL: {
		const JsPath M = V.meta[I.a];
		js_path_tail(O, !I.first, M.tot_len, V.paths[I.a].circular != 0);
		js_string_or_null(O, M.name_len); JS_LIT(O, JS_DESC_KEY); js_string_or_null(O, M.desc_len); JS_LIT(O, "\n    }");
		break; }
	case JS_K_BLOCKS: js_close(O, !I.first, "\n  }", 4, '}'); JS_LIT(O, ",\n  \"blocks\": {"); break;
	case JS_K_B_HEAD: js_block_head(O, I.first, V.blocks[I.a].block_id); O.at += V.blocks[I.a].cons_len; JS_LIT(O, "\",\n      \"alignments\": {"); break;
	case JS_K_M_HEAD: if (!I.first) gf_put(O, ','); JS_LIT(O, "\n        \""); gf_dec(O, V.nodes[V.border[I.a]].node_id); JS_LIT(O, "\": {\n          \"subs\": ["); break;
	case JS_K_SUB: {
		const pga_sub_t S = V.subs[I.a];
		if (!I.first) gf_put(O, ',');
		JS_LIT(O, "\n            {\n              \"pos\": "); gf_dec(O, S.pos); JS_LIT(O, ",\n              \"alt\": \""); gf_put(O, (char)S.alt); JS_LIT(O, "\"\n            }");
		break; }
	case JS_K_J_DELS: js_close(O, !I.first, "\n          ]", 12, ']'); JS_LIT(O, ",\n          \"dels\": ["); break;
	case JS_K_DEL: {
		const pga_del_t D = V.dels[I.a];
		if (!I.first) gf_put(O, ',');
		JS_LIT(O, "\n            {\n              \"pos\": "); gf_dec(O, D.pos); JS_LIT(O, ",\n              \"len\": "); gf_dec(O, D.len); JS_LIT(O, "\n            }");
		break; }
	case JS_K_J_INSS: js_close(O, !I.first, "\n          ]", 12, ']'); JS_LIT(O, ",\n          \"inss\": ["); break;
	case JS_K_INS: {
		const pga_ins_t S = V.inss[I.a];
		const gf_u64 a = (gf_u64)I.c * V.chunk, n = S.len - a < V.chunk ? S.len - a : V.chunk;
		if (I.c == 0) {
			if (!I.first) gf_put(O, ',');
			JS_LIT(O, "\n            {\n              \"pos\": "); gf_dec(O, S.pos); JS_LIT(O, ",\n              \"seq\": \"");
		}
		gf_puts(O, V.ins_seq + S.seq_off + a, (uint32_t)n);
		if (a + n == S.len) JS_LIT(O, "\"\n            }");
		break; }
	case JS_K_M_TAIL: js_close(O, !I.first, "\n          ]", 12, ']'); JS_LIT(O, "\n        }"); break;
	case JS_K_B_TAIL: js_close(O, !I.first, "\n      }", 8, '}'); JS_LIT(O, "\n    }"); break;
	case JS_K_NODES: js_close(O, !I.first, "\n  }", 4, '}'); JS_LIT(O, ",\n  \"nodes\": {"); break;
	case JS_K_NODE: {
		const uint32_t at = V.order[I.a];
		const pga_topo_node_t N = V.nodes[at];
		if (!I.first) gf_put(O, ',');
		JS_LIT(O, "\n    \""); gf_dec(O, N.node_id); JS_LIT(O, "\": {\n      \"id\": "); gf_dec(O, N.node_id);
		JS_LIT(O, ",\n      \"block_id\": "); gf_dec(O, V.blocks[N.block].block_id); JS_LIT(O, ",\n      \"path_id\": "); gf_dec(O, V.paths[V.path_of[at]].path_id);
		JS_LIT(O, ",\n      \"strand\": \""); gf_put(O, N.reverse ? '-' : '+'); JS_LIT(O, "\",\n      \"position\": [\n        "); gf_dec(O, N.pos0);
		JS_LIT(O, ",\n        "); gf_dec(O, N.pos1); JS_LIT(O, "\n      ]\n    }");
		break; }
	default: js_close(O, !I.first, "\n  }", 4, '}'); JS_LIT(O, "\n}"); break;
	}
}

// ---------------------------------------------------------------- 1. the two orders: keys for the sort by node_id, then by block
static __global__ __launch_bounds__(GF_THREADS) void k_json_idkeys(JsDev V)
{
	for (uint64_t i = (uint64_t)blockIdx.x * GF_THREADS + threadIdx.x; i < V.n_nodes; i += (uint64_t)gridDim.x * GF_THREADS) { V.id_key[i] = V.nodes[i].node_id; V.pos[i] = (uint32_t)i; }
}
// behind the first sort: two nodes with one id are neighbours; the block of every sorted position (checked on the host)
static __global__ __launch_bounds__(GF_THREADS) void k_json_blkkeys(JsDev V)
{
	for (uint64_t i = (uint64_t)blockIdx.x * GF_THREADS + threadIdx.x; i < V.n_nodes; i += (uint64_t)gridDim.x * GF_THREADS) {
		if (i && V.id_skey[i] == V.id_skey[i - 1]) atomicMin(&V.err[JS_E_DUPID], (gf_u64)i);
		V.blk_key[i] = V.nodes[V.order[i]].block;
	}
}

// ---------------------------------------------------------------- 2. the edits: counts per slot, items per insertion, what is refused
static __global__ __launch_bounds__(GF_THREADS) void k_json_counts(JsDev V)
{
	for (uint64_t s = (uint64_t)blockIdx.x * GF_THREADS + threadIdx.x; s < V.n_slots; s += (uint64_t)gridDim.x * GF_THREADS) {
		const pga_rc_member_t M = V.members[s];
		V.cnt_s[s] = M.n_subs; V.cnt_d[s] = M.n_dels; V.cnt_i[s] = M.n_inss;
	}
}
static __global__ __launch_bounds__(GF_THREADS) void k_json_chunks(JsDev V)
{
	for (uint64_t i = (uint64_t)blockIdx.x * GF_THREADS + threadIdx.x; i < V.n_inss; i += (uint64_t)gridDim.x * GF_THREADS) V.chunks[i] = js_chunks(V.inss[i].len, V.chunk);
}
static __global__ __launch_bounds__(GF_THREADS) void k_json_check_subs(JsDev V)
{
	for (uint64_t i = (uint64_t)blockIdx.x * GF_THREADS + threadIdx.x; i < V.n_subs; i += (uint64_t)gridDim.x * GF_THREADS)
		if (!js_plain(V.subs[i].alt)) atomicMin(&V.err[JS_E_ALT], (gf_u64)i);
}
// one thread per chunk of an insertion (behind the scan of chunks[]): its range first, no letter of an insertion out of range is read
static __global__ __launch_bounds__(GF_THREADS) void k_json_check_inss(JsDev V)
{
	const gf_u64 n = V.icoff[V.n_inss];
	for (gf_u64 c = (gf_u64)blockIdx.x * GF_THREADS + threadIdx.x; c < n; c += (gf_u64)gridDim.x * GF_THREADS) {
		const gf_u64 i = ts_last_le(V.icoff, 0, V.n_inss, c);
		const pga_ins_t S = V.inss[i];
		if (S.seq_off > V.n_ins_seq || S.len > V.n_ins_seq - S.seq_off) { atomicMin(&V.err[JS_E_INS_RANGE], i); continue; }
		const gf_u64 a = (c - V.icoff[i]) * V.chunk, z = S.len - a < V.chunk ? S.len : a + V.chunk;
		bool bad = false;
		for (gf_u64 k = a; k < z; ++k) bad = bad || !js_plain((uint32_t)(unsigned char)V.ins_seq[S.seq_off + k]);
		if (bad) atomicMin(&V.err[JS_E_INS_LETTER], i);
	}
}

// ---------------------------------------------------------------- 3. the hierarchy (behind the first wait: every slot is named exactly once)
static __global__ __launch_bounds__(GF_THREADS) void k_json_mitems(JsDev V)
{
	for (uint64_t e = (uint64_t)blockIdx.x * GF_THREADS + threadIdx.x; e < V.n_slots; e += (uint64_t)gridDim.x * GF_THREADS) {
		const pga_topo_node_t N = V.nodes[V.border[e]];
		const gf_u64 s = (gf_u64)V.slot_first[N.block] + N.member, i0 = V.ins_off[s], i1 = V.ins_off[s + 1];
		V.mitems[e] = 4 + V.cnt_s[s] + V.cnt_d[s] + (V.icoff[i1] - V.icoff[i0]);
	}
}
static __global__ __launch_bounds__(GF_THREADS) void k_json_bstart(JsDev V)
{
	for (uint64_t k = (uint64_t)blockIdx.x * GF_THREADS + threadIdx.x; k <= V.n_alive; k += (uint64_t)gridDim.x * GF_THREADS)
		V.bstart[k] = 2 * k + V.moff[k < V.n_alive ? V.slot_first[V.ablk[k]] : V.n_slots];
}

// ---------------------------------------------------------------- 4. the layout: every item's length; behind the scan where keys and tails start
static __global__ __launch_bounds__(GF_THREADS) void k_json_lens(JsDev V)
{
	for (uint64_t x = (uint64_t)blockIdx.x * GF_THREADS + threadIdx.x; x < V.n_items; x += (uint64_t)gridDim.x * GF_THREADS) {
		GfOut O{nullptr, 0, 0, 0};
		js_emit(V, x, O);
		V.len[x] = O.at;
	}
}
// a key stands behind the comma (all entries but the first) and "\n    "
static __global__ __launch_bounds__(GF_THREADS) void k_json_offs(JsDev V)
{
	const uint64_t n = V.n_paths > V.n_alive ? V.n_paths : V.n_alive;
	for (uint64_t k = (uint64_t)blockIdx.x * GF_THREADS + threadIdx.x; k < n; k += (uint64_t)gridDim.x * GF_THREADS) {
		if (k < V.n_paths) {
			const gf_u64 x = 1 + V.paths[k].node_off + 2 * k;
			V.path_off[k] = V.off[x] + (k ? 6 : 5); V.tail_off[k] = V.off[x + V.paths[k].n_nodes + 1];
		}
		if (k < V.n_alive) V.block_off[V.ablk[k]] = V.off[2 + V.n_pitems + V.bstart[k]] + (k ? 6 : 5);
	}
}

// ---------------------------------------------------------------- 5. the tile [t0, t1), 0 <= t0 < t1 <= off[n_items]: one thread per item
static __global__ __launch_bounds__(GF_THREADS) void k_json_tile(JsDev V)
{
	__shared__ gf_u64 s_rng[2];
	if (threadIdx.x < 2) s_rng[threadIdx.x] = ts_last_le(V.off, 0, V.n_items, threadIdx.x ? V.t1 - 1 : V.t0);
	__syncthreads();
	const gf_u64 lo = s_rng[0], hi = s_rng[1];
	for (gf_u64 x = lo + (gf_u64)blockIdx.x * GF_THREADS + threadIdx.x; x <= hi; x += (gf_u64)gridDim.x * GF_THREADS) {
		GfOut O{V.tile, V.t0, V.t1, V.off[x]};
		js_emit(V, x, O);
	}
}

// ---------------------------------------------------------------- host side: what is refused before a launch, escaping, the tables
inline void js_fail(const std::string &what) { throw std::runtime_error("pga_export_json: " + what); }
static const char JS_EMPTY[] = "{\n  \"paths\": {},\n  \"blocks\": {},\n  \"nodes\": {}\n}";

// serde_json's escaping of a string: \" \\ \b \f \n \r \t, other bytes below 0x20 as \u00xx (lower-case hex), everything else verbatim
static std::string js_escape(const char *s, uint32_t n)
{
	static const char hex[] = "0123456789abcdef";
	std::string o;
	o.reserve(n);
	for (uint32_t k = 0; k < n; ++k) {
		const unsigned char c = (unsigned char)s[k];
		switch (c) {
		case '"': o += "\\\""; break;
		case '\\': o += "\\\\"; break;
		case '\b': o += "\\b"; break;
		case '\f': o += "\\f"; break;
		case '\n': o += "\\n"; break;
		case '\r': o += "\\r"; break;
		case '\t': o += "\\t"; break;
		default:
			if (c < 0x20) { o += "\\u00"; o += hex[c >> 4]; o += hex[c & 15]; } else o += (char)c;
		}
	}
	return o;
}

struct JsTables {
	TpTables T;
	std::vector<uint32_t> ablk;                    // the alive blocks
	std::vector<JsPath> meta;
	std::vector<std::string> name, desc;           // escaped; empty for null
	uint64_t n_subs = 0, n_dels = 0, n_inss = 0;
	std::vector<gf_u64> cons_at, name_at, desc_at; // per alive block / per path: the file offset of the first letter (behind the layout)
};
// everything the host can refuse, before anything is launched; the totals of the edit lists, the escaped names
static void js_validate(int64_t n_blocks, const pga_topo_block_t *blocks, int64_t n_paths, const pga_topo_path_t *paths, int64_t n_nodes, const pga_topo_node_t *nodes,
                        const char *const *cons, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss, const char *ins_seq,
                        uint64_t n_ins_seq, const uint64_t *tot_len, const char *const *names, const uint32_t *name_len, const char *const *descs, const uint32_t *desc_len,
                        uint32_t flags, JsTables &J)
{
	try { tp_validate(n_blocks, blocks, n_paths, paths, n_nodes, nodes, 0, nullptr, 0, J.T); }
	catch (std::runtime_error &e) { const std::string w = e.what(); const size_t at = w.find(": "); js_fail(at == std::string::npos ? w : w.substr(at + 2)); }
	if (flags) js_fail("unknown flag");
	if (J.T.n_slots && !members) js_fail("null members with a member to write");
	for (uint64_t s = 0; s < J.T.n_slots; ++s) { J.n_subs += members[s].n_subs; J.n_dels += members[s].n_dels; J.n_inss += members[s].n_inss; }
	if ((J.n_subs && !subs) || (J.n_dels && !dels) || (J.n_inss && !inss)) js_fail("a null edit list with a non-zero count");
	if (n_ins_seq && !ins_seq) js_fail("null insertion letters with a non-zero length");
	if (n_paths && (!tot_len || !names || !name_len || !descs || !desc_len)) js_fail("null tot_len, names or descs with a path to write");
	for (int64_t b = 0; b < n_blocks; ++b) {
		if (!blocks[b].alive) continue;
		if (blocks[b].cons_len && (!cons || !cons[b])) js_fail("null consensus of an alive block (block " + std::to_string(b) + ")");
		J.ablk.push_back((uint32_t)b);
	}
	J.meta.resize((size_t)n_paths); J.name.resize((size_t)n_paths); J.desc.resize((size_t)n_paths);
	for (int64_t p = 0; p < n_paths; ++p) {
		if (names[p]) J.name[p] = js_escape(names[p], name_len[p]);
		if (descs[p]) J.desc[p] = js_escape(descs[p], desc_len[p]);
		if (J.name[p].size() >= JS_NULL || J.desc[p].size() >= JS_NULL) js_fail("an escaped name or description of 2^32 - 1 bytes or more (path " + std::to_string(p) + ")");
		J.meta[p] = JsPath{tot_len[p], names[p] ? (uint32_t)J.name[p].size() : JS_NULL, descs[p] ? (uint32_t)J.desc[p].size() : JS_NULL};
	}
}
// what the device found before the first wait
static void js_report(const uint32_t *topo_err, const gf_u64 *err)
{
	if (topo_err[TP_E_DEPTH] != TP_NONE) js_fail("the nodes of a block do not sum to its depth (block " + std::to_string(topo_err[TP_E_DEPTH]) + ")");
	if (topo_err[TP_E_SLOT] != TP_NONE) js_fail(std::string("a (block, member) slot is named by ") + ((topo_err[TP_E_SLOT] & 1u) ? "two nodes" : "no node") + " (slot " + std::to_string(topo_err[TP_E_SLOT] >> 1) + ")");
	if (err[JS_E_DUPID] != JS_NONE) js_fail("two nodes with one node_id (rank " + std::to_string(err[JS_E_DUPID]) + " of the sorted ids)");
	if (err[JS_E_ALT] != JS_NONE) js_fail("a substitution letter that JSON would escape (sub " + std::to_string(err[JS_E_ALT]) + ")");
	if (err[JS_E_INS_RANGE] != JS_NONE) js_fail("seq_off + len of an insertion runs past the insertion letters (insertion " + std::to_string(err[JS_E_INS_RANGE]) + ")");
	if (err[JS_E_INS_LETTER] != JS_NONE) js_fail("an insertion letter that JSON would escape (insertion " + std::to_string(err[JS_E_INS_LETTER]) + ")");
}
// an upper bound of the file's length (it exceeds the true length by less than 2^9 bytes per path, block, member, node and edit), n_chunks: icoff[n_inss]
static void js_bound(const JsTables &J, const pga_topo_block_t *blocks, uint64_t n_nodes, uint64_t n_chunks, uint32_t chunk)
{
	unsigned __int128 bound = 64 + (unsigned __int128)n_nodes * (256 + 32) + (unsigned __int128)J.T.n_slots * 128 + (unsigned __int128)(J.n_subs + J.n_dels + J.n_inss) * 128 +
	                          (unsigned __int128)n_chunks * chunk;
	for (uint32_t b : J.ablk) bound += 160 + blocks[b].cons_len;
	for (size_t p = 0; p < J.meta.size(); ++p) bound += 256 + J.name[p].size() + J.desc[p].size();
	if (bound >= ((unsigned __int128)1 << 63)) js_fail("a file of 2^63 bytes or more");
}
// where the host's letters go: behind the layout, from the offsets of the block keys and the path tails
static void js_fill_table(JsTables &J, const pga_topo_block_t *blocks, const pga_topo_path_t *paths, const gf_u64 *block_off, const gf_u64 *tail_off)
{
	J.cons_at.resize(J.ablk.size()); J.name_at.resize(J.meta.size()); J.desc_at.resize(J.meta.size());
	for (size_t k = 0; k < J.ablk.size(); ++k) {
		GfOut O{nullptr, 0, 0, 0};
		js_block_head(O, true, blocks[J.ablk[k]].block_id);                   // (block_off is the key's: behind "\n    ")
		J.cons_at[k] = block_off[J.ablk[k]] + O.at - 5;
	}
	for (size_t p = 0; p < J.meta.size(); ++p) {
		GfOut O{nullptr, 0, 0, 0};
		js_path_tail(O, paths[p].n_nodes != 0, J.meta[p].tot_len, paths[p].circular != 0);
		J.name_at[p] = tail_off[p] + O.at + 1;
		js_string_or_null(O, J.meta[p].name_len);
		J.desc_at[p] = tail_off[p] + O.at + (sizeof(JS_DESC_KEY) - 1) + 1;
	}
}
// the names, descriptions and consensus letters whose bytes fall into the tile [t0, t1) at `tile`; pi, bi: the first path / alive block that
// may still reach into a tile (they only move forward: O(paths + blocks) over a call)
static void js_host_fill(const JsTables &J, const pga_topo_block_t *blocks, const char *const *cons, char *tile, gf_u64 t0, gf_u64 t1, size_t &pi, size_t &bi)
{
	auto copy = [&](const char *src, gf_u64 a, gf_u64 n) {                  // the file bytes [a, a + n) are src[0 .. n)
		const gf_u64 lo = std::max(a, t0), hi = std::min(a + n, t1);
		if (lo < hi) memcpy(tile + (lo - t0), src + (lo - a), (size_t)(hi - lo));
	};
	for (; pi < J.meta.size(); ++pi) {
		if (J.name_at[pi] >= t1) break;
		copy(J.name[pi].data(), J.name_at[pi], J.name[pi].size());
		if (J.desc_at[pi] >= t1) break;                                       // (the name is copied again with the next tile: it lies in front of it)
		copy(J.desc[pi].data(), J.desc_at[pi], J.desc[pi].size());
		if (J.desc_at[pi] + J.desc[pi].size() > t1) break;                    // it goes on in the next tile
	}
	for (; bi < J.ablk.size(); ++bi) {
		const gf_u64 a = J.cons_at[bi], n = blocks[J.ablk[bi]].cons_len;
		if (a >= t1) break;
		if (n) copy(cons[J.ablk[bi]], a, n);
		if (a + n > t1) break;
	}
}

} // namespace pga
