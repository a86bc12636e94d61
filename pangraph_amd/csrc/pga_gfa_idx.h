// pga_gfa_idx.h -- the kernels and host tables of pga_gfa.hip (export gfa: io/gfa.rs:79-279 gfa_write / convert_pangraph_to_gfa, Edge of
// circularize/circularize_utils.rs:46-102, on the flat graph of pga_plan_simplify).
// No wave intrinsic, plain stores and the atomics of pga_topo_idx.h only: all of this compiles under hipcc and, with dev/emu/hip_emu.h
// included first, under g++ -std=c++17 -DPGA_EMU (tests/emu/gfa_emu.cpp runs it against a direct scalar construction).
// The path lookup, the graph checks, the edge key and the run heads are pga_topo_idx.h's; the two radix sorts and the scan over the run
// heads are rocPRIM's (pga_gfa.hip) and are not in here.
//
// A POSITION is an index into nodes[]; it is KEPT when its block passes the filter (gfa.rs:239-262).  A STEP is a kept position, numbered
// by the scan over the kept flags: the steps of a path are consecutive, a path's first step is the scanned value at its node_off.  The
// LINK of a step is the pair with the next step of its path, with the path's first step behind the last one of a circular path
// (gfa.rs:201-216), as the key of pga_topo_idx.h; sorted keys are the output order, a run of equal keys is a link with its count.
// The file is a list of ITEMS in file order, each with a byte length:
//   0 the header line, 1 "# blocks\n" (empty without a segment), 2 .. the S lines, "# edges\n", the L lines, "# paths\n", and per
//   emitted path k its head ("P\t" name "\t"), its steps ("{id}{+|-}" and a comma behind all but the last), its tail ("\t*" [circular] "\n"):
//   the head of path k is path item rows[k].step_off + 2 k.
// gf_emit() writes an item through a WINDOW [t0, t1) of the file: a byte inside it is stored, one outside only counted.  With an empty
// window it gives the item's length (k_gfa_lens), so the layout and the text cannot disagree; a 64-bit scan over the lengths gives every
// item its file offset (the tile scan of pga_tile_scan.h); k_gfa_tile writes the items that intersect a tile, an item cut by a tile edge in two parts by two launches.
// Consensus letters and path names are skipped: the host copies them into the tile from the caller's buffers (gf_host_fill).
#pragma once
#include "pga_topo_idx.h"

namespace pga {

typedef unsigned long long gf_u64;
constexpr int GF_THREADS = TS_THREADS, GF_TILE = TS_TILE;
enum { GF_K_HEADER = 0, GF_K_CBLOCKS, GF_K_SEG, GF_K_CEDGES, GF_K_LINK, GF_K_CPATHS, GF_K_HEAD, GF_K_STEP, GF_K_TAIL };

typedef TileScan<gf_u64> GfScan;           // pga_tile_scan.h, one quantity: off[i] = the sum of val[0 .. i) of a TsArray, off[n] the total
struct GfRow { gf_u64 step_off; uint32_t n_steps, name_len; int32_t circular, pad; };   // an emitted path
struct GfDev {
	uint64_t n_nodes, n_paths, n_blocks;
	const pga_topo_node_t *nodes; const pga_topo_path_t *paths; const pga_topo_block_t *blocks;
	const uint32_t *path_of;                 // per position (behind k_topo_keys)
	pga_gfa_params_t prm;
	// duplication
	gf_u64 *dkey; const gf_u64 *dskey;       // per position: block << 32 | path index; sorted
	uint32_t *dup, *used;                    // per block (zeroed before): duplicated; named by a kept position
	// the filter and the steps
	gf_u64 *keep; const gf_u64 *koff;        // per position: 0 / 1; its scan (n_nodes + 1 entries)
	pga_gfa_step_t *steps; uint32_t *step_path;   // n_nodes entries each, the first koff[n_nodes] written
	gf_u64 *path_steps;                      // per path: its first step, its number of steps
	tp_u64 *lkey;                            // n_nodes entries, all-ones before: the link of every step
	// the links (behind the sort and k_topo_heads / _runs)
	const tp_u64 *lskey; const uint32_t *head_off, *run_start; pga_topo_edge_t *links;
	// the layout
	uint64_t n_seg, n_links, n_rows, n_steps, n_items;
	const pga_gfa_segment_t *segs; const GfRow *rows;
	gf_u64 *len; const gf_u64 *off;          // per item; off: n_items + 1 entries
	gf_u64 *row_off;                         // per emitted path: where its P line starts
	// the tile
	char *tile; gf_u64 t0, t1;
};

// the number of decimal digits: comparisons against the powers of ten, no division
__host__ __device__ inline uint32_t gf_width(gf_u64 v)
{
	const gf_u64 p10[19] = {10ULL, 100ULL, 1000ULL, 10000ULL, 100000ULL, 1000000ULL, 10000000ULL, 100000000ULL, 1000000000ULL, 10000000000ULL, 100000000000ULL,
	                        1000000000000ULL, 10000000000000ULL, 100000000000000ULL, 1000000000000000ULL, 10000000000000000ULL, 100000000000000000ULL,
	                        1000000000000000000ULL, 10000000000000000000ULL};
	uint32_t w = 1;
	for (int k = 0; k < 19; ++k) w += v >= p10[k] ? 1u : 0u;
	return w;
}

// ---------------------------------------------------------------- the window
struct GfOut { char *tile; gf_u64 t0, t1, at; };
__host__ __device__ inline void gf_put(GfOut &O, char c) { if (O.at >= O.t0 && O.at < O.t1) O.tile[O.at - O.t0] = c; ++O.at; }
__host__ __device__ inline void gf_puts(GfOut &O, const char *s, uint32_t n)
{
	if (O.at + n <= O.t0 || O.at >= O.t1) { O.at += n; return; }
	for (uint32_t k = 0; k < n; ++k) gf_put(O, s[k]);
}
__host__ __device__ inline void gf_dec(GfOut &O, gf_u64 v)
{
	const uint32_t w = gf_width(v);
	if (!(O.at + w <= O.t0 || O.at >= O.t1))
		for (uint32_t k = w; k-- > 0; v /= 10) { const gf_u64 at = O.at + k; if (at >= O.t0 && at < O.t1) O.tile[at - O.t0] = (char)('0' + (int)(v % 10)); }
	O.at += w;
}

struct GfItem { int kind; gf_u64 a; bool last; };
__host__ __device__ inline GfItem gf_item(const GfDev &V, gf_u64 x)
{
	if (x == 0) return GfItem{GF_K_HEADER, 0, false};
	if (x == 1) return GfItem{GF_K_CBLOCKS, 0, false};
	x -= 2;
	if (x < V.n_seg) return GfItem{GF_K_SEG, x, false};
	x -= V.n_seg;
	if (x == 0) return GfItem{GF_K_CEDGES, 0, false};
	x -= 1;
	if (x < V.n_links) return GfItem{GF_K_LINK, x, false};
	x -= V.n_links;
	if (x == 0) return GfItem{GF_K_CPATHS, 0, false};
	x -= 1;
	gf_u64 lo = 0, hi = V.n_rows;                                           // rows[lo].step_off + 2 lo <= x < the same of hi
	while (hi - lo > 1) { const gf_u64 mid = (lo + hi) >> 1; if (V.rows[mid].step_off + 2 * mid <= x) lo = mid; else hi = mid; }
	const GfRow R = V.rows[lo];
	const gf_u64 j = x - (R.step_off + 2 * lo);
	if (j == 0) return GfItem{GF_K_HEAD, lo, false};
	if (j == (gf_u64)R.n_steps + 1) return GfItem{GF_K_TAIL, lo, false};
	return GfItem{GF_K_STEP, R.step_off + j - 1, j == R.n_steps};
}
// item x through the window; O.at: where the item starts, behind the call where it ends
__host__ __device__ inline void gf_emit(const GfDev &V, gf_u64 x, GfOut &O)
{
	const GfItem I = gf_item(V, x);
	switch (I.kind) {
	case GF_K_HEADER: gf_puts(O, "H\tVN:Z:1.0\n", 11); break;
	case GF_K_CBLOCKS: if (V.n_seg) gf_puts(O, "# blocks\n", 9); break;
	case GF_K_CEDGES: if (V.n_links) gf_puts(O, "# edges\n", 8); break;
	case GF_K_CPATHS: if (V.n_rows) gf_puts(O, "# paths\n", 8); break;
	case GF_K_SEG: {
		const pga_gfa_segment_t S = V.segs[I.a];
		gf_puts(O, "S\t", 2); gf_dec(O, V.blocks[S.block].block_id); gf_put(O, '\t');
		if (V.prm.include_sequences) O.at += S.cons_len; else gf_put(O, '*');   // (the letters are the host's)
		gf_puts(O, "\tRC:i:", 6); gf_dec(O, (gf_u64)S.depth * S.cons_len); gf_puts(O, "\tLN:i:", 6); gf_dec(O, S.cons_len);
		if (S.duplicated) gf_puts(O, "\tTP:Z:duplicated", 16);
		gf_put(O, '\n');
		break; }
	case GF_K_LINK: {
		const pga_topo_edge_t E = V.links[I.a];
		gf_puts(O, "L\t", 2); gf_dec(O, V.blocks[E.b1].block_id); gf_put(O, '\t'); gf_put(O, E.s1 ? '-' : '+'); gf_put(O, '\t');
		gf_dec(O, V.blocks[E.b2].block_id); gf_put(O, '\t'); gf_put(O, E.s2 ? '-' : '+'); gf_puts(O, "\t*\tRC:i:", 8); gf_dec(O, E.count); gf_put(O, '\n');
		break; }
	case GF_K_HEAD: gf_puts(O, "P\t", 2); O.at += V.rows[I.a].name_len; gf_put(O, '\t'); break;   // (the name is the host's)
	case GF_K_STEP: {
		const pga_gfa_step_t S = V.steps[I.a];
		gf_dec(O, V.blocks[S.block].block_id); gf_put(O, S.reverse ? '-' : '+');
		if (!I.last) gf_put(O, ',');
		break; }
	default: gf_puts(O, "\t*", 2); if (V.rows[I.a].circular) gf_puts(O, "\tTP:Z:circular", 14); gf_put(O, '\n'); break;
	}
}

// ---------------------------------------------------------------- 1. duplication: (block, path) keys; equal neighbours of the sorted keys
static __global__ __launch_bounds__(GF_THREADS) void k_gfa_dupkeys(GfDev V)
{
	for (uint64_t i = (uint64_t)blockIdx.x * GF_THREADS + threadIdx.x; i < V.n_nodes; i += (uint64_t)gridDim.x * GF_THREADS)
		V.dkey[i] = (gf_u64)V.nodes[i].block << 32 | V.path_of[i];
}
// every writer stores the same value: no atomic
static __global__ __launch_bounds__(GF_THREADS) void k_gfa_dupflags(GfDev V)
{
	for (uint64_t i = (uint64_t)blockIdx.x * GF_THREADS + threadIdx.x + 1; i < V.n_nodes; i += (uint64_t)gridDim.x * GF_THREADS)
		if (V.dskey[i] == V.dskey[i - 1]) V.dup[V.dskey[i] >> 32] = 1u;
}

// ---------------------------------------------------------------- 2. the filter, one thread per position
static __global__ __launch_bounds__(GF_THREADS) void k_gfa_keep(GfDev V)
{
	for (uint64_t i = (uint64_t)blockIdx.x * GF_THREADS + threadIdx.x; i < V.n_nodes; i += (uint64_t)gridDim.x * GF_THREADS) {
		const uint32_t b = V.nodes[i].block;                                  // (checked on the host)
		const pga_topo_block_t B = V.blocks[b];
		const bool keep = B.cons_len >= V.prm.min_len && B.cons_len <= V.prm.max_len && B.depth >= V.prm.min_depth && B.depth <= V.prm.max_depth &&
		                  !(V.prm.no_duplicated && V.dup[b]);
		V.keep[i] = keep ? 1ULL : 0ULL;
		if (keep) V.used[b] = 1u;
	}
}

// ---------------------------------------------------------------- 3. behind the scan of keep[]: the steps, the paths' shares, the link keys
static __global__ __launch_bounds__(GF_THREADS) void k_gfa_steps(GfDev V)
{
	for (uint64_t i = (uint64_t)blockIdx.x * GF_THREADS + threadIdx.x; i < V.n_nodes; i += (uint64_t)gridDim.x * GF_THREADS) {
		if (!V.keep[i]) continue;
		const pga_topo_node_t A = V.nodes[i];
		V.steps[V.koff[i]] = pga_gfa_step_t{A.block, A.reverse ? 1 : 0};
		V.step_path[V.koff[i]] = V.path_of[i];
	}
}
static __global__ __launch_bounds__(GF_THREADS) void k_gfa_path_steps(GfDev V)
{
	for (uint64_t p = (uint64_t)blockIdx.x * GF_THREADS + threadIdx.x; p < V.n_paths; p += (uint64_t)gridDim.x * GF_THREADS) {
		const pga_topo_path_t P = V.paths[p];
		const gf_u64 a = V.koff[P.node_off], z = V.koff[P.node_off + P.n_nodes];
		V.path_steps[2 * p] = a; V.path_steps[2 * p + 1] = z - a;
	}
}
// one thread per step: the pair with the next step of its path, the first one behind the last of a circular path
static __global__ __launch_bounds__(GF_THREADS) void k_gfa_link_keys(GfDev V)
{
	const gf_u64 n_steps = V.koff[V.n_nodes];
	for (uint64_t r = (uint64_t)blockIdx.x * GF_THREADS + threadIdx.x; r < n_steps; r += (uint64_t)gridDim.x * GF_THREADS) {
		const pga_topo_path_t P = V.paths[V.step_path[r]];
		const gf_u64 a = V.koff[P.node_off], z = V.koff[P.node_off + P.n_nodes];
		const gf_u64 next = r + 1 < z ? r + 1 : P.circular ? a : ~0ULL;
		if (next == ~0ULL) continue;                                          // (lkey[] is all-ones before)
		const pga_gfa_step_t A = V.steps[r], B = V.steps[next];
		V.lkey[r] = tp_key(A.block, (uint32_t)A.reverse, B.block, (uint32_t)B.reverse);
	}
}
// one thread per run of the sorted keys
static __global__ __launch_bounds__(GF_THREADS) void k_gfa_links(GfDev V)
{
	const uint64_t n_runs = V.head_off[V.n_nodes];
	for (uint64_t r = (uint64_t)blockIdx.x * GF_THREADS + threadIdx.x; r < n_runs; r += (uint64_t)gridDim.x * GF_THREADS)
		V.links[r] = tp_edge(V.lskey[V.run_start[r]], V.run_start[r + 1] - V.run_start[r]);
}

// ---------------------------------------------------------------- 4. the layout: every item's length; behind the scan where the P lines start
static __global__ __launch_bounds__(GF_THREADS) void k_gfa_lens(GfDev V)
{
	for (uint64_t x = (uint64_t)blockIdx.x * GF_THREADS + threadIdx.x; x < V.n_items; x += (uint64_t)gridDim.x * GF_THREADS) {
		GfOut O{nullptr, 0, 0, 0};
		gf_emit(V, x, O);
		V.len[x] = O.at;
	}
}
static __global__ __launch_bounds__(GF_THREADS) void k_gfa_row_off(GfDev V)
{
	const uint64_t base = 4 + V.n_seg + V.n_links;
	for (uint64_t k = (uint64_t)blockIdx.x * GF_THREADS + threadIdx.x; k < V.n_rows; k += (uint64_t)gridDim.x * GF_THREADS)
		V.row_off[k] = V.off[base + V.rows[k].step_off + 2 * k];
}

// ---------------------------------------------------------------- 5. the tile [t0, t1), 0 <= t0 < t1 <= off[n_items]: one thread per item
static __global__ __launch_bounds__(GF_THREADS) void k_gfa_tile(GfDev V)
{
	__shared__ gf_u64 s_rng[2];
	if (threadIdx.x < 2) s_rng[threadIdx.x] = ts_last_le(V.off, 0, V.n_items, threadIdx.x ? V.t1 - 1 : V.t0);
	__syncthreads();
	const gf_u64 lo = s_rng[0], hi = s_rng[1];
	for (gf_u64 x = lo + (gf_u64)blockIdx.x * GF_THREADS + threadIdx.x; x <= hi; x += (gf_u64)gridDim.x * GF_THREADS) {
		GfOut O{V.tile, V.t0, V.t1, V.off[x]};
		gf_emit(V, x, O);
	}
}

// ---------------------------------------------------------------- host side: what is refused before a launch, the tables behind the first wait
inline void gf_fail(const std::string &what) { throw std::runtime_error("pga_export_gfa: " + what); }

static void gf_validate(int64_t n_blocks, const pga_topo_block_t *blocks, int64_t n_paths, const pga_topo_path_t *paths, int64_t n_nodes, const pga_topo_node_t *nodes,
                        const char *const *cons, const pga_gfa_params_t *p, uint32_t flags, TpTables &T)
{
	try { tp_validate(n_blocks, blocks, n_paths, paths, n_nodes, nodes, 0, nullptr, 0, T); }
	catch (std::runtime_error &e) { const std::string w = e.what(); const size_t at = w.find(": "); gf_fail(at == std::string::npos ? w : w.substr(at + 2)); }
	if (flags & ~PGA_GFA_STEPS) gf_fail("unknown flag");
	if (!p) gf_fail("null parameters");
	if (p->min_len > p->max_len) gf_fail("minimum_length above maximum_length");
	if (p->min_depth > p->max_depth) gf_fail("minimum_depth above maximum_depth");
	if (p->include_sequences && !cons && n_blocks) gf_fail("include_sequences without consensus letters");
}
// what the device found before the first wait
static void gf_report(const uint32_t *topo_err)
{
	if (topo_err[TP_E_DEPTH] != TP_NONE) gf_fail("the nodes of a block do not sum to its depth (block " + std::to_string(topo_err[TP_E_DEPTH]) + ")");
	if (topo_err[TP_E_SLOT] != TP_NONE) gf_fail(std::string("a (block, member) slot is named by ") + ((topo_err[TP_E_SLOT] & 1u) ? "two nodes" : "no node") + " (slot " + std::to_string(topo_err[TP_E_SLOT] >> 1) + ")");
}
struct GfTables { std::vector<pga_gfa_segment_t> segs; std::vector<pga_gfa_path_t> paths; std::vector<GfRow> rows; };
// the emitted segments and paths (byte_off still 0), from the flags per block and the shares per path; the refusals that need them
static void gf_tables(int64_t n_blocks, const pga_topo_block_t *blocks, int64_t n_paths, const pga_topo_path_t *paths, const char *const *cons, const char *const *names,
                      const uint32_t *name_len, const pga_gfa_params_t &prm, const uint32_t *used, const uint32_t *dup, const gf_u64 *path_steps, uint64_t n_steps,
                      uint64_t n_links, GfTables &G)
{
	unsigned __int128 bound = 36 + (unsigned __int128)n_steps * 22 + (unsigned __int128)n_links * 66;
	for (int64_t b = 0; b < n_blocks; ++b) {
		if (!used[b]) continue;
		if (prm.include_sequences && blocks[b].cons_len && !cons[b]) gf_fail("null consensus of an emitted block (block " + std::to_string(b) + ")");
		G.segs.push_back(pga_gfa_segment_t{(uint32_t)b, blocks[b].depth, blocks[b].cons_len, dup[b] ? 1 : 0, 0});
		bound += 83 + (prm.include_sequences ? blocks[b].cons_len : 0u);
	}
	for (int64_t p = 0; p < n_paths; ++p) {
		const gf_u64 a = path_steps[2 * p], n = path_steps[2 * p + 1];
		if (a + n > n_steps || n > paths[p].n_nodes) gf_fail("internal: the steps of a path lie outside the step list (path " + std::to_string(p) + ")");
		if (n == 0) continue;
		if (!names || !name_len) gf_fail("null names with a path to emit");
		if (name_len[p] && !names[p]) gf_fail("null name of an emitted path (path " + std::to_string(p) + ")");
		G.paths.push_back(pga_gfa_path_t{(uint32_t)p, (uint32_t)n, a, 0});
		G.rows.push_back(GfRow{a, (uint32_t)n, name_len[p], paths[p].circular ? 1 : 0, 0});
		bound += 20 + name_len[p];
	}
	if (bound >= ((unsigned __int128)1 << 63)) gf_fail("a file of 2^63 bytes or more");
}
// the consensus letters and names whose bytes fall into the tile [t0, t1) at `tile`; si, pi: the first segment / path that may still
// reach into a tile (they only move forward: O(segments + paths) over a call)
static void gf_host_fill(const GfTables &G, const pga_topo_block_t *blocks, const char *const *cons, const char *const *names, bool include_sequences,
                         char *tile, gf_u64 t0, gf_u64 t1, size_t &si, size_t &pi)
{
	auto copy = [&](const char *src, gf_u64 a, gf_u64 n) {                  // the file bytes [a, a + n) are src[0 .. n)
		const gf_u64 lo = std::max(a, t0), hi = std::min(a + n, t1);
		if (lo < hi) memcpy(tile + (lo - t0), src + (lo - a), (size_t)(hi - lo));
	};
	for (; include_sequences && si < G.segs.size(); ++si) {
		const pga_gfa_segment_t &S = G.segs[si];
		const gf_u64 a = S.byte_off + 3 + gf_width(blocks[S.block].block_id);
		if (a >= t1) break;
		if (S.cons_len) copy(cons[S.block], a, S.cons_len);
		if (a + S.cons_len > t1) break;                                       // it goes on in the next tile
	}
	for (; pi < G.paths.size(); ++pi) {
		const gf_u64 a = G.paths[pi].byte_off + 2, n = G.rows[pi].name_len;
		if (a >= t1) break;
		if (n) copy(names[G.paths[pi].path], a, n);
		if (a + n > t1) break;
	}
}

} // namespace pga
