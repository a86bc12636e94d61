// pga_gfa.hip -- `pangraph export gfa` (io/gfa.rs:79-279) on the flat graph of pga_plan_simplify: the tables of the file (segments, links,
// paths, steps) and its text, streamed.  The reference builds a map of segments, filters every path into a new vector, counts links in a
// hash map and formats line by line; here a POSITION, a STEP and an ITEM of the file are the units of work.
//   host               validation (all of it before anything is launched); one upload of the three arrays
//   k_topo_keys / _check   pga_topo_idx.h: the path of every position, every (block, member) slot named exactly once
//   k_gfa_dupkeys, rocPRIM sort, k_gfa_dupflags   a block with two nodes on one path is duplicated (on the unfiltered graph)
//   k_gfa_keep, the scan, k_gfa_steps / _path_steps   the filter, every kept node's place, the compacted steps, every path's share
//   k_gfa_link_keys, rocPRIM sort, k_topo_heads / _runs, k_gfa_links   one key per step, run heads, the links with their counts
//   host               the first wait: the checks, the counts; then the small tables come back and the emitted segments and paths are
//                      listed (O(blocks + paths)), names and consensus pointers checked
//   k_gfa_lens, the scan, k_gfa_row_off   every item's byte length (the emitter through an empty window), its file offset
//   host               the second wait: n_bytes, byte_off of segments and paths.  Verdict mode ends here.
//   k_gfa_tile         per tile of PGA_EXPORT_TILE_KB: the items that intersect it, one thread per item.  Two device tiles and two pinned
//                      blocks as in pga_export.hip: while the sink consumes tile t-1, tile t is copied and the kernel writes tile t+1.
//   host               behind the copy of a tile: the consensus letters and names that fall into it (gf_host_fill), then the sink
// The kernels and the host tables are pga_gfa_idx.h (no wave intrinsic: tests/emu/gfa_emu.cpp runs them on the host).
// All arithmetic is integer; concurrent stores to one word store the same value, so the result does not depend on the launch geometry.
#include "pga_common.h"
#include "pga_graph_host.h"
#include "../../include/pga_align.h"
#include "pga_gfa_idx.h"

namespace pga {

static unsigned gf_grid(uint64_t items) { return grid_for(items, GF_THREADS, 2048); }

static thread_local double g_gf_ms[4] = {0, 0, 0, 0};
void gfa_last_ms(double *ms) { for (int i = 0; i < 4; ++i) ms[i] = g_gf_ms[i]; }

static const char GF_HEADER[] = "H\tVN:Z:1.0\n";

void export_gfa_host(int64_t n_blocks, const pga_topo_block_t *blocks, int64_t n_paths, const pga_topo_path_t *paths, int64_t n_nodes, const pga_topo_node_t *nodes,
                     const char *const *cons, const char *const *names, const uint32_t *name_len, const pga_gfa_params_t *p, uint32_t flags, pga_gfa_out_t *out,
                     pga_gfa_sink_t sink, void *ctx)
{
	TpTables T;
	gf_validate(n_blocks, blocks, n_paths, paths, n_nodes, nodes, cons, p, flags, T);
	const uint64_t tile_bytes = export_tile_bytes(gf_fail);
	out->segments = host_array<pga_gfa_segment_t>(0, "pga_export_gfa"); out->links = host_array<pga_topo_edge_t>(0, "pga_export_gfa"); out->paths = host_array<pga_gfa_path_t>(0, "pga_export_gfa");
	if (flags & PGA_GFA_STEPS) out->steps = host_array<pga_gfa_step_t>(0, "pga_export_gfa");
	out->n_bytes = sizeof(GF_HEADER) - 1;
	auto header_only = [&]() { if (sink && sink(ctx, GF_HEADER, (int64_t)sizeof(GF_HEADER) - 1) != 0) gf_fail("sink stopped the export"); };
	if (n_paths == 0 || n_nodes == 0) { header_only(); return; }
	const uint64_t nn = (uint64_t)n_nodes, np = (uint64_t)n_paths, nb = (uint64_t)n_blocks;

	// (declared before the streams: the streams are drained first when the scope is left, by a throw too)
	DBuf<char> d_tile[2];
	PinBlock pin[2];
	DBuf<pga_topo_node_t> d_nodes(nn + 1); DBuf<pga_topo_path_t> d_paths(np + 1); DBuf<pga_topo_block_t> d_blocks(nb + 1);
	DBuf<uint32_t> d_depth(nb + 1), d_first(nb + 2), d_pathof(nn + 1), d_cnts(T.n_slots + nb + 1), d_terr(TP_ERRS), d_flags(2 * nb + 1), d_steppath(nn + 1);
	DBuf<uint32_t> d_head(nn + 1), d_hoff(nn + 1), d_rstart(nn + 1);
	DBuf<tp_u64> d_key(nn + 1), d_k0(nn + 1), d_k1(nn + 1);
	DBuf<gf_u64> d_keep(nn + 1), d_psteps(2 * np + 1), d_len, d_rowoff;
	DBuf<pga_gfa_step_t> d_steps(nn + 1); DBuf<pga_topo_edge_t> d_links(nn + 1);
	DBuf<pga_gfa_segment_t> d_segs; DBuf<GfRow> d_rows;
	TileScanBufs<gf_u64> b_keep, b_items;
	Event ev_0, ev_1, ev_ka[2], ev_kb[2], ev_c[2];
	StreamLease s_kern, s_copy;
	const hipStream_t st = s_kern.s, sc = s_copy.s;

	// ---- the uploads, the checks of the graph as pga_plan_simplify makes them ----
	PGA_HIP(hipEventRecord(ev_0.e, st));
	upload(d_nodes, nodes, nn, st); upload(d_paths, paths, np, st); upload(d_blocks, blocks, nb, st);
	upload(d_depth, T.depth.data(), nb, st); upload(d_first, T.slot_first.data(), nb + 1, st);
	d_cnts.zero(st); d_flags.zero(st);
	PGA_HIP(hipMemsetAsync(d_terr.p, 0xff, TP_ERRS * sizeof(uint32_t), st));
	PGA_HIP(hipMemsetAsync(d_k0.p, 0xff, (nn + 1) * sizeof(tp_u64), st));
	TpDev K;
	memset(&K, 0, sizeof(K));
	K.n_nodes = nn; K.n_paths = np; K.n_blocks = nb; K.n_slots = T.n_slots;
	K.nodes = d_nodes.p; K.paths = d_paths.p; K.depth = d_depth.p; K.slot_first = d_first.p; K.path_of = d_pathof.p; K.key = d_key.p;
	K.slot_cnt = d_cnts.p; K.blk_cnt = d_cnts.p + T.n_slots; K.err = d_terr.p;
	GfDev V;
	memset(&V, 0, sizeof(V));
	V.n_nodes = nn; V.n_paths = np; V.n_blocks = nb; V.nodes = d_nodes.p; V.paths = d_paths.p; V.blocks = d_blocks.p; V.path_of = d_pathof.p; V.prm = *p;
	V.dup = d_flags.p; V.used = d_flags.p + nb; V.keep = d_keep.p; V.steps = d_steps.p; V.step_path = d_steppath.p; V.path_steps = d_psteps.p; V.links = d_links.p;
	const GfScan s_keep = b_keep.make(nn, 1);
	V.koff = s_keep.off;
	const unsigned g_pos = gf_grid(nn + 1);
	hipLaunchKernelGGL(k_topo_keys, dim3(g_pos), dim3(TP_THREADS), 0, st, K);
	hipLaunchKernelGGL(k_topo_check, dim3(gf_grid(std::max<uint64_t>(T.n_slots, nb))), dim3(TP_THREADS), 0, st, K);
	// ---- duplication, the filter, the steps ----
	V.dkey = d_key.p; V.dskey = d_k1.p;                                     // (the edge keys of k_topo_keys are not used: their buffer serves)
	hipLaunchKernelGGL(k_gfa_dupkeys, dim3(g_pos), dim3(GF_THREADS), 0, st, V);
	radix_sort_keys(d_key.p, d_k1.p, nn, 64, st);
	hipLaunchKernelGGL(k_gfa_dupflags, dim3(g_pos), dim3(GF_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_gfa_keep, dim3(g_pos), dim3(GF_THREADS), 0, st, V);
	tile_scan_launch(s_keep, TsArray<gf_u64>{d_keep.p}, st);
	hipLaunchKernelGGL(k_gfa_steps, dim3(g_pos), dim3(GF_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_gfa_path_steps, dim3(gf_grid(np)), dim3(GF_THREADS), 0, st, V);
	// ---- the links: keys in d_k0 (all-ones where a step has no successor, and behind the last step), sorted into d_k1 ----
	V.lkey = d_k0.p; V.lskey = d_k1.p; V.head_off = d_hoff.p; V.run_start = d_rstart.p;
	K.skey = d_k1.p; K.head = d_head.p; K.head_off = d_hoff.p; K.run_start = d_rstart.p;
	hipLaunchKernelGGL(k_gfa_link_keys, dim3(g_pos), dim3(GF_THREADS), 0, st, V);
	radix_sort_keys(d_k0.p, d_k1.p, nn, 64, st);
	hipLaunchKernelGGL(k_topo_heads, dim3(g_pos), dim3(TP_THREADS), 0, st, K);
	excl_scan(d_head.p, d_hoff.p, nn + 1, st);
	hipLaunchKernelGGL(k_topo_runs, dim3(g_pos), dim3(TP_THREADS), 0, st, K);
	hipLaunchKernelGGL(k_gfa_links, dim3(g_pos), dim3(GF_THREADS), 0, st, V);
	PGA_HIP(hipGetLastError());
	// ---- the first wait: nothing behind it runs on input that was not checked ----
	uint32_t terr[TP_ERRS], n_runs = 0;
	gf_u64 n_steps = 0;
	fetch(terr, (const uint32_t*)d_terr.p, TP_ERRS, st); fetch(&n_runs, (const uint32_t*)d_hoff.p + nn, 1, st); fetch(&n_steps, (const gf_u64*)s_keep.off + nn, 1, st);
	PGA_HIP(sync_stream(st));
	gf_report(terr);
	if (n_steps > nn || n_runs > n_steps) gf_fail("internal: the device counted more steps than positions, or more links than steps");
	const uint64_t n_links = n_runs;
	std::vector<uint32_t> h_flags(2 * nb);
	std::vector<gf_u64> h_psteps(2 * np);
	free(out->links); out->links = nullptr; out->links = host_array<pga_topo_edge_t>(n_links, "pga_export_gfa");
	if (flags & PGA_GFA_STEPS) { free(out->steps); out->steps = nullptr; out->steps = host_array<pga_gfa_step_t>(n_steps, "pga_export_gfa"); fetch(out->steps, (const pga_gfa_step_t*)d_steps.p, n_steps, st); }
	fetch(h_flags.data(), (const uint32_t*)d_flags.p, 2 * nb, st); fetch(h_psteps.data(), (const gf_u64*)d_psteps.p, 2 * np, st);
	fetch(out->links, (const pga_topo_edge_t*)d_links.p, n_links, st);
	PGA_HIP(sync_stream(st));
	GfTables G;
	gf_tables(n_blocks, blocks, n_paths, paths, cons, names, name_len, *p, h_flags.data() + nb, h_flags.data(), h_psteps.data(), n_steps, n_links, G);
	const uint64_t n_seg = G.segs.size(), n_rows = G.rows.size();
	out->n_links = (int64_t)n_links; out->n_steps = (int64_t)n_steps;
	if (n_steps == 0) { header_only(); return; }
	// ---- the layout ----
	const uint64_t n_items = 4 + n_seg + n_links + n_steps + 2 * n_rows;
	d_segs.alloc(n_seg + 1); d_rows.alloc(n_rows + 1); d_len.alloc(n_items + 1); d_rowoff.alloc(n_rows + 1);
	upload(d_segs, G.segs.data(), n_seg, st); upload(d_rows, G.rows.data(), n_rows, st);
	const GfScan s_items = b_items.make(n_items, 1);
	V.n_seg = n_seg; V.n_links = n_links; V.n_rows = n_rows; V.n_steps = n_steps; V.n_items = n_items;
	V.segs = d_segs.p; V.rows = d_rows.p; V.len = d_len.p; V.off = s_items.off; V.row_off = d_rowoff.p;
	hipLaunchKernelGGL(k_gfa_lens, dim3(gf_grid(n_items)), dim3(GF_THREADS), 0, st, V);
	tile_scan_launch(s_items, TsArray<gf_u64>{d_len.p}, st);
	hipLaunchKernelGGL(k_gfa_row_off, dim3(gf_grid(n_rows)), dim3(GF_THREADS), 0, st, V);
	PGA_HIP(hipGetLastError());
	// ---- the second wait: the length of the file, where every S and P line starts ----
	std::vector<gf_u64> h_segoff(n_seg), h_rowoff(n_rows);
	gf_u64 n_bytes = 0;
	fetch(&n_bytes, (const gf_u64*)s_items.off + n_items, 1, st);
	fetch(h_segoff.data(), (const gf_u64*)s_items.off + 2, n_seg, st); fetch(h_rowoff.data(), (const gf_u64*)d_rowoff.p, n_rows, st);
	PGA_HIP(hipEventRecord(ev_1.e, st));
	PGA_HIP(sync_stream(st));
	if (n_bytes >= (1ULL << 63)) gf_fail("a file of 2^63 bytes or more");
	for (uint64_t k = 0; k < n_seg; ++k) G.segs[k].byte_off = h_segoff[k];
	for (uint64_t k = 0; k < n_rows; ++k) G.paths[k].byte_off = h_rowoff[k];
	free(out->segments); out->segments = nullptr; out->segments = host_array<pga_gfa_segment_t>(n_seg, "pga_export_gfa");
	free(out->paths); out->paths = nullptr; out->paths = host_array<pga_gfa_path_t>(n_rows, "pga_export_gfa");
	std::copy(G.segs.begin(), G.segs.end(), out->segments); std::copy(G.paths.begin(), G.paths.end(), out->paths);
	out->n_segments = (int64_t)n_seg; out->n_paths = (int64_t)n_rows; out->n_bytes = n_bytes;
	{ float ms = 0; PGA_HIP(hipEventElapsedTime(&ms, ev_0.e, ev_1.e)); g_gf_ms[0] = ms; g_gf_ms[1] = g_gf_ms[2] = g_gf_ms[3] = 0; }
	if (!sink) return;
	// ---- the tiles ----
	const uint64_t n_tiles = (n_bytes + tile_bytes - 1) / tile_bytes, cap = std::min<uint64_t>(n_bytes, tile_bytes);
	for (int b = 0; b < (n_tiles > 1 ? 2 : 1); ++b) { d_tile[b].alloc(cap); pin[b].p = (char*)pin_alloc(cap); }
	auto span = [&](uint64_t t, gf_u64 &a, gf_u64 &z) { a = t * tile_bytes; z = std::min<gf_u64>(n_bytes, a + tile_bytes); };
	auto launch = [&](uint64_t t) {
		const int b = (int)(t & 1);
		GfDev W = V;
		span(t, W.t0, W.t1);
		W.tile = d_tile[b].p;
		PGA_HIP(hipEventRecord(ev_ka[b].e, st));
		hipLaunchKernelGGL(k_gfa_tile, dim3((unsigned)std::min<uint64_t>(std::max<uint64_t>((W.t1 - W.t0) / (8 * GF_THREADS), 1), 2048)), dim3(GF_THREADS), 0, st, W);
		PGA_HIP(hipGetLastError());
		PGA_HIP(hipEventRecord(ev_kb[b].e, st));
	};
	size_t si = 0, pi = 0;
	double ms_kern = 0, ms_fill = 0, ms_sink = 0;
	auto deliver = [&](uint64_t t) {                                        // tile t lies in its pinned block: the host's letters, then the sink
		gf_u64 a, z; span(t, a, z);
		const double c0 = now_ms();
		gf_host_fill(G, blocks, cons, names, p->include_sequences != 0, pin[t & 1].p, a, z, si, pi);
		const double c1 = now_ms();
		const int rc = sink(ctx, pin[t & 1].p, (int64_t)(z - a));
		ms_fill += c1 - c0; ms_sink += now_ms() - c1;
		if (rc != 0) {
			(void)hipStreamSynchronize(st); (void)hipStreamSynchronize(sc);     // drain what is in flight: no further sink call
			gf_fail("sink stopped the export");
		}
	};
	auto copied = [&](uint64_t t) {                                         // waits for the copy of tile t; its kernel is over then too
		PGA_HIP(sync_event(ev_c[t & 1].e));
		float ms = 0; PGA_HIP(hipEventElapsedTime(&ms, ev_ka[t & 1].e, ev_kb[t & 1].e)); ms_kern += ms;
	};
	launch(0);
	for (uint64_t t = 0; t < n_tiles; ++t) {
		gf_u64 a, z; span(t, a, z);
		const int b = (int)(t & 1);
		PGA_HIP(hipStreamWaitEvent(sc, ev_kb[b].e, 0));
		PGA_HIP(hipMemcpyAsync(pin[b].p, d_tile[b].p, z - a, hipMemcpyDeviceToHost, sc));   // (the sink of tile t-2 has returned)
		PGA_HIP(hipEventRecord(ev_c[b].e, sc));
		if (t >= 1) copied(t - 1);
		if (t + 1 < n_tiles) launch(t + 1);                                   // (into the device tile of t-1, whose copy is complete)
		if (t >= 1) deliver(t - 1);
	}
	copied(n_tiles - 1);
	deliver(n_tiles - 1);
	g_gf_ms[1] = ms_kern; g_gf_ms[2] = ms_fill; g_gf_ms[3] = ms_sink;
}

} // namespace pga
