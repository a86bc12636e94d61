// pga_json.hip -- the pangraph JSON (serde_json::to_writer_pretty of Pangraph, as build_run.rs:78 and simplify_run.rs:20 write it) on the flat
// graph of pga_plan_simplify and the block arrays of pga_reconsensus: where its parts start, and its text, streamed.  The reference walks
// three BTreeMaps and formats value by value; here an ITEM of the file is the unit of work.
//   host               validation (all of it before anything is launched), the escaped names; one upload of the graph and the edit lists
//   k_topo_keys / _check   pga_topo_idx.h: the path of every position, every (block, member) slot named exactly once
//   k_json_idkeys, rocPRIM sort, k_json_blkkeys, rocPRIM sort   the positions by node_id ("nodes"), then stably by block ("alignments")
//   k_json_counts, three scans, k_json_chunks, the scan   where every member's edits start, the items of every insertion
//   k_json_check_subs / _inss   letters that JSON would escape, insertions out of range
//   host               the first wait: the checks; nothing behind it runs on input that was not checked
//   k_json_mitems, the scan, k_json_bstart   the items of every emitted member, the first item of every block
//   host               the second wait: the number of items (it sizes the layout)
//   k_json_lens, the scan, k_json_offs   every item's byte length (the emitter through an empty window), its file offset
//   host               the third wait: n_bytes and the offsets.  Verdict mode ends here.
//   k_json_tile        per tile of PGA_EXPORT_TILE_KB: the items that intersect it, one thread per item, two tiles in flight as in pga_gfa.hip
//   host               behind the copy of a tile: names, descriptions and consensus letters that fall into it (js_host_fill), then the sink
// The kernels and the host tables are pga_json_idx.h (no wave intrinsic: tests/emu/json_emu.cpp runs them on the host).
// All arithmetic is integer; concurrent stores to one word store the same value or go through atomicMin.
#include "pga_common.h"
#include "pga_graph_host.h"
#include "../../include/pga_align.h"
#include "pga_json_idx.h"

namespace pga {

static unsigned js_grid(uint64_t items) { return grid_for(items, GF_THREADS, 2048); }
// measurement only: PGA_JSON_INS_CHUNK overrides the letters of an insertion per item (the text does not depend on it)
static uint32_t js_chunk()
{
	const char *e = getenv("PGA_JSON_INS_CHUNK");
	if (!e || !*e) return JS_CHUNK;
	char *end = nullptr;
	const long long v = strtoll(e, &end, 10);
	if (*end || v < 1 || v > (1LL << 30)) js_fail(std::string("PGA_JSON_INS_CHUNK must be a number of letters from 1 to 2^30 (got '") + e + "')");
	return (uint32_t)v;
}

static thread_local double g_js_ms[4] = {0, 0, 0, 0};
void json_last_ms(double *ms) { for (int i = 0; i < 4; ++i) ms[i] = g_js_ms[i]; }

void export_json_host(int64_t n_blocks, const pga_topo_block_t *blocks, int64_t n_paths, const pga_topo_path_t *paths, int64_t n_nodes, const pga_topo_node_t *nodes,
                      const char *const *cons, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss, const char *ins_seq,
                      uint64_t n_ins_seq, const uint64_t *tot_len, const char *const *names, const uint32_t *name_len, const char *const *descs, const uint32_t *desc_len,
                      uint32_t flags, pga_json_out_t *out, pga_gfa_sink_t sink, void *ctx)
{
	JsTables J;
	js_validate(n_blocks, blocks, n_paths, paths, n_nodes, nodes, cons, members, subs, dels, inss, ins_seq, n_ins_seq, tot_len, names, name_len, descs, desc_len, flags, J);
	const uint64_t tile_bytes = export_tile_bytes(js_fail);
	const uint32_t chunk = js_chunk();
	const uint64_t nn = (uint64_t)n_nodes, np = (uint64_t)n_paths, nb = (uint64_t)n_blocks, ns = J.T.n_slots, na = J.ablk.size();
	out->path_off = host_array<uint64_t>(np, "pga_export_json"); out->block_off = host_array<uint64_t>(nb, "pga_export_json"); out->node_order = host_array<uint32_t>(nn, "pga_export_json");
	out->n_paths = n_paths; out->n_blocks = n_blocks; out->n_nodes = n_nodes;
	if (nb == 0 && np == 0 && nn == 0) {
		out->n_bytes = sizeof(JS_EMPTY) - 1; out->section_off[0] = 4; out->section_off[1] = 19; out->section_off[2] = 35;
		if (sink && sink(ctx, JS_EMPTY, (int64_t)sizeof(JS_EMPTY) - 1) != 0) js_fail("sink stopped the export");
		return;
	}

	// (declared before the streams: the streams are drained first when the scope is left, by a throw too)
	DBuf<char> d_tile[2];
	PinBlock pin[2];
	DBuf<pga_topo_node_t> d_nodes(nn + 1); DBuf<pga_topo_path_t> d_paths(np + 1); DBuf<pga_topo_block_t> d_blocks(nb + 1); DBuf<JsPath> d_meta(np + 1);
	DBuf<uint32_t> d_depth(nb + 1), d_first(nb + 2), d_pathof(nn + 1), d_cnts(ns + nb + 1), d_terr(TP_ERRS), d_ablk(na + 1);
	DBuf<uint32_t> d_pos(nn + 1), d_order(nn + 1), d_bk(nn + 1), d_bsk(nn + 1), d_border(nn + 1);
	DBuf<tp_u64> d_key(nn + 1);
	DBuf<gf_u64> d_idk(nn + 1), d_idsk(nn + 1), d_jerr(JS_ERRS), d_cs(ns + 1), d_cd(ns + 1), d_ci(ns + 1), d_chunks(J.n_inss + 1), d_mitems(ns + 1), d_bstart(na + 1), d_len;
	DBuf<gf_u64> d_pathoff(np + 1), d_tailoff(np + 1), d_blockoff(nb + 1);
	DBuf<pga_rc_member_t> d_members(ns + 1); DBuf<pga_sub_t> d_subs(J.n_subs + 1); DBuf<pga_del_t> d_dels(J.n_dels + 1); DBuf<pga_ins_t> d_inss(J.n_inss + 1);
	DBuf<char> d_insseq(n_ins_seq + 1);
	TileScanBufs<gf_u64> b_s, b_d, b_i, b_c, b_m, b_items;
	Event ev_0, ev_1, ev_ka[2], ev_kb[2], ev_c[2];
	StreamLease s_kern, s_copy;
	const hipStream_t st = s_kern.s, sc = s_copy.s;

	// ---- the uploads, the checks of the graph as pga_plan_simplify makes them ----
	PGA_HIP(hipEventRecord(ev_0.e, st));
	upload(d_nodes, nodes, nn, st); upload(d_paths, paths, np, st); upload(d_blocks, blocks, nb, st); upload(d_meta, J.meta.data(), np, st);
	upload(d_depth, J.T.depth.data(), nb, st); upload(d_first, J.T.slot_first.data(), nb + 1, st); upload(d_ablk, J.ablk.data(), na, st);
	upload(d_members, members, ns, st); upload(d_subs, subs, J.n_subs, st); upload(d_dels, dels, J.n_dels, st); upload(d_inss, inss, J.n_inss, st); upload(d_insseq, ins_seq, n_ins_seq, st);
	d_cnts.zero(st);
	PGA_HIP(hipMemsetAsync(d_terr.p, 0xff, TP_ERRS * sizeof(uint32_t), st));
	PGA_HIP(hipMemsetAsync(d_jerr.p, 0xff, JS_ERRS * sizeof(gf_u64), st));
	PGA_HIP(hipMemsetAsync(d_blockoff.p, 0xff, (nb + 1) * sizeof(gf_u64), st));
	TpDev K;
	memset(&K, 0, sizeof(K));
	K.n_nodes = nn; K.n_paths = np; K.n_blocks = nb; K.n_slots = ns;
	K.nodes = d_nodes.p; K.paths = d_paths.p; K.depth = d_depth.p; K.slot_first = d_first.p; K.path_of = d_pathof.p; K.key = d_key.p;
	K.slot_cnt = d_cnts.p; K.blk_cnt = d_cnts.p + ns; K.err = d_terr.p;
	JsDev V;
	memset(&V, 0, sizeof(V));
	V.n_nodes = nn; V.n_paths = np; V.n_blocks = nb; V.n_slots = ns; V.n_alive = na; V.n_subs = J.n_subs; V.n_dels = J.n_dels; V.n_inss = J.n_inss; V.n_ins_seq = n_ins_seq;
	V.nodes = d_nodes.p; V.paths = d_paths.p; V.blocks = d_blocks.p; V.meta = d_meta.p; V.slot_first = d_first.p; V.path_of = d_pathof.p;
	V.members = d_members.p; V.subs = d_subs.p; V.dels = d_dels.p; V.inss = d_inss.p; V.ins_seq = d_insseq.p; V.chunk = chunk;
	V.id_key = d_idk.p; V.pos = d_pos.p; V.id_skey = d_idsk.p; V.order = d_order.p; V.blk_key = d_bk.p; V.border = d_border.p; V.err = d_jerr.p;
	V.cnt_s = d_cs.p; V.cnt_d = d_cd.p; V.cnt_i = d_ci.p; V.chunks = d_chunks.p; V.mitems = d_mitems.p; V.ablk = d_ablk.p; V.bstart = d_bstart.p;
	V.path_off = d_pathoff.p; V.tail_off = d_tailoff.p; V.block_off = d_blockoff.p;
	const GfScan s_s = b_s.make(ns, 1), s_d = b_d.make(ns, 1), s_i = b_i.make(ns, 1), s_c = b_c.make(J.n_inss, 1), s_m = b_m.make(ns, 1);
	V.sub_off = s_s.off; V.del_off = s_d.off; V.ins_off = s_i.off; V.icoff = s_c.off; V.moff = s_m.off;
	const unsigned g_pos = js_grid(nn + 1);
	hipLaunchKernelGGL(k_topo_keys, dim3(g_pos), dim3(TP_THREADS), 0, st, K);
	hipLaunchKernelGGL(k_topo_check, dim3(js_grid(std::max<uint64_t>(ns, nb))), dim3(TP_THREADS), 0, st, K);
	// ---- the two orders ----
	unsigned blk_bits = 1;
	while (blk_bits < 32 && (nb >> blk_bits)) ++blk_bits;
	hipLaunchKernelGGL(k_json_idkeys, dim3(g_pos), dim3(GF_THREADS), 0, st, V);
	radix_sort_pairs(d_idk.p, d_idsk.p, d_pos.p, d_order.p, nn, 64, st);
	hipLaunchKernelGGL(k_json_blkkeys, dim3(g_pos), dim3(GF_THREADS), 0, st, V);
	radix_sort_pairs(d_bk.p, d_bsk.p, d_order.p, d_border.p, nn, blk_bits, st);
	// ---- the edits ----
	hipLaunchKernelGGL(k_json_counts, dim3(js_grid(ns)), dim3(GF_THREADS), 0, st, V);
	tile_scan_launch(s_s, TsArray<gf_u64>{d_cs.p}, st); tile_scan_launch(s_d, TsArray<gf_u64>{d_cd.p}, st); tile_scan_launch(s_i, TsArray<gf_u64>{d_ci.p}, st);
	hipLaunchKernelGGL(k_json_chunks, dim3(js_grid(J.n_inss)), dim3(GF_THREADS), 0, st, V);
	tile_scan_launch(s_c, TsArray<gf_u64>{d_chunks.p}, st);
	hipLaunchKernelGGL(k_json_check_subs, dim3(js_grid(J.n_subs)), dim3(GF_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_json_check_inss, dim3(js_grid(J.n_inss * 4)), dim3(GF_THREADS), 0, st, V);
	PGA_HIP(hipGetLastError());
	// ---- the first wait: nothing behind it runs on input that was not checked ----
	uint32_t terr[TP_ERRS];
	gf_u64 jerr[JS_ERRS], n_chunks = 0;
	fetch(terr, (const uint32_t*)d_terr.p, TP_ERRS, st); fetch(jerr, (const gf_u64*)d_jerr.p, JS_ERRS, st); fetch(&n_chunks, (const gf_u64*)s_c.off + J.n_inss, 1, st);
	fetch(out->node_order, (const uint32_t*)d_order.p, nn, st);
	PGA_HIP(sync_stream(st));
	js_report(terr, jerr);
	if (ns != nn) js_fail("internal: the device accepted a graph whose slots and nodes differ in number");
	js_bound(J, blocks, nn, n_chunks, chunk);
	// ---- the hierarchy and the layout ----
	hipLaunchKernelGGL(k_json_mitems, dim3(js_grid(ns)), dim3(GF_THREADS), 0, st, V);
	tile_scan_launch(s_m, TsArray<gf_u64>{d_mitems.p}, st);
	hipLaunchKernelGGL(k_json_bstart, dim3(js_grid(na + 1)), dim3(GF_THREADS), 0, st, V);
	gf_u64 n_mitems = 0;
	fetch(&n_mitems, (const gf_u64*)s_m.off + ns, 1, st);
	PGA_HIP(sync_stream(st));
	V.n_pitems = nn + 2 * np; V.n_bitems = 2 * na + n_mitems; V.n_items = 4 + V.n_pitems + V.n_bitems + nn;
	d_len.alloc(V.n_items + 1);
	const GfScan s_items = b_items.make(V.n_items, 1);
	V.len = d_len.p; V.off = s_items.off;
	hipLaunchKernelGGL(k_json_lens, dim3(js_grid(V.n_items)), dim3(GF_THREADS), 0, st, V);
	tile_scan_launch(s_items, TsArray<gf_u64>{d_len.p}, st);
	hipLaunchKernelGGL(k_json_offs, dim3(js_grid(std::max(np, na))), dim3(GF_THREADS), 0, st, V);
	PGA_HIP(hipGetLastError());
	// ---- the wait behind the layout: the length of the file, where every key starts ----
	std::vector<gf_u64> h_tailoff(np);
	gf_u64 n_bytes = 0, sec[2] = {0, 0};
	fetch(&n_bytes, (const gf_u64*)s_items.off + V.n_items, 1, st);
	fetch(&sec[0], (const gf_u64*)s_items.off + 1 + V.n_pitems, 1, st); fetch(&sec[1], (const gf_u64*)s_items.off + 2 + V.n_pitems + V.n_bitems, 1, st);
	fetch((gf_u64*)out->path_off, (const gf_u64*)d_pathoff.p, np, st); fetch((gf_u64*)out->block_off, (const gf_u64*)d_blockoff.p, nb, st);
	fetch(h_tailoff.data(), (const gf_u64*)d_tailoff.p, np, st);
	PGA_HIP(hipEventRecord(ev_1.e, st));
	PGA_HIP(sync_stream(st));
	if (n_bytes >= (1ULL << 63)) js_fail("a file of 2^63 bytes or more");
	out->n_bytes = n_bytes;
	out->section_off[0] = 4; out->section_off[1] = sec[0] + (np ? 4 : 1) + 4; out->section_off[2] = sec[1] + (na ? 4 : 1) + 4;
	js_fill_table(J, blocks, paths, (const gf_u64*)out->block_off, h_tailoff.data());
	{ float ms = 0; PGA_HIP(hipEventElapsedTime(&ms, ev_0.e, ev_1.e)); g_js_ms[0] = ms; g_js_ms[1] = g_js_ms[2] = g_js_ms[3] = 0; }
	if (!sink) return;
	// ---- the tiles ----
	const uint64_t n_tiles = (n_bytes + tile_bytes - 1) / tile_bytes, cap = std::min<uint64_t>(n_bytes, tile_bytes);
	for (int b = 0; b < (n_tiles > 1 ? 2 : 1); ++b) { d_tile[b].alloc(cap); pin[b].p = (char*)pin_alloc(cap); }
	auto span = [&](uint64_t t, gf_u64 &a, gf_u64 &z) { a = t * tile_bytes; z = std::min<gf_u64>(n_bytes, a + tile_bytes); };
	auto launch = [&](uint64_t t) {
		const int b = (int)(t & 1);
		JsDev W = V;
		span(t, W.t0, W.t1);
		W.tile = d_tile[b].p;
		PGA_HIP(hipEventRecord(ev_ka[b].e, st));
		hipLaunchKernelGGL(k_json_tile, dim3((unsigned)std::min<uint64_t>(std::max<uint64_t>((W.t1 - W.t0) / (32 * GF_THREADS), 1), 2048)), dim3(GF_THREADS), 0, st, W);
		PGA_HIP(hipGetLastError());
		PGA_HIP(hipEventRecord(ev_kb[b].e, st));
	};
	size_t pi = 0, bi = 0;
	double ms_kern = 0, ms_fill = 0, ms_sink = 0;
	auto deliver = [&](uint64_t t) {                                        // tile t lies in its pinned block: the host's letters, then the sink
		gf_u64 a, z; span(t, a, z);
		const double c0 = now_ms();
		js_host_fill(J, blocks, cons, pin[t & 1].p, a, z, pi, bi);
		const double c1 = now_ms();
		const int rc = sink(ctx, pin[t & 1].p, (int64_t)(z - a));
		ms_fill += c1 - c0; ms_sink += now_ms() - c1;
		if (rc != 0) {
			(void)hipStreamSynchronize(st); (void)hipStreamSynchronize(sc);     // drain what is in flight: no further sink call
			js_fail("sink stopped the export");
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
	g_js_ms[1] = ms_kern; g_js_ms[2] = ms_fill; g_js_ms[3] = ms_sink;
}

} // namespace pga
