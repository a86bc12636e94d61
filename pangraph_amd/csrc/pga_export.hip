// pga_export.hip -- the two exports of a finished graph on the device, streamed: pga_block_sequences (export block-sequences,
// PangraphBlock::sequences, pangraph_block.rs:135-189: one row per member) and pga_core_alignment (export core-genome, core_block_aln with
// concatenate_records, export_core_genome.rs:53-141: one row per path, its pieces the core blocks in guide order with the guide's strand).
// The row table and the kernel are pga_rows.h.  What runs where:
//   host     validation and the core selection (all of it before anything is launched), the row tables, chunk by chunk
//   device   k_rows<false> over the unit space of a chunk
// Rows are taken in delivery order (`order`, or their own) and grouped into CHUNKS whose run tables stay under PGA_EXPORT_RUNS_KB (default
// 262144; a single larger row is a chunk of its own).  Per chunk the device receives the runs, one copy of every consensus a piece reads and
// the slice of the insertion letters the pieces point into.
//   verdict mode (no sink)  one grid-stride launch per chunk with out == nullptr: only the flags come back.
//   sink mode               the unit space of a chunk is cut into TILES of PGA_EXPORT_TILE_KB (default 16384, the knee of the pinned chunks,
//                           DESIGN.md section 8).  Two device tiles and two pinned blocks (pin_alloc): while the sink consumes tile t-1 on the
//                           calling thread, tile t is copied into its pinned block on the copy stream and the kernel writes tile t+1 on the
//                           kernel stream.  A device tile is written again only after the host has seen its copy complete, a pinned block
//                           only after the sink has returned.  Letters go from the device into pinned blocks and nowhere else, and the
//                           library holds no row buffer.
// Neither knob changes a result.
#include "pga_common.h"
#include "pga_graph_host.h"
#include "../../include/pga_align.h"
#include "pga_rows.h"

namespace pga {

constexpr int EX_BUSY_FAMILY = 16;                           // pga_busy_end (include/pga_align.h): the first family behind those of pga_stats_t

namespace {
struct ExPin { char *p = nullptr; uint64_t cap = 0; ~ExPin() { pin_free(p); } };
}

// rows[r] = pieces[piece_first[r] .. piece_first[r + 1]); res[r] for every row; rows are built and delivered in `order`
static void export_rows(const std::string &who, const RowGraph &G, uint64_t n_rows, const std::vector<uint64_t> &piece_first, const std::vector<RowPiece> &pieces,
                        const uint64_t *order, pga_export_res_t *res, pga_export_sink_t sink, void *ctx)
{
	auto fail = [&](const std::string &what) { throw std::runtime_error(who + ": " + what); };
	// ---- everything that fails the call does so here, before anything is launched ----
	if (n_rows && !res) fail("null result list");
	if (order) {
		std::vector<char> seen((size_t)n_rows, 0);
		for (uint64_t k = 0; k < n_rows; ++k) {
			if (order[k] >= n_rows || seen[order[k]]) fail("order is not a permutation of the rows (entry " + std::to_string(k) + ")");
			seen[order[k]] = 1;
		}
	}
	for (uint64_t r = 0; r < n_rows; ++r) {
		uint64_t l = 0;
		for (uint64_t q = piece_first[r]; q < piece_first[r + 1]; ++q) { l += G.mem_len[pieces[q].member]; if (l > (1ULL << 31)) fail("row over 2^31 letters (row " + std::to_string(r) + ")"); }
		res[r].status = 0; res[r].pad = 0; res[r].len = l;
	}
	const uint64_t tile_units = export_tile_bytes(fail) / ROW_LETTERS;
	const uint64_t runs_cap = knob_kb(fail, "PGA_EXPORT_RUNS_KB", 262144, 1) * 1024 / sizeof(RowRun);
	const uint32_t gap_flag = G.aligned ? 0u : ROW_GAP;

	// (declared before the streams: the streams are drained first when the scope is left, by a throw too)
	DBuf<char> d_cons, d_iseq, d_tile[2];
	DBuf<RowJob> d_jobs; DBuf<RowRun> d_runs; DBuf<uint32_t> d_flags;
	ExPin pin[2];
	RowTable T; PreparedEdit P; std::vector<PrSeg> segs_scratch;
	std::vector<pga_export_seg_t> segs;
	std::vector<uint32_t> flags;
	Event ev_ka[2], ev_kb[2], ev_c[2];                                  // per tile buffer: before and behind its kernel, behind its copy
	StreamLease s_kern, s_copy;                                           // (release drains the stream)
	const hipStream_t sk = s_kern.s, sc = s_copy.s;

	uint64_t k = 0;
	while (k < n_rows) {
		// ---- the chunk: rows in delivery order while the run table stays under the cap ----
		T.clear();
		for (uint64_t in_chunk = 0; k < n_rows; ++k, ++in_chunk) {
			const uint64_t r = order ? order[k] : k;
			const RowTable::Mark mk = T.mark();
			row_append_row(G, r, pieces.data() + piece_first[r], piece_first[r + 1] - piece_first[r], T, P, segs_scratch);
			if (T.runs.size() > runs_cap && in_chunk) { T.undo(mk); break; }
		}
		if (T.jobs.empty()) continue;
		if (T.jobs.size() >= (1ULL << 31)) fail("more than 2^31 rows in one chunk");
		const uint64_t units = T.units, n_jobs = T.jobs.size();
		const uint64_t ins_lo = T.ins_lo < T.ins_hi ? T.ins_lo : 0, ins_n = T.ins_lo < T.ins_hi ? T.ins_hi - T.ins_lo : 0;
		d_cons.alloc(T.cons.size() + 16); d_iseq.alloc(ins_n + 16);
		if (!T.cons.empty()) PGA_HIP(hipMemcpyAsync(d_cons.p, T.cons.data(), T.cons.size(), hipMemcpyHostToDevice, sk));
		if (ins_n) PGA_HIP(hipMemcpyAsync(d_iseq.p, G.ins_seq + ins_lo, ins_n, hipMemcpyHostToDevice, sk));
		d_jobs.upload(T.jobs, sk); d_runs.upload(T.runs, sk);
		d_flags.alloc(n_jobs); d_flags.zero(sk);
		if (!sink) {
			const unsigned grid = (unsigned)std::min<uint64_t>((units + ROW_THREADS - 1) / ROW_THREADS, 2048);
			EventTimer et(sk);
			hipLaunchKernelGGL(k_rows<false>, dim3(grid), dim3(ROW_THREADS), 0, sk, d_jobs.p, (int)n_jobs, (uint64_t)0, units, d_runs.p, d_cons.p, d_iseq.p, ins_lo,
			                   (char*)nullptr, d_flags.p, gap_flag, (const char*)nullptr, (unsigned long long*)nullptr, (unsigned long long*)nullptr);
			PGA_HIP(hipGetLastError());
			et.finish(EX_BUSY_FAMILY);
		} else {
			const uint64_t n_tiles = (units + tile_units - 1) / tile_units, tile_bytes = std::min(units, tile_units) * ROW_LETTERS;
			for (int b = 0; b < (n_tiles > 1 ? 2 : 1); ++b) {                   // (nothing of an earlier chunk is in flight any more)
				d_tile[b].alloc(tile_bytes);
				if (pin[b].cap < tile_bytes) { pin_free(pin[b].p); pin[b].p = nullptr; pin[b].cap = 0; pin[b].p = (char*)pin_alloc(tile_bytes); pin[b].cap = tile_bytes; }
			}
			auto span = [&](uint64_t t, uint64_t &a, uint64_t &z) { a = t * tile_units; z = std::min(units, a + tile_units); };
			auto launch = [&](uint64_t t) {
				uint64_t a, z; span(t, a, z);
				const int b = (int)(t & 1);
				PGA_HIP(hipEventRecord(ev_ka[b].e, sk));
				hipLaunchKernelGGL(k_rows<false>, dim3((unsigned)((z - a + ROW_THREADS - 1) / ROW_THREADS)), dim3(ROW_THREADS), 0, sk, d_jobs.p, (int)n_jobs, a, z, d_runs.p,
				                   d_cons.p, d_iseq.p, ins_lo, d_tile[b].p, d_flags.p, gap_flag, (const char*)nullptr, (unsigned long long*)nullptr, (unsigned long long*)nullptr);
				PGA_HIP(hipGetLastError());
				PGA_HIP(hipEventRecord(ev_kb[b].e, sk));
			};
			size_t jc = 0;                                                      // the first job that reaches into the tile to deliver
			auto deliver = [&](uint64_t t) {                                    // tile t lies in its pinned block: its segments, then the sink
				uint64_t a, z; span(t, a, z);
				segs.clear();
				while (jc < n_jobs) {
					const RowJob &J = T.jobs[jc];
					if (J.unit0 >= z) break;
					const uint64_t from = std::max(J.unit0, a), row_off = (from - J.unit0) * ROW_LETTERS, row_end = std::min<uint64_t>(J.len, (z - J.unit0) * ROW_LETTERS);
					segs.push_back(pga_export_seg_t{T.job_row[jc], row_off, (from - a) * ROW_LETTERS, (uint32_t)(row_end - row_off), 0u});
					if (J.unit0 + row_pad(J.len) / ROW_LETTERS > z) break;              // the row goes on in the next tile
					++jc;
				}
				if (sink(ctx, (int64_t)segs.size(), segs.data(), pin[t & 1].p) != 0) {
					(void)hipStreamSynchronize(sk); (void)hipStreamSynchronize(sc);   // drain what is in flight: no further sink call
					fail("sink stopped the export");
				}
			};
			auto copied = [&](uint64_t t) {                                     // waits for the copy of tile t; its kernel is over then too
				PGA_HIP(sync_event(ev_c[t & 1].e));
				busy_note(EX_BUSY_FAMILY, ev_ka[t & 1].e, ev_kb[t & 1].e);
			};
			launch(0);
			for (uint64_t t = 0; t < n_tiles; ++t) {
				uint64_t a, z; span(t, a, z);
				const int b = (int)(t & 1);
				PGA_HIP(hipStreamWaitEvent(sc, ev_kb[b].e, 0));
				PGA_HIP(hipMemcpyAsync(pin[b].p, d_tile[b].p, (z - a) * ROW_LETTERS, hipMemcpyDeviceToHost, sc));   // (the sink of tile t-2 has returned)
				PGA_HIP(hipEventRecord(ev_c[b].e, sc));
				if (t >= 1) copied(t - 1);
				if (t + 1 < n_tiles) launch(t + 1);                               // (into the device tile of t-1, whose copy is complete)
				if (t >= 1) deliver(t - 1);
			}
			copied(n_tiles - 1);
			deliver(n_tiles - 1);
		}
		{
			Downloads dl(sk);
			dl.add(flags, d_flags.p, n_jobs);
			dl.wait();
		}
		PGA_HIP(sync_stream(sk));                                             // (the chunk's host tables may go)
		for (size_t j = 0; j < n_jobs; ++j) res[T.job_row[j]].status = (flags[j] & ROW_BAD_COMP) ? 2 : (flags[j] & ROW_GAP) ? 3 : 0;
	}
}

void block_sequences_host(int64_t n_blocks, const pga_rc_block_t *blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss,
                          const char *ins_seq, int aligned, const uint64_t *order, pga_export_res_t *res, pga_export_sink_t sink, void *ctx)
{
	const std::string who = "pga_block_sequences";
	RowGraph G;
	row_graph_init(G, who, n_blocks, blocks, members, subs, dels, inss, ins_seq, aligned != 0, 1);
	std::vector<uint64_t> piece_first(G.n_mem + 1);
	std::vector<RowPiece> pieces(G.n_mem);
	for (uint64_t m = 0; m < G.n_mem; ++m) { piece_first[m] = m; pieces[m] = RowPiece{m, 0u, 0u}; }
	piece_first[G.n_mem] = G.n_mem;
	export_rows(who, G, G.n_mem, piece_first, pieces, order, res, sink, ctx);
}

void core_alignment_host(int64_t n_blocks, const pga_rc_block_t *blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss,
                         const char *ins_seq, const uint32_t *member_path, int64_t n_paths, int64_t guide_path, int64_t n_guide_nodes, const pga_recon_node_t *guide_nodes,
                         int aligned, const uint64_t *order, pga_export_res_t *res, pga_core_block_t **core_out, int64_t *n_core_out, pga_export_sink_t sink, void *ctx)
{
	const std::string who = "pga_core_alignment";
	auto fail = [&](const std::string &what) { throw std::runtime_error(who + ": " + what); };
	RowGraph G;
	row_graph_init(G, who, n_blocks, blocks, members, subs, dels, inss, ins_seq, aligned != 0, 1);
	if (n_paths < 0 || n_guide_nodes < 0) fail("negative count");
	std::vector<pga_core_block_t> core;
	std::vector<uint64_t> piece_first((size_t)n_paths + 1, 0);
	std::vector<RowPiece> pieces;
	if (n_paths > 0) {
		if (n_paths >= (1LL << 32)) fail("more than 2^32 paths");
		if (G.n_mem && !member_path) fail("null member_path");
		if (n_guide_nodes && !guide_nodes) fail("null guide node list");
		for (uint64_t m = 0; m < G.n_mem; ++m) if (member_path[m] >= (uint64_t)n_paths) fail("member_path names a path that does not exist (member " + std::to_string(m) + ")");
		if (guide_path < 0 || guide_path >= n_paths) fail("guide_path names a path that does not exist");
		// core_block_ids (pangraph.rs:235-255): the blocks present exactly once in each path = as many members as paths, no path twice
		std::vector<char> is_core((size_t)n_blocks, 0);
		std::vector<int64_t> stamp((size_t)n_paths, -1);
		uint64_t n_core_ids = 0;
		for (int64_t b = 0; b < n_blocks; ++b) {
			if (blocks[b].n_members != (uint64_t)n_paths) continue;
			bool once = true;
			for (uint64_t m = G.mem_first[b]; m < G.mem_first[b + 1] && once; ++m) { if (stamp[member_path[m]] == b) once = false; stamp[member_path[m]] = b; }
			if (once) { is_core[b] = 1; ++n_core_ids; }
		}
		uint64_t col = 0;
		for (int64_t k = 0; k < n_guide_nodes; ++k) {
			const uint64_t m = guide_nodes[k].member;
			if (m >= G.n_mem) fail("guide node names a member that does not exist (node " + std::to_string(k) + ")");
			if (member_path[m] != (uint64_t)guide_path) fail("guide node whose member is not on guide_path (node " + std::to_string(k) + ")");
			const uint32_t b = G.blk_of[m];
			if (!is_core[b]) continue;
			if (is_core[b] == 2) fail("core block named twice by the guide nodes (block " + std::to_string(b) + ")");
			is_core[b] = 2;
			core.push_back(pga_core_block_t{b, guide_nodes[k].reverse ? 1 : 0, col, blocks[b].cons_len, 0u});
			col += blocks[b].cons_len;
		}
		if (core.size() != n_core_ids) fail("core block not named by the guide nodes");
		// row p: the member of every core block that lies on path p, in guide order
		pieces.resize(core.size() * (size_t)n_paths);
		for (size_t c = 0; c < core.size(); ++c)
			for (uint64_t m = G.mem_first[core[c].block]; m < G.mem_first[core[c].block + 1]; ++m)
				pieces[(size_t)member_path[m] * core.size() + c] = RowPiece{m, (uint32_t)core[c].reverse, 0u};
		for (int64_t p = 0; p <= n_paths; ++p) piece_first[p] = (uint64_t)p * core.size();
	}
	export_rows(who, G, (uint64_t)n_paths, piece_first, pieces, order, res, sink, ctx);
	pga_core_block_t *out = (pga_core_block_t*)malloc((core.size() ? core.size() : 1) * sizeof(pga_core_block_t));
	if (!out) fail("out of host memory");
	if (!core.empty()) memcpy(out, core.data(), core.size() * sizeof(pga_core_block_t));
	*core_out = out; *n_core_out = (int64_t)core.size();
}

} // namespace pga
