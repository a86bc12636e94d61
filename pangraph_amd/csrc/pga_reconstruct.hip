// pga_reconstruct.hip -- reconstruct (packages/pangraph/src/commands/reconstruct/reconstruct_run.rs:56-127) for all paths of a graph: blocks
// with their members' edit lists and the node chains of the paths in, every path's sequence out -- or, in verify mode, only whether it is
// the sequence the caller expects.
//   edits.rs:307-329          Edit::apply of a node's edits to its block's consensus
//   io/seq.rs:9-33            reverse_complement of a node on the reverse strand
//   reconstruct_run.rs:82-97  concatenation, the length check, rotate_right by the first node's position
// What runs where:
// The row table and the kernel are pga_rows.h: a path is a row whose pieces are its nodes.  What runs where:
//   host     list bookkeeping, O(nodes + edits): validation (all of it before anything is launched), every member's built length, and one
//            run table per path (row_piece_runs per node, on a few host threads).  Empty nodes contribute no run.
//   device   k_rows<true>, one thread per 16 written letters: the rotation and the mirrored index of reverse runs are on the load side,
//            the store is one aligned 16-byte vector; the comparison with the expected letters is fused (verify-only stores nothing)
// Paths are processed in chunks whose built letters stay under PGA_RECON_CHUNK_MB (default 2048; a longer single path is a chunk of its
// own).  Per chunk the device receives the runs, one copy of every consensus a node of the chunk reads, the slice of the insertion letters
// its members point into and, in verify mode, the expected letters.  The result does not depend on the chunking.
#include "pga_common.h"
#include "../../include/pga_align.h"
#include "pga_rows.h"

namespace pga {

constexpr int RC_BUSY_FAMILY = 15;                           // pga_busy_end (include/pga_align.h)

static size_t recon_chunk_bytes()
{
	const char *e = getenv("PGA_RECON_CHUNK_MB");
	const double mb = e ? atof(e) : 2048.0;
	return (size_t)(std::max(mb, 1.0) * (double)(1u << 20));
}

void reconstruct_host(int64_t n_blocks, const pga_rc_block_t *blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss,
                      const char *ins_seq, int64_t n_paths, const pga_recon_path_t *paths, const pga_recon_node_t *nodes, const char *const *expected,
                      const uint64_t *expected_len, pga_recon_res_t *res, char **out_seq)
{
	auto fail = [](const std::string &what) { throw std::runtime_error("pga_reconstruct: " + what); };
	const bool verify = expected != nullptr, write = out_seq != nullptr;
	// ---- offsets and validation: everything that fails the call does so here, before anything is launched ----
	const int n_threads = range_threads();
	RowGraph G;
	row_graph_init(G, "pga_reconstruct", n_blocks, blocks, members, subs, dels, inss, ins_seq, false, n_threads);
	if (n_paths && (!paths || !res)) fail("null path list");
	if (verify && !expected_len) fail("expected sequences without their lengths");
	std::vector<uint64_t> node_first((size_t)n_paths + 1, 0);
	for (int64_t p = 0; p < n_paths; ++p) node_first[p + 1] = node_first[p] + paths[p].n_nodes;
	if (node_first[n_paths] && !nodes) fail("null node list");
	// per path: the built length, the status as far as the host knows it, the place in the output (every path at a multiple of 16)
	std::vector<uint64_t> len((size_t)n_paths), dst((size_t)n_paths + 1, 0);
	std::vector<int32_t> status((size_t)n_paths, 0);
	for (int64_t p = 0; p < n_paths; ++p) {
		uint64_t l = 0;
		for (uint64_t k = node_first[p]; k < node_first[p + 1]; ++k) {
			if (nodes[k].member >= G.n_mem) fail("node names a member that does not exist (path " + std::to_string(p) + ", node " + std::to_string(k - node_first[p]) + ")");
			l += G.mem_len[nodes[k].member];
			if (l > (1ULL << 31)) fail("path longer than 2^31 letters (path " + std::to_string(p) + ")");
		}
		if (verify && expected_len[p] && !expected[p]) fail("null expected sequence with a non-zero length (path " + std::to_string(p) + ")");
		len[p] = l;
		if (paths[p].n_nodes) {                                               // (a path without nodes: Seq::new(), nothing is checked)
			if (l != paths[p].tot_len) status[p] = 1;
			else if (paths[p].first_pos > l) status[p] = 4;
		}
		if (status[p] == 0 && verify && expected_len[p] != l) status[p] = 5;
		dst[p + 1] = dst[p] + row_pad(l);
	}
	struct Owned { char *p = nullptr; ~Owned() { free(p); } } obuf;
	if (write) { obuf.p = (char*)malloc((size_t)dst[n_paths] + 1); if (!obuf.p) fail("out of host memory"); }
	StreamLease stream;
	hipStream_t st = stream.s;
	const size_t chunk_cap = recon_chunk_bytes();
	int64_t p0 = 0;
	while (p0 < n_paths) {
		// ---- the chunk: paths p0 .. p1 ----
		int64_t p1 = p0 + 1;
		while (p1 < n_paths && dst[p1 + 1] - dst[p0] <= chunk_cap) ++p1;
		const uint64_t k0 = node_first[p0], k1 = node_first[p1], chunk_letters = dst[p1] - dst[p0];
		std::vector<uint32_t> flags((size_t)(p1 - p0), 0u);
		std::vector<unsigned long long> first((size_t)(p1 - p0), ~0ULL), count((size_t)(p1 - p0), 0ULL);
		if (chunk_letters) {
			// one copy of every consensus a node reads, the range of the insertion letters the members point into, every node's offset in its path
			RowTable T;
			std::vector<uint32_t> node_at((size_t)(k1 - k0));
			for (int64_t p = p0; p < p1; ++p) {
				uint32_t o = 0;
				for (uint64_t k = node_first[p]; k < node_first[p + 1]; ++k) { node_at[k - k0] = o; o += G.mem_len[nodes[k].member]; row_place(G, nodes[k].member, T); }
			}
			// ---- the runs of every node, in node order (a few host threads, nodes are independent) ----
			std::vector<std::vector<RowRun>> part((size_t)n_threads);
			std::vector<uint32_t> node_runs((size_t)(k1 - k0), 0u);
			thread_ranges(k1 - k0, n_threads, [&](int t, uint64_t a, uint64_t z) {
				PreparedEdit P; std::vector<PrSeg> segs; std::vector<RowRun> &out = part[t];
				for (uint64_t k = k0 + a; k < k0 + z; ++k) {
					const size_t had = out.size();
					row_piece_runs(G, RowPiece{nodes[k].member, nodes[k].reverse ? 1u : 0u, 0u}, node_at[k - k0], T.cons_at.find(G.blk_of[nodes[k].member])->second, out, P, segs);
					node_runs[k - k0] = (uint32_t)(out.size() - had);
				}
			});
			for (auto &v : part) { T.runs.insert(T.runs.end(), v.begin(), v.end()); std::vector<RowRun>().swap(v); }
			uint64_t run_off = 0;
			for (int64_t p = p0; p < p1; ++p) {
				uint64_t nr = 0;
				for (uint64_t k = node_first[p]; k < node_first[p + 1]; ++k) nr += node_runs[k - k0];
				if (len[p]) {                                                     // (unit0 * 16 == dst[p] - dst[p0]: a path without letters takes no bytes)
					T.jobs.push_back(RowJob{run_off, T.units, (uint32_t)nr, (uint32_t)len[p], status[p] == 1 || status[p] == 4 ? 0u : (uint32_t)paths[p].first_pos,
					                        verify && status[p] == 0 ? 1u : 0u});
					T.job_row.push_back((uint64_t)p);
					T.units += row_pad(len[p]) / ROW_LETTERS;
				}
				run_off += nr;
			}
			if (run_off != T.runs.size() || T.units * ROW_LETTERS != chunk_letters) fail("internal: the run tables do not add up");
			const size_t n_jobs = T.jobs.size();
			if (n_jobs >= (1ULL << 31)) fail("more than 2^31 paths in one chunk");
			// ---- the device ----
			const uint64_t il = T.ins_lo < T.ins_hi ? T.ins_lo : 0, ih = T.ins_lo < T.ins_hi ? T.ins_hi : 0;
			DBuf<char> d_cons(T.cons.size() + 16), d_iseq(ih - il + 16), d_out, d_exp;
			if (!T.cons.empty()) PGA_HIP(hipMemcpyAsync(d_cons.p, T.cons.data(), T.cons.size(), hipMemcpyHostToDevice, st));
			if (ih > il) PGA_HIP(hipMemcpyAsync(d_iseq.p, ins_seq + il, ih - il, hipMemcpyHostToDevice, st));
			if (write) d_out.alloc(chunk_letters);
			if (verify) {
				d_exp.alloc(chunk_letters);
				for (size_t j = 0; j < n_jobs; ++j) if (T.jobs[j].cmp) PGA_HIP(hipMemcpyAsync(d_exp.p + T.jobs[j].unit0 * ROW_LETTERS, expected[T.job_row[j]], T.jobs[j].len, hipMemcpyHostToDevice, st));
			}
			DBuf<RowJob> d_jobs; d_jobs.upload(T.jobs, st);
			DBuf<RowRun> d_runs; d_runs.upload(T.runs, st);
			DBuf<uint32_t> d_flags(n_jobs); d_flags.zero(st);
			DBuf<unsigned long long> d_first(n_jobs), d_count(n_jobs);
			PGA_HIP(hipMemsetAsync(d_first.p, 0xff, n_jobs * sizeof(unsigned long long), st));
			d_count.zero(st);
			const unsigned grid = (unsigned)std::min<uint64_t>((T.units + ROW_THREADS - 1) / ROW_THREADS, 2048);
			{
				EventTimer et(st);
				hipLaunchKernelGGL(k_rows<true>, dim3(grid), dim3(ROW_THREADS), 0, st, d_jobs.p, (int)n_jobs, (uint64_t)0, T.units, d_runs.p, d_cons.p, d_iseq.p, il,
				                   write ? d_out.p : nullptr, d_flags.p, ROW_GAP, verify ? d_exp.p : nullptr, d_first.p, d_count.p);
				PGA_HIP(hipGetLastError());
				et.finish(RC_BUSY_FAMILY);                                          // (synchronises: the host buffers above may go)
			}
			Downloads dl(st);
			std::vector<uint32_t> j_flags; std::vector<unsigned long long> j_first, j_count;
			dl.add(j_flags, d_flags.p, n_jobs);
			if (verify) { dl.add(j_first, d_first.p, n_jobs); dl.add(j_count, d_count.p, n_jobs); }
			if (write) PGA_HIP(hipMemcpyAsync(obuf.p + dst[p0], d_out.p, chunk_letters, hipMemcpyDeviceToHost, st));
			dl.wait();
			PGA_HIP(sync_stream(st));
			for (size_t j = 0; j < n_jobs; ++j) {
				const size_t q = (size_t)((int64_t)T.job_row[j] - p0);
				flags[q] = j_flags[j];
				if (verify && T.jobs[j].cmp) { first[q] = j_first[j]; count[q] = j_count[j]; }
			}
		}
		// ---- the verdicts, in the order of include/pga_align.h: 2, 3, then what the host knew (1, 4, 5) ----
		for (int64_t p = p0; p < p1; ++p) {
			const size_t q = (size_t)(p - p0);
			pga_recon_res_t &o = res[p];
			memset(&o, 0, sizeof(o));
			o.status = (flags[q] & ROW_BAD_COMP) ? 2 : (flags[q] & ROW_GAP) ? 3 : status[p];
			o.len = len[p];
			o.seq_off = write && o.status == 0 ? dst[p] : 0;
			o.first_mismatch = -1; o.n_mismatch = 0;
			if (verify && o.status == 0 && count[q]) { o.first_mismatch = (int64_t)first[q]; o.n_mismatch = (int64_t)count[q]; }
		}
		p0 = p1;
	}
	if (write) { *out_seq = obuf.p; obuf.p = nullptr; }
}

} // namespace pga
