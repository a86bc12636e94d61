// pga_detach_idx.h -- the index arithmetic of pga_detach.hip (detach_unaligned.rs:24-114 over Edit::aligned_count, edits.rs:439-442): the
// member decision, what the offsets sum, the pack kernel, and the host side (the same decision, the orphans' rows, the block id).  None of it
// uses a wave intrinsic, so all of this compiles under hipcc and, with dev/emu/hip_emu.h included first, under g++ -std=c++17 -DPGA_EMU
// (tests/emu/detach_emu.cpp runs it against a direct scalar construction).  The one-wave scans of pga_detach.hip (wave_incl_u64 of pga_wave.h) are not in here; XXH64 is pga_xxh64.h.
//
// An input member m is KEPT or UNALIGNED: unaligned iff the 64-bit sum of its deletion lengths reaches its block's cons_len (a block with
// cons_len == 0: every member).  Five quantities are summed over the members in input order (dt_scan_value), exclusive:
//   DT_KEPT    1 per kept member        -> the member's index in out->members
//   DT_SUB / DT_DEL / DT_INS            -> the first entry of a kept member's list in out->subs / dels / inss
//   DT_ORPHAN  1 per unaligned member   -> its rank k: orphans[k], block n_blocks + k, member (all kept) + k
#pragma once
#include "../../include/pga_align.h"
#include "pga_rows.h"
#include "pga_xxh64.h"
#include <algorithm>

namespace pga {

typedef unsigned long long dt_u64;
constexpr int DT_THREADS = 256, DT_WAVES = DT_THREADS / 64;
enum { DT_KEPT = 0, DT_SUB = 1, DT_DEL = 2, DT_INS = 3, DT_ORPHAN = 4, DT_SCANS = 5 };

struct DtDev {
	uint64_t n_mem, n_blocks_in, cap_orphans;                 // cap_orphans: entries of `orphans` (what the host counted)
	const pga_rc_member_t *members; const uint32_t *cons_len;   // per member: its counts, its block's cons_len
	const uint64_t *sub_off, *del_off, *ins_off;                // per member (n_mem + 1 entries): its first entry in subs / dels / inss
	const pga_sub_t *subs; const pga_del_t *dels; const pga_ins_t *inss;
	const pga_detach_member_t *who;
	dt_u64 *del_sum;                                            // per member: the sum of its deletion lengths
	uint32_t *unal;                                             // per member: 1 unaligned, 0 kept
	dt_u64 *off;                                                // DT_SCANS x (n_mem + 1): exclusive sums, entry n_mem the total
};

// Edit::aligned_count(cons_len) == 0: cons_len.saturating_sub(sum) == 0
__host__ __device__ inline uint32_t dt_unaligned(dt_u64 del_sum, uint32_t cons_len) { return del_sum >= (dt_u64)cons_len ? 1u : 0u; }
// what scan q adds for member m
__host__ __device__ inline dt_u64 dt_scan_value(const pga_rc_member_t &M, uint32_t unal, int q)
{
	if (q == DT_ORPHAN) return unal;
	if (unal) return 0ULL;
	return q == DT_KEPT ? 1ULL : q == DT_SUB ? (dt_u64)M.n_subs : q == DT_DEL ? (dt_u64)M.n_dels : (dt_u64)M.n_inss;
}
__host__ __device__ inline const dt_u64 *dt_off(const DtDev &V, int q) { return V.off + (uint64_t)q * (V.n_mem + 1); }

// pass 1, one wave per member, lanes stride over its deletions: the sum in the wave's LDS word (one atomic per lane that saw a length), then,
// behind a barrier, lane 0 writes it out with the decision.  Every wave of a workgroup takes the same number of turns, so the barriers are
// reached by all of them.
__global__ __launch_bounds__(DT_THREADS) void k_detach_count(DtDev V)
{
	__shared__ dt_u64 s_sum[DT_WAVES];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (uint64_t m0 = (uint64_t)blockIdx.x * DT_WAVES; m0 < V.n_mem; m0 += (uint64_t)gridDim.x * DT_WAVES) {
		const uint64_t m = m0 + wave;
		if (lane == 0) s_sum[wave] = 0;
		__syncthreads();
		if (m < V.n_mem) {
			const uint64_t d0 = V.del_off[m];
			const uint32_t n = V.members[m].n_dels;
			dt_u64 part = 0;
			for (uint32_t t = lane; t < n; t += 64) part += V.dels[d0 + t].len;
			if (part) atomicAdd(&s_sum[wave], part);
		}
		__syncthreads();
		if (m < V.n_mem && lane == 0) { const dt_u64 sum = s_sum[wave]; V.del_sum[m] = sum; V.unal[m] = dt_unaligned(sum, V.cons_len[m]); }
	}
}

// pass 2 (behind the scans), one wave per member, lanes over entries: a kept member's record, map entry and three lists to their new
// places; an unaligned member's empty record behind all kept ones, its map entry and its orphan record (member, node_id, block; len,
// block_id and status are the host's, from the row table and the letters).
__global__ __launch_bounds__(DT_THREADS) void k_detach_pack(DtDev V, pga_rc_member_t *o_members, pga_sub_t *o_subs, pga_del_t *o_dels, pga_ins_t *o_inss,
                                                            int64_t *member_map, pga_detach_orphan_t *orphans)
{
	const uint32_t lane = threadIdx.x & 63u;
	const dt_u64 *kept = dt_off(V, DT_KEPT), *so = dt_off(V, DT_SUB), *dl = dt_off(V, DT_DEL), *io = dt_off(V, DT_INS), *orph = dt_off(V, DT_ORPHAN);
	const dt_u64 n_kept = kept[V.n_mem];
	for (uint64_t m = (uint64_t)blockIdx.x * DT_WAVES + (threadIdx.x >> 6); m < V.n_mem; m += (uint64_t)gridDim.x * DT_WAVES) {
		const pga_rc_member_t M = V.members[m];
		if (V.unal[m]) {
			const dt_u64 k = orph[m];
			if (lane == 0) {
				o_members[n_kept + k] = pga_rc_member_t{0u, 0u, 0u};
				member_map[m] = (int64_t)(n_kept + k);
				if (k < V.cap_orphans) orphans[k] = pga_detach_orphan_t{m, V.who[m].node_id, 0ULL, (uint32_t)(V.n_blocks_in + k), 0u, 0, 0};
			}
			continue;
		}
		if (lane == 0) { o_members[kept[m]] = M; member_map[m] = (int64_t)kept[m]; }
		const uint64_t s0 = V.sub_off[m], d0 = V.del_off[m], i0 = V.ins_off[m];
		for (uint32_t t = lane; t < M.n_subs; t += 64) o_subs[so[m] + t] = V.subs[s0 + t];
		for (uint32_t t = lane; t < M.n_dels; t += 64) o_dels[dl[m] + t] = V.dels[d0 + t];
		for (uint32_t t = lane; t < M.n_inss; t += 64) o_inss[io[m] + t] = V.inss[i0 + t];
	}
}

// ---------------------------------------------------------------- host side
// id((node_id, &seq)): node_id and the length as little-endian u64, then the letters; buf is scratch
static uint64_t dt_block_id(uint64_t node_id, const char *seq, uint64_t len, std::vector<uint8_t> &buf)
{
	buf.resize((size_t)(16 + len));
	for (int i = 0; i < 8; ++i) { buf[i] = (uint8_t)(node_id >> (8 * i)); buf[8 + i] = (uint8_t)(len >> (8 * i)); }
	if (len) memcpy(buf.data() + 16, seq, (size_t)len);
	return xxh64_bytes(buf.data(), 16 + len, 0);
}

// what the host works out before anything is launched: the decision for every member (so that runs are built for orphans only and
// nothing has to come back from the device before the row table exists), the totals the output is allocated by, the orphans' rows
struct DtTables {
	std::vector<uint8_t> unal;                                  // per member
	std::vector<uint64_t> orphans;                              // their members, in push order
	std::vector<uint32_t> kept_in;                              // per block: members kept
	uint64_t tot[DT_SCANS] = {0, 0, 0, 0, 0};
	RowTable rows;                                              // one row per orphan with letters; rows.job_row: its rank
	std::vector<uint32_t> len; std::vector<uint64_t> cons_off;  // per orphan: its length, its letters in out->cons
};

// G: row_graph_init in ALIGNED mode (the lists are checked, nothing is prepared).  The members it detaches are then prepared one by one and
// G is switched to unaligned mode for row_piece_runs.  Throws std::runtime_error on what fails the call.
static void dt_build_tables(RowGraph &G, const pga_detach_member_t *who, int n_threads, DtTables &T)
{
	auto fail = [](const std::string &what) { throw std::runtime_error("pga_detach_unaligned: " + what); };
	const uint64_t n_mem = G.n_mem;
	if (n_mem && !who) fail("null node list with members present");
	T.unal.assign((size_t)n_mem, 0);
	thread_ranges(n_mem, n_threads, [&](int, uint64_t m0, uint64_t m1) {
		for (uint64_t m = m0; m < m1; ++m) {
			dt_u64 sum = 0;
			for (uint64_t t = G.del_off[m]; t < G.del_off[m + 1]; ++t) sum += G.dels[t].len;
			T.unal[m] = (uint8_t)dt_unaligned(sum, G.blocks[G.blk_of[m]].cons_len);
			if (!G.ins_seq) for (uint64_t t = G.ins_off[m]; t < G.ins_off[m + 1]; ++t) if (G.inss[t].len) fail("null insertion letters with a non-zero length (member " + std::to_string(m) + ")");
		}
	});
	T.kept_in.assign((size_t)G.n_blocks, 0);
	for (uint64_t m = 0; m < n_mem; ++m) {
		const pga_rc_member_t &M = G.members[m];
		for (int q = 0; q < DT_SCANS; ++q) T.tot[q] += dt_scan_value(M, T.unal[m], q);
		if (T.unal[m]) T.orphans.push_back(m); else ++T.kept_in[G.blk_of[m]];
	}
	if ((uint64_t)G.n_blocks + T.orphans.size() >= (1ULL << 32)) fail("more than 2^32 blocks afterwards");
	// ---- the orphans' rows: one piece each, unaligned mode ----
	G.aligned = false;
	PreparedEdit P; std::vector<PrSeg> segs;
	T.len.assign(T.orphans.size(), 0); T.cons_off.assign(T.orphans.size(), 0);
	for (size_t k = 0; k < T.orphans.size(); ++k) {
		const uint64_t m = T.orphans[k];
		const uint32_t L = G.blocks[G.blk_of[m]].cons_len;
		uint64_t letters = 0;
		for (uint64_t t = G.ins_off[m]; t < G.ins_off[m + 1]; ++t) letters += G.inss[t].len;
		if ((uint64_t)L + letters > (1ULL << 31)) fail("member longer than 2^31 letters (member " + std::to_string(m) + ")");
		G.mem_len[m] = prepare_edit(G.subs + G.sub_off[m], G.members[m].n_subs, G.dels + G.del_off[m], G.members[m].n_dels, G.inss + G.ins_off[m], G.members[m].n_inss, G.ins_seq, L, P);
		const RowPiece piece{m, who[m].reverse ? 1u : 0u, 0u};
		T.cons_off[k] = T.rows.units * ROW_LETTERS;
		T.len[k] = (uint32_t)row_append_row(G, (uint64_t)k, &piece, 1, T.rows, P, segs);
	}
	if (T.rows.jobs.size() >= (1ULL << 31)) fail("more than 2^31 rows");
}

} // namespace pga
