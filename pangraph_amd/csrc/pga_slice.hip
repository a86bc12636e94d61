// pga_slice.hip -- block_slice (packages/pangraph/src/pangraph/slice.rs:12-202) for every interval of every block a merge cuts
// (reweave.rs:342-402 split_block, called block after block by reweave.rs:427-438): consensus lengths, interval tables, old nodes and
// edit lists in; per (block, interval) the kept members with their sliced edits, coordinates, new position and strand, and the members
// whose slice is empty (Edit::is_empty_alignment, edits.rs:351-367) out.
// The reference lets every interval scan every list of every member again.  Here an EDIT finds its interval: the intervals of a block are
// sorted and disjoint, so a substitution or an insertion belongs to at most one of them and a deletion to a contiguous range, both found by
// binary search.  A "pair" is one (block, interval, member); pairs are numbered in that order, which is the order of the output.
//   host              validation, O(edits); the block and member tables; one upload of every list
//   k_slice_count     one wave per member: per pair the number of sliced subs / dels / inss and the summed clipped deletion lengths and
//                     insertion lengths; per (member, gap between intervals) what the deletions and insertions outside every interval add
//                     to the coordinates behind them
//   k_slice_coords    one thread per member walks its intervals in order: interval_node_coords (slice.rs:103-127) as running sums,
//                     the checks the reference would panic on, and the emptiness CANDIDATES (no inserted letter, deletion lengths >= slice)
//   k_slice_empty     exact emptiness of the candidates: the slice is covered iff its start and every deletion end inside it lie inside
//                     some deletion (lane-parallel over the points, quadratic for candidates only)
//   k_slice_scan_*    offsets of the KEPT members' counts in pair order: inside every slice, then over the slices
//   k_slice_members   one thread per pair: the pga_slice_member_t of a kept member, the entry of a dropped one
//   k_slice_write     one wave per member, its lists in chunks of 64 walked in order: a lane's slot inside its pair's list is the pair's
//                     running count plus the number of lower lanes that go to the same interval -- list order is kept for any input order
// All arithmetic is integer; atomic adds only feed sums and counts, so the result does not depend on the launch geometry.
#include "pga_common.h"
#include "pga_graph_host.h"
#include "pga_wave.h"
#include "../../include/pga_align.h"

namespace pga {

struct SlBlk { uint64_t mem0, int0, pair0, gap0, slice0; uint32_t n_mem, n_int, cons_len, pad; };   // first member / interval / pair / gap bin / slice of a block
struct SlMem { uint64_t sub_off, del_off, ins_off; uint32_t blk, pad; };                            // first edit of a member in the three lists
struct SlTot { unsigned long long kept, dropped, subs, dels, inss; };
typedef unsigned long long sl_u64;

constexpr uint32_t SL_NONE = 0xffffffffu;
constexpr int SL_THREADS = 256, SL_WAVES = SL_THREADS / 64;
constexpr uint32_t SL_CANDIDATE = 1, SL_DROPPED = 2;
// what k_slice_coords reports (the reference panics on each: usize underflow in slice.rs:108/112 and :99, or a position past usize)
enum { SL_ERR_DELETIONS = 1, SL_ERR_COORD_WIDE = 2, SL_ERR_POSITION = 3 };

struct SlDev {
	const SlBlk *blk; const SlMem *mem; const pga_slice_interval_t *iv; const pga_rc_member_t *cnt; const pga_slice_node_t *node;
	const pga_sub_t *subs; const pga_del_t *dels; const pga_ins_t *inss;
	uint32_t *n_sub, *n_del, *n_ins;      // per pair: sliced counts (k_slice_write counts them up once more as its cursors)
	sl_u64 *sum_ins, *sum_del;            // per pair: summed insertion lengths / clipped deletion lengths ...
	sl_u64 *coords, *state;               // ... and, the same memory from k_slice_coords on: node_start | node_end << 32, and 0 / SL_CANDIDATE / SL_DROPPED
	sl_u64 *gap_del, *gap_ins;            // per (member, gap g = the positions between interval g - 1 and interval g): deleted positions, inserted letters
	uint32_t *loc_k, *loc_s, *loc_d, *loc_i;   // per pair: rank among the kept (or the dropped) members of its slice; first edit relative to the slice
	SlTot *slice_tot, *slice_base;        // per slice: totals, and their exclusive sums (entry n_slices: the grand totals)
	uint32_t *err;                        // [0] code, [1..2] the member
	uint64_t n_blocks, n_mem, n_pairs, n_slices;
};

// the last block whose first pair / slice / ... is <= key (blocks that own none share the value of the next one that does)
__device__ __forceinline__ uint64_t sl_block_of(const SlBlk *blk, uint64_t n, uint64_t key, uint64_t SlBlk::*first)
{
	uint64_t lo = 0, hi = n - 1;
	while (lo < hi) { const uint64_t mid = (lo + hi + 1) >> 1; if (blk[mid].*first <= key) lo = mid; else hi = mid - 1; }
	return lo;
}
// number of intervals that end at or before x == the first interval with end > x
__device__ __forceinline__ uint32_t sl_first_end_above(const pga_slice_interval_t *iv, uint32_t n, uint32_t x)
{
	uint32_t lo = 0, hi = n;
	while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (iv[mid].end > x) hi = mid; else lo = mid + 1; }
	return lo;
}
// number of intervals that start before x
__device__ __forceinline__ uint32_t sl_starts_below(const pga_slice_interval_t *iv, uint32_t n, uint32_t x)
{
	uint32_t lo = 0, hi = n;
	while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (iv[mid].start < x) lo = mid + 1; else hi = mid; }
	return lo;
}
// the interval of a substitution or an insertion at pos (Interval::contains, PangraphInterval::insertion_overlap), or SL_NONE and the gap it lies in
__device__ __forceinline__ uint32_t sl_interval_of(const pga_slice_interval_t *iv, uint32_t n, uint32_t pos, uint32_t cons_len, bool is_ins, uint32_t &gap)
{
	const uint32_t j = sl_first_end_above(iv, n, pos);
	gap = j;
	if (j < n && iv[j].start <= pos) return j;
	if (is_ins && pos == cons_len && n && iv[n - 1].end == cons_len) return n - 1;
	return SL_NONE;
}
// the intervals [lo, hi) a deletion [p, q) is sliced into (Interval::has_overlap_with: end > p && start < q)
__device__ __forceinline__ void sl_del_range(const pga_slice_interval_t *iv, uint32_t n, uint32_t p, uint32_t q, uint32_t &lo, uint32_t &hi)
{
	lo = sl_first_end_above(iv, n, p);
	hi = sl_starts_below(iv, n, q);
	if (hi < lo) hi = lo;               // (cannot happen for p <= q: an interval that ends at or before p starts before q)
}
__device__ __forceinline__ uint32_t sl_wave_min(uint32_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, d); v = o < v ? o : v; }
	return v;
}

__global__ __launch_bounds__(SL_THREADS) void k_slice_count(SlDev V)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t n_waves = (uint64_t)gridDim.x * SL_WAVES;
	for (uint64_t m = (uint64_t)blockIdx.x * SL_WAVES + (threadIdx.x >> 6); m < V.n_mem; m += n_waves) {
		const SlMem M = V.mem[m]; const SlBlk B = V.blk[M.blk]; const pga_rc_member_t C = V.cnt[m];
		if (B.n_int == 0) continue;
		const pga_slice_interval_t *iv = V.iv + B.int0;
		const uint64_t mloc = m - B.mem0, pair0 = B.pair0 + mloc, gap0 = B.gap0 + mloc * ((uint64_t)B.n_int + 1);
		for (uint32_t t = lane; t < C.n_subs; t += 64) {
			uint32_t g; const uint32_t j = sl_interval_of(iv, B.n_int, V.subs[M.sub_off + t].pos, B.cons_len, false, g);
			if (j != SL_NONE) atomicAdd(&V.n_sub[pair0 + (uint64_t)j * B.n_mem], 1u);
		}
		for (uint32_t t = lane; t < C.n_inss; t += 64) {
			const pga_ins_t x = V.inss[M.ins_off + t];
			uint32_t g; const uint32_t j = sl_interval_of(iv, B.n_int, x.pos, B.cons_len, true, g);
			if (j != SL_NONE) { const uint64_t P = pair0 + (uint64_t)j * B.n_mem; atomicAdd(&V.n_ins[P], 1u); if (x.len) atomicAdd(&V.sum_ins[P], (sl_u64)x.len); }
			else if (x.len) atomicAdd(&V.gap_ins[gap0 + g], (sl_u64)x.len);      // (behind the last interval: no boundary reads it)
		}
		for (uint32_t t = lane; t < C.n_dels; t += 64) {
			const pga_del_t d = V.dels[M.del_off + t];
			const uint32_t p = d.pos, q = d.pos + d.len;
			uint32_t lo, hi; sl_del_range(iv, B.n_int, p, q, lo, hi);
			for (uint32_t j = lo; j < hi; ++j) {
				const uint64_t P = pair0 + (uint64_t)j * B.n_mem;
				const uint32_t a = max(p, iv[j].start), z = min(q, iv[j].end);
				atomicAdd(&V.n_del[P], 1u);
				if (z > a) atomicAdd(&V.sum_del[P], (sl_u64)(z - a));
			}
			if (d.len) for (uint32_t g = lo; g <= hi; ++g) {                      // the gaps next to those intervals: the only ones it can reach
				const uint32_t a = max(p, g ? iv[g - 1].end : 0u), z = min(q, g < B.n_int ? iv[g].start : B.cons_len);
				if (z > a) atomicAdd(&V.gap_del[gap0 + g], (sl_u64)(z - a));
			}
		}
	}
}

__device__ __forceinline__ void sl_fail(const SlDev &V, uint32_t code, uint64_t m)
{
	if (atomicCAS(&V.err[0], 0u, code) == 0u) { V.err[1] = (uint32_t)(m & 0xffffffffu); V.err[2] = (uint32_t)(m >> 32); }
}

// slice.rs:103-127 with D(x) = deleted positions below x (a position two deletions share counts twice, as there) and I(x) = letters
// inserted before x: s = start - D(start) + I(start), e = end - D(end) + I(end) (+ the insertions at cons_len when end == cons_len, which
// k_slice_count has put into the last interval's own sum)
__global__ __launch_bounds__(SL_THREADS) void k_slice_coords(SlDev V)
{
	for (uint64_t m = (uint64_t)blockIdx.x * SL_THREADS + threadIdx.x; m < V.n_mem; m += (uint64_t)gridDim.x * SL_THREADS) {
		const SlMem M = V.mem[m]; const SlBlk B = V.blk[M.blk];
		const pga_slice_interval_t *iv = V.iv + B.int0;
		const pga_slice_node_t N = V.node[m];
		const uint64_t mloc = m - B.mem0, gap0 = B.gap0 + mloc * ((uint64_t)B.n_int + 1);
		sl_u64 D = 0, I = 0;
		for (uint32_t j = 0; j < B.n_int; ++j) {
			const uint64_t P = B.pair0 + (uint64_t)j * B.n_mem + mloc;
			const sl_u64 start = iv[j].start, end = iv[j].end;
			D += V.gap_del[gap0 + j]; I += V.gap_ins[gap0 + j];
			bool bad = D > start;
			const sl_u64 s = start - D + I;
			const sl_u64 dl = V.sum_del[P], il = V.sum_ins[P];
			D += dl; I += il;
			bad = bad || D > end;
			const sl_u64 e = end - D + I;
			if (bad) { sl_fail(V, SL_ERR_DELETIONS, m); V.coords[P] = 0; V.state[P] = 0; continue; }
			if (s > 0xffffffffULL || e > 0xffffffffULL) { sl_fail(V, SL_ERR_COORD_WIDE, m); V.coords[P] = 0; V.state[P] = 0; continue; }
			if (N.reverse) {                                                      // slice.rs:79-80 and :99 subtract both coordinates
				const sl_u64 room = N.circular ? N.pos_end + N.path_len : N.pos_end;
				if (room < e || room < s) sl_fail(V, SL_ERR_POSITION, m);
			}
			V.coords[P] = s | e << 32;                                            // (over sum_ins / sum_del: read above)
			V.state[P] = (il == 0 && dl >= end - start) ? SL_CANDIDATE : 0;
		}
	}
}

// Edit::is_empty_alignment for the candidates: apply() leaves nothing iff the union of the sliced deletions is the whole slice.  The union
// is the whole slice iff `start` is inside a deletion and so is the end of every deletion that ends inside the slice.
__global__ __launch_bounds__(SL_THREADS) void k_slice_empty(SlDev V)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t n_waves = (uint64_t)gridDim.x * SL_WAVES;
	for (uint64_t base = ((uint64_t)blockIdx.x * SL_WAVES + (threadIdx.x >> 6)) * 64; base < V.n_pairs; base += n_waves * 64) {
		unsigned long long todo = __ballot(base + lane < V.n_pairs && V.state[base + lane] == SL_CANDIDATE);
		while (todo) {
			const uint64_t P = base + (uint64_t)(__ffsll((long long)todo) - 1);
			todo &= todo - 1;
			const SlBlk B = V.blk[sl_block_of(V.blk, V.n_blocks, P, &SlBlk::pair0)];
			const uint32_t j = (uint32_t)((P - B.pair0) / B.n_mem);
			const uint64_t m = B.mem0 + (P - B.pair0) % B.n_mem;
			const pga_slice_interval_t X = V.iv[B.int0 + j];
			const pga_del_t *dels = V.dels + V.mem[m].del_off;
			const uint32_t nd = V.cnt[m].n_dels;
			bool open = false;                                                    // one of this lane's points lies in no deletion
			for (uint32_t c0 = 0; c0 <= nd; c0 += 64) {                           // point 0: the start; point t + 1: the end of deletion t
				const uint32_t t = c0 + lane;
				uint32_t x = X.start; bool have = t == 0;
				if (t >= 1 && t <= nd) { const pga_del_t d = dels[t - 1]; x = d.pos + d.len; have = x > X.start && x < X.end; }
				bool in = false;
				for (uint32_t k = 0; k < nd; ++k) { const pga_del_t d = dels[k]; in = in || (d.pos <= x && x < d.pos + d.len); }
				open = open || (have && !in);
			}
			if (!__ballot(open) && lane == 0) V.state[P] = SL_DROPPED;
		}
	}
}

// one wave per slice: ranks and first edits of its members, kept and dropped counted apart
__global__ __launch_bounds__(SL_THREADS) void k_slice_scan_local(SlDev V)
{
	const uint32_t lane = threadIdx.x & 63u;
	const unsigned long long below = (1ULL << lane) - 1ULL;
	const uint64_t n_waves = (uint64_t)gridDim.x * SL_WAVES;
	for (uint64_t sl = (uint64_t)blockIdx.x * SL_WAVES + (threadIdx.x >> 6); sl < V.n_slices; sl += n_waves) {
		const SlBlk B = V.blk[sl_block_of(V.blk, V.n_blocks, sl, &SlBlk::slice0)];
		const uint64_t P0 = B.pair0 + (sl - B.slice0) * B.n_mem;
		uint32_t run_k = 0, run_x = 0, run_s = 0, run_d = 0, run_i = 0;
		for (uint32_t c0 = 0; c0 < B.n_mem; c0 += 64) {
			const bool ok = c0 + lane < B.n_mem;
			const uint64_t P = P0 + c0 + lane;
			const bool kept = ok && V.state[P] != SL_DROPPED;
			const uint32_t vs = kept ? V.n_sub[P] : 0u, vd = kept ? V.n_del[P] : 0u, vi = kept ? V.n_ins[P] : 0u;
			uint32_t is = vs, id = vd, ii = vi;                                   // inclusive sums over the lanes
#pragma unroll
			for (int d = 1; d < 64; d <<= 1) {
				const uint32_t a = (uint32_t)__shfl_up((int)is, d), b = (uint32_t)__shfl_up((int)id, d), c = (uint32_t)__shfl_up((int)ii, d);
				if ((int)lane >= d) { is += a; id += b; ii += c; }
			}
			const unsigned long long km = __ballot(kept), xm = __ballot(ok && !kept);
			if (ok) {
				V.loc_k[P] = kept ? run_k + (uint32_t)__popcll(km & below) : run_x + (uint32_t)__popcll(xm & below);
				V.loc_s[P] = run_s + is - vs; V.loc_d[P] = run_d + id - vd; V.loc_i[P] = run_i + ii - vi;
			}
			run_k += (uint32_t)__popcll(km); run_x += (uint32_t)__popcll(xm);
			run_s += (uint32_t)__shfl((int)is, 63); run_d += (uint32_t)__shfl((int)id, 63); run_i += (uint32_t)__shfl((int)ii, 63);
		}
		if (lane == 0) V.slice_tot[sl] = SlTot{run_k, run_x, run_s, run_d, run_i};
	}
}

// ONE wave: exclusive sums of the slice totals in slice order, the grand totals behind them, and the slice records of the output
__global__ __launch_bounds__(64) void k_slice_scan_slices(SlDev V, pga_slice_res_t *out)
{
	const uint32_t lane = threadIdx.x;
	SlTot run{0, 0, 0, 0, 0};
	for (uint64_t c0 = 0; c0 < V.n_slices; c0 += 64) {
		const uint64_t sl = c0 + lane;
		const bool ok = sl < V.n_slices;
		SlTot t{0, 0, 0, 0, 0};
		if (ok) t = V.slice_tot[sl];
		const SlTot in{wave_incl_u64(t.kept, lane), wave_incl_u64(t.dropped, lane), wave_incl_u64(t.subs, lane), wave_incl_u64(t.dels, lane), wave_incl_u64(t.inss, lane)};
		if (ok) {
			V.slice_base[sl] = SlTot{run.kept + in.kept - t.kept, run.dropped + in.dropped - t.dropped, run.subs + in.subs - t.subs, run.dels + in.dels - t.dels, run.inss + in.inss - t.inss};
			pga_slice_res_t r; r.member_off = run.kept + in.kept - t.kept; r.n_kept = (uint32_t)t.kept; r.n_dropped = (uint32_t)t.dropped;
			out[sl] = r;
		}
		run.kept += __shfl(in.kept, 63); run.dropped += __shfl(in.dropped, 63); run.subs += __shfl(in.subs, 63); run.dels += __shfl(in.dels, 63); run.inss += __shfl(in.inss, 63);
	}
	if (lane == 0) V.slice_base[V.n_slices] = run;
}

// one thread per pair: the record of a kept member (new_strandedness slice.rs:55-61, new_position_* slice.rs:67-101), the entry of a dropped one
__global__ __launch_bounds__(SL_THREADS) void k_slice_members(SlDev V, pga_slice_member_t *members, pga_rc_member_t *counts, uint32_t *dropped)
{
	for (uint64_t P = (uint64_t)blockIdx.x * SL_THREADS + threadIdx.x; P < V.n_pairs; P += (uint64_t)gridDim.x * SL_THREADS) {
		const SlBlk B = V.blk[sl_block_of(V.blk, V.n_blocks, P, &SlBlk::pair0)];
		const uint32_t j = (uint32_t)((P - B.pair0) / B.n_mem), mloc = (uint32_t)((P - B.pair0) % B.n_mem);
		const SlTot base = V.slice_base[B.slice0 + j];
		if (V.state[P] == SL_DROPPED) { dropped[base.dropped + V.loc_k[P]] = mloc; continue; }
		const pga_slice_node_t N = V.node[B.mem0 + mloc];
		const sl_u64 c = V.coords[P], s = c & 0xffffffffULL, e = c >> 32;
		pga_slice_member_t o;
		memset(&o, 0, sizeof(o));                                               // (the padding too: the records compare as bytes)
		o.member = mloc;
		o.reverse = ((N.reverse != 0) != (V.iv[B.int0 + j].flip != 0)) ? 1 : 0;
		o.node_start = (uint32_t)s; o.node_end = (uint32_t)e;
		if (N.circular) {
			const sl_u64 L = N.path_len;
			if (!N.reverse) { o.pos_start = (N.pos_start + s) % L; o.pos_end = (N.pos_start + e) % L; }
			else { o.pos_start = (N.pos_end + L - e) % L; o.pos_end = (N.pos_end + L - s) % L; }
		} else if (!N.reverse) { o.pos_start = N.pos_start + s; o.pos_end = N.pos_start + e; }
		else { o.pos_start = N.pos_end - e; o.pos_end = N.pos_end - s; }
		o.counts.n_subs = V.n_sub[P]; o.counts.n_dels = V.n_del[P]; o.counts.n_inss = V.n_ins[P];
		o.sub_off = base.subs + V.loc_s[P]; o.del_off = base.dels + V.loc_d[P]; o.ins_off = base.inss + V.loc_i[P];
		members[base.kept + V.loc_k[P]] = o;
		counts[base.kept + V.loc_k[P]] = o.counts;                               // the same counts, packed: what pga_solve_promises / pga_reconsensus take
	}
}

// Every lane holds the intervals [next, last) its edit goes to (none: next == last).  The wave takes the touched intervals in ascending
// order; for interval T the lanes that go there get consecutive slots in lane order behind the pair's running count, which the lowest of
// them advances (one atomic add with return per chunk and touched interval: it orders the chunks of a list, which one wave walks in turn).
// put(T, slot) stores the lane's edit; a dropped pair takes no slots.
template <int LIST, class Put> __device__ __forceinline__ void sl_place(const SlDev &V, const SlBlk &B, uint64_t mloc, uint32_t next, uint32_t last, Put put)
{
	const uint32_t lane = threadIdx.x & 63u;
	const unsigned long long below = (1ULL << lane) - 1ULL;
	for (;;) {
		const uint32_t T = sl_wave_min(next < last ? next : SL_NONE);
		if (T == SL_NONE) break;
		const bool mine = next < last && next == T;
		const unsigned long long who = __ballot(mine);
		const int leader = __ffsll((long long)who) - 1;
		sl_u64 at = ~0ULL;
		if ((int)lane == leader) {
			const uint64_t P = B.pair0 + (uint64_t)T * B.n_mem + mloc;
			if (V.state[P] != SL_DROPPED) {
				const SlTot base = V.slice_base[B.slice0 + T];
				const uint32_t n = (uint32_t)__popcll(who);
				if (LIST == 0) at = base.subs + V.loc_s[P] + atomicAdd(&V.n_sub[P], n);
				else if (LIST == 1) at = base.dels + V.loc_d[P] + atomicAdd(&V.n_del[P], n);
				else at = base.inss + V.loc_i[P] + atomicAdd(&V.n_ins[P], n);
			}
		}
		at = __shfl(at, leader);
		if (mine) { if (at != ~0ULL) put(T, at + (sl_u64)__popcll(who & below)); ++next; }
	}
}

__global__ __launch_bounds__(SL_THREADS) void k_slice_write(SlDev V, pga_sub_t *o_subs, pga_del_t *o_dels, pga_ins_t *o_inss)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t n_waves = (uint64_t)gridDim.x * SL_WAVES;
	for (uint64_t m = (uint64_t)blockIdx.x * SL_WAVES + (threadIdx.x >> 6); m < V.n_mem; m += n_waves) {
		const SlMem M = V.mem[m]; const SlBlk B = V.blk[M.blk]; const pga_rc_member_t C = V.cnt[m];
		if (B.n_int == 0) continue;
		const pga_slice_interval_t *iv = V.iv + B.int0;
		const uint64_t mloc = m - B.mem0;
		for (uint32_t c0 = 0; c0 < C.n_subs; c0 += 64) {
			pga_sub_t x{0, 0}; uint32_t j = SL_NONE, g;
			if (c0 + lane < C.n_subs) { x = V.subs[M.sub_off + c0 + lane]; j = sl_interval_of(iv, B.n_int, x.pos, B.cons_len, false, g); }
			sl_place<0>(V, B, mloc, j, j == SL_NONE ? j : j + 1, [&](uint32_t T, sl_u64 slot) { o_subs[slot] = pga_sub_t{x.pos - iv[T].start, x.alt}; });
		}
		for (uint32_t c0 = 0; c0 < C.n_dels; c0 += 64) {
			uint32_t p = 0, q = 0, lo = 0, hi = 0;
			if (c0 + lane < C.n_dels) { const pga_del_t d = V.dels[M.del_off + c0 + lane]; p = d.pos; q = d.pos + d.len; sl_del_range(iv, B.n_int, p, q, lo, hi); }
			sl_place<1>(V, B, mloc, lo, hi, [&](uint32_t T, sl_u64 slot) {
				const uint32_t a = max(p, iv[T].start), z = min(q, iv[T].end);          // slice.rs:26-28
				o_dels[slot] = pga_del_t{a - iv[T].start, z - a};
			});
		}
		for (uint32_t c0 = 0; c0 < C.n_inss; c0 += 64) {
			pga_ins_t x{0, 0, 0}; uint32_t j = SL_NONE, g;
			if (c0 + lane < C.n_inss) { x = V.inss[M.ins_off + c0 + lane]; j = sl_interval_of(iv, B.n_int, x.pos, B.cons_len, true, g); }
			sl_place<2>(V, B, mloc, j, j == SL_NONE ? j : j + 1, [&](uint32_t T, sl_u64 slot) { o_inss[slot] = pga_ins_t{x.pos - iv[T].start, x.len, x.seq_off}; });
		}
	}
}

// ---------------------------------------------------------------- host side
// (not host_array of pga_graph_host.h: these arrays are written in full and are not zeroed)
template <class T> static T *sl_host_array(uint64_t n)
{
	T *p = (T*)malloc((size_t)(n ? n : 1) * sizeof(T));
	if (!p) throw std::runtime_error("pga_slice_blocks: out of host memory");
	return p;
}
static unsigned sl_grid(uint64_t items, uint64_t per_block) { return grid_for(items, per_block, 1u << 18); }

void slice_blocks_host(int64_t n_blocks, const pga_slice_block_t *blocks, const pga_slice_interval_t *intervals, const pga_rc_member_t *members, const pga_slice_node_t *nodes,
                       const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss, pga_slice_out_t *out)
{
	auto fail = [](const std::string &what) { throw std::runtime_error("pga_slice_blocks: " + what); };
	// ---- tables and validation, O(blocks + intervals + members + edits) ----
	std::vector<SlBlk> blk((size_t)n_blocks);
	uint64_t n_mem = 0, n_int = 0, n_pairs = 0, n_gaps = 0, n_slices = 0;
	for (int64_t b = 0; b < n_blocks; ++b) {
		const pga_slice_block_t &Q = blocks[b];
		if (Q.cons_len == 0) fail("block " + std::to_string(b) + " has an empty consensus");
		blk[b] = SlBlk{n_mem, n_int, n_pairs, n_gaps, n_slices, Q.n_members, Q.n_intervals, Q.cons_len, 0u};
		n_mem += Q.n_members; n_int += Q.n_intervals; n_slices += Q.n_intervals;
		n_pairs += (uint64_t)Q.n_members * Q.n_intervals; n_gaps += (uint64_t)Q.n_members * ((uint64_t)Q.n_intervals + 1);
	}
	if (n_int && !intervals) fail("null interval list");
	if (n_mem && (!members || !nodes)) fail("null member list");
	for (int64_t b = 0; b < n_blocks; ++b) {
		uint32_t prev_end = 0;
		for (uint32_t j = 0; j < blk[b].n_int; ++j) {
			const pga_slice_interval_t &X = intervals[blk[b].int0 + j];
			if (X.start >= X.end || X.end > blk[b].cons_len || X.start < prev_end)
				fail("the intervals of block " + std::to_string(b) + " are not sorted, non-empty, disjoint and inside the consensus (interval " + std::to_string(j) + ")");
			prev_end = X.end;
		}
	}
	std::vector<SlMem> mem((size_t)n_mem);
	uint64_t n_subs = 0, n_dels = 0, n_inss = 0;
	for (int64_t b = 0; b < n_blocks; ++b) {
		const uint64_t s0 = n_subs, d0 = n_dels, i0 = n_inss;
		for (uint64_t m = blk[b].mem0; m < blk[b].mem0 + blk[b].n_mem; ++m) {
			mem[m] = SlMem{n_subs, n_dels, n_inss, (uint32_t)b, 0u};
			n_subs += members[m].n_subs; n_dels += members[m].n_dels; n_inss += members[m].n_inss;
			if (nodes[m].circular && nodes[m].path_len == 0) fail("circular node on a path of length 0 (member " + std::to_string(m) + ")");
		}
		if (n_subs - s0 >= (1ULL << 32) || n_dels - d0 >= (1ULL << 32) || n_inss - i0 >= (1ULL << 32)) fail("more than 2^32 edits of one kind in block " + std::to_string(b));
	}
	if (n_blocks >= (1LL << 32)) fail("more than 2^32 blocks");
	if ((n_subs && !subs) || (n_dels && !dels) || (n_inss && !inss)) fail("null edit list");
	for (uint64_t m = 0; m < n_mem; ++m) {
		const uint32_t L = blk[mem[m].blk].cons_len;
		for (uint64_t t = mem[m].sub_off, z = t + members[m].n_subs; t < z; ++t) if (subs[t].pos >= L) fail("substitution beyond the consensus (member " + std::to_string(m) + ")");
		for (uint64_t t = mem[m].del_off, z = t + members[m].n_dels; t < z; ++t) if ((uint64_t)dels[t].pos + dels[t].len > L) fail("deletion beyond the consensus (member " + std::to_string(m) + ")");
		for (uint64_t t = mem[m].ins_off, z = t + members[m].n_inss; t < z; ++t) if (inss[t].pos > L) fail("insertion beyond the consensus (member " + std::to_string(m) + ")");
	}
	out->slices = sl_host_array<pga_slice_res_t>(n_slices);
	if (n_slices == 0 || n_mem == 0) {                                            // nothing to slice: every slice is empty
		for (uint64_t s = 0; s < n_slices; ++s) out->slices[s] = pga_slice_res_t{0, 0, 0};
		out->members = sl_host_array<pga_slice_member_t>(0); out->counts = sl_host_array<pga_rc_member_t>(0); out->dropped = sl_host_array<uint32_t>(0);
		out->subs = sl_host_array<pga_sub_t>(0); out->dels = sl_host_array<pga_del_t>(0); out->inss = sl_host_array<pga_ins_t>(0);
		return;
	}
	// ---- the device ----
	StreamLease stream;
	hipStream_t st = stream.s;
	DBuf<SlBlk> d_blk; d_blk.upload(blk, st);
	DBuf<SlMem> d_mem; d_mem.upload(mem, st);
	DBuf<pga_slice_interval_t> d_iv; d_iv.upload(intervals, n_int, st);
	DBuf<pga_rc_member_t> d_cnt; d_cnt.upload(members, n_mem, st);
	DBuf<pga_slice_node_t> d_node; d_node.upload(nodes, n_mem, st);
	DBuf<pga_sub_t> d_subs(n_subs + 1); DBuf<pga_del_t> d_dels(n_dels + 1); DBuf<pga_ins_t> d_inss(n_inss + 1);
	if (n_subs) PGA_HIP(hipMemcpyAsync(d_subs.p, subs, n_subs * sizeof(pga_sub_t), hipMemcpyHostToDevice, st));
	if (n_dels) PGA_HIP(hipMemcpyAsync(d_dels.p, dels, n_dels * sizeof(pga_del_t), hipMemcpyHostToDevice, st));
	if (n_inss) PGA_HIP(hipMemcpyAsync(d_inss.p, inss, n_inss * sizeof(pga_ins_t), hipMemcpyHostToDevice, st));
	DBuf<uint32_t> d_n(3 * n_pairs + 1), d_loc(4 * n_pairs + 1), d_err(4);
	DBuf<sl_u64> d_sum(2 * n_pairs + 1), d_gap(2 * n_gaps);
	DBuf<SlTot> d_tot(n_slices), d_base(n_slices + 1);
	d_n.zero(st); d_sum.zero(st); d_gap.zero(st); d_err.zero(st);
	SlDev V;
	V.blk = d_blk.p; V.mem = d_mem.p; V.iv = d_iv.p; V.cnt = d_cnt.p; V.node = d_node.p; V.subs = d_subs.p; V.dels = d_dels.p; V.inss = d_inss.p;
	V.n_sub = d_n.p; V.n_del = d_n.p + n_pairs; V.n_ins = d_n.p + 2 * n_pairs;
	V.sum_ins = V.coords = d_sum.p; V.sum_del = V.state = d_sum.p + n_pairs;
	V.gap_del = d_gap.p; V.gap_ins = d_gap.p + n_gaps;
	V.loc_k = d_loc.p; V.loc_s = d_loc.p + n_pairs; V.loc_d = d_loc.p + 2 * n_pairs; V.loc_i = d_loc.p + 3 * n_pairs;
	V.slice_tot = d_tot.p; V.slice_base = d_base.p; V.err = d_err.p;
	V.n_blocks = (uint64_t)n_blocks; V.n_mem = n_mem; V.n_pairs = n_pairs; V.n_slices = n_slices;
	DBuf<pga_slice_res_t> d_slices(n_slices);
	hipLaunchKernelGGL(k_slice_count, dim3(sl_grid(n_mem, SL_WAVES)), dim3(SL_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_slice_coords, dim3(sl_grid(n_mem, SL_THREADS)), dim3(SL_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_slice_empty, dim3(sl_grid(n_pairs, SL_WAVES * 64)), dim3(SL_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_slice_scan_local, dim3(sl_grid(n_slices, SL_WAVES)), dim3(SL_THREADS), 0, st, V);
	hipLaunchKernelGGL(k_slice_scan_slices, dim3(1), dim3(64), 0, st, V, d_slices.p);
	PGA_HIP(hipGetLastError());
	// ---- the one read-back before the write pass: the totals size the output, the error word ends the call ----
	SlTot tot; uint32_t err[4];
	PGA_HIP(hipMemcpyAsync(&tot, d_base.p + n_slices, sizeof(tot), hipMemcpyDeviceToHost, st));
	PGA_HIP(hipMemcpyAsync(err, d_err.p, sizeof(err), hipMemcpyDeviceToHost, st));
	PGA_HIP(sync_stream(st));
	if (err[0]) {
		const std::string who = " (member " + std::to_string((uint64_t)err[1] | (uint64_t)err[2] << 32) + ")";
		if (err[0] == SL_ERR_DELETIONS) fail("overlapping deletions remove more positions than lie before an interval boundary" + who);
		if (err[0] == SL_ERR_COORD_WIDE) fail("node coordinates outside 32 bits" + who);
		fail("reverse node ends before its coordinates inside the block (pos_end < node_end)" + who);
	}
	if (tot.kept + tot.dropped != n_pairs) fail("internal: kept and dropped members do not add up");
	DBuf<pga_slice_member_t> d_members(tot.kept + 1); DBuf<pga_rc_member_t> d_counts(tot.kept + 1); DBuf<uint32_t> d_dropped(tot.dropped + 1);
	DBuf<pga_sub_t> d_osubs(tot.subs + 1); DBuf<pga_del_t> d_odels(tot.dels + 1); DBuf<pga_ins_t> d_oinss(tot.inss + 1);
	hipLaunchKernelGGL(k_slice_members, dim3(sl_grid(n_pairs, SL_THREADS)), dim3(SL_THREADS), 0, st, V, d_members.p, d_counts.p, d_dropped.p);
	d_n.zero(st);                                                                 // the counts are in the records now; the write pass counts up again
	hipLaunchKernelGGL(k_slice_write, dim3(sl_grid(n_mem, SL_WAVES)), dim3(SL_THREADS), 0, st, V, d_osubs.p, d_odels.p, d_oinss.p);
	PGA_HIP(hipGetLastError());
	out->members = sl_host_array<pga_slice_member_t>(tot.kept); out->counts = sl_host_array<pga_rc_member_t>(tot.kept); out->dropped = sl_host_array<uint32_t>(tot.dropped);
	out->subs = sl_host_array<pga_sub_t>(tot.subs); out->dels = sl_host_array<pga_del_t>(tot.dels); out->inss = sl_host_array<pga_ins_t>(tot.inss);
	PGA_HIP(hipMemcpyAsync(out->slices, d_slices.p, n_slices * sizeof(pga_slice_res_t), hipMemcpyDeviceToHost, st));
	if (tot.kept) PGA_HIP(hipMemcpyAsync(out->members, d_members.p, tot.kept * sizeof(pga_slice_member_t), hipMemcpyDeviceToHost, st));
	if (tot.kept) PGA_HIP(hipMemcpyAsync(out->counts, d_counts.p, tot.kept * sizeof(pga_rc_member_t), hipMemcpyDeviceToHost, st));
	if (tot.dropped) PGA_HIP(hipMemcpyAsync(out->dropped, d_dropped.p, tot.dropped * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	if (tot.subs) PGA_HIP(hipMemcpyAsync(out->subs, d_osubs.p, tot.subs * sizeof(pga_sub_t), hipMemcpyDeviceToHost, st));
	if (tot.dels) PGA_HIP(hipMemcpyAsync(out->dels, d_odels.p, tot.dels * sizeof(pga_del_t), hipMemcpyDeviceToHost, st));
	if (tot.inss) PGA_HIP(hipMemcpyAsync(out->inss, d_oinss.p, tot.inss * sizeof(pga_ins_t), hipMemcpyDeviceToHost, st));
	PGA_HIP(sync_stream(st));
}

} // namespace pga
