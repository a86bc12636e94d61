/* pga_align.h -- the drop-in boundary, part 2: the native batch entry of libpgalign.so.
 *
 * One call aligns G independent all-vs-all GROUPS (one group = the block set of one `find_matches` call,
 * reference: packages/pangraph/src/pangraph/graph_merging.rs:176-185 ->
 * packages/pangraph/src/align/minimap2_lib/align_with_minimap2_lib.rs:15-85) and returns, per group, exactly the
 * records `align_with_minimap2_lib` would build from minimap2's output (alignment.rs:13-57), in query order
 * (ascending sequence index inside the group, then minimap2's own order inside a query).
 * Plain pointers and sizes only; results are owned by the library until pga_result_free().
 *
 * Errors: negative return + pga_last_error() (thread-local string).  The library needs a gfx950 device; it has
 * no CPU fallback.
 */
#ifndef PGA_ALIGN_H
#define PGA_ALIGN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
	int32_t sensitivity;         /* 5 | 10 | 20  -> minimap2 preset asm5/asm10/asm20 (align_with_minimap2_lib.rs:35-40) */
	int32_t kmer_length;         /* <=0: preset default (-K, alignment_args.rs:33-35)                                  */
	int32_t indel_len_threshold; /* -l; minimap2 -s = max(len-10, 5) (align_with_minimap2_lib.rs:47)                  */
	int32_t n_threads;           /* host threads for CIGAR post-processing; <=0: all cores                           */
} pga_params_t;

/* One record == one `Alignment` (alignment.rs:40-57). */
typedef struct {
	int32_t group;               /* index of the group the record belongs to */
	int32_t qry, ref;            /* sequence indices inside the group (-> Hit.name) */
	int32_t qry_len, qry_start, qry_end;
	int32_t ref_len, ref_start, ref_end;
	int32_t matches, length, quality;  /* mlen, blen, mapq */
	int32_t reverse;             /* 0 forward, 1 reverse (orientation) */
	int32_t align;               /* AS = dp_score */
	int32_t n_ambi, inv;
	double divergence;           /* de = 1 - mm_event_identity (packages/minimap2/src/map.rs:320-325) */
	uint64_t cigar_off;          /* first op in the CIGAR pool */
	uint32_t n_cigar;            /* ops are len<<4|op, op in "MIDNSHP=XB" */
	uint32_t pad;
} pga_match_t;

typedef struct pga_result_s pga_result_t;

typedef struct {                 /* stage wall times (s) and work counters of a call */
	double upload, sketch, index, seed, chain, align, total;
	double n_bases, n_minimizers, n_anchors, n_dp_jobs, n_dp_cells, n_matches, n_dp_bases;
	/* the path's own kernels, device time from HIP events on the launch stream (streams overlap: the times do not add up to `total`):
	 * [0] k_sketch_tiles  [1] k_chain_fast (+k_chain_segments)  [2] k_bt_list + k_bt_walk  [3] k_extd2_fast (register tiles)
	 * [4] k_extd2_wide<256>  [5] k_ll_i16  [6] k_rs_init + k_rs_pass + k_rs_small (sort replay)  [7] k_gapfill_band (corridor gap fills)
	 * [8] k_extd2_wide<512>  [9] k_extd2_wide<1024>  [10] index build (device sorts + CSR kernels)  [11] seeding kernels + anchor sort
	 * [12] k_approx_strips (large unbanded gap fills over several workgroups)  [13] k_extd2_lanes (banded problems, rows in registers)
	 * [14..15] unused.  kern_cells: DP cells evaluated by the DP kernels ([3] [4] [5] [7] [8] [9] [12] [13]), 0 elsewhere.
	 * The struct is read through pga_result_stats() only and is sized by PGA_STATS_VERSION: version 2 (round 2) grew the arrays from 10 to
	 * 16 entries and added kern_cells -- a consumer compiled against version 1 must be rebuilt. */
#define PGA_STATS_VERSION 2
	double kern_ms[16], kern_launches[16], kern_alg_bytes[16], kern_cells[16];
	double aligned_span;         /* sum of (qry_end - qry_start) over the emitted matches (secondary metric) */
} pga_stats_t;

/* seqs: n_seqs sequences, ASCII, NOT necessarily NUL-terminated (lengths in seq_lens); names: NUL-terminated
 * decimal BlockId strings (unique inside a group); group_off: n_groups+1 offsets into the sequence arrays. */
int pga_align_groups(const pga_params_t *params, int32_t n_groups, const int64_t *group_off,
                     const char *const *seqs, const uint32_t *seq_lens, const char *const *names, pga_result_t **out);
/* Same work split in two: pga_batch_create() copies the sequences to the device (2-step hand-over for callers
 * that keep block sequences resident across self-merge rounds); pga_batch_align() runs sketch -> index -> seed ->
 * chain -> extend on the resident bases and may be called repeatedly. */
typedef struct pga_batch_s pga_batch_t;
int pga_batch_create(int32_t n_groups, const int64_t *group_off, const char *const *seqs, const uint32_t *seq_lens, const char *const *names, pga_batch_t **out);
int pga_batch_align(pga_batch_t *batch, const pga_params_t *params, pga_result_t **out);
/* The batch of the next self-merge round: a sequence with seqs[i] == NULL is the src_index[i]-th sequence of `old` (numbered in hand-over
 * order) and is copied device to device from its packed store; the others are handed over as in pga_batch_create (block
 * sequences stay resident across rounds; the reference re-copies every block as ASCII per call, minimap2/src/index.rs:31-37).  seq_lens[i]
 * of a derived sequence must equal its source's.  `old` is not modified and may be freed afterwards. */
int pga_batch_derive(const pga_batch_t *old, int32_t n_groups, const int64_t *group_off, const char *const *seqs, const int64_t *src_index,
                     const uint32_t *seq_lens, const char *const *names, pga_batch_t **out);
/* Multi-GPU hosts, waves with fewer groups than ranks (the reference parallelises over the queries of one index,
 * align_with_minimap2_lib.rs:64-74): every shard indexes ALL sequences of the batch and maps, of every group, a contiguous range of the
 * queries (balanced by length).  The shards' match lists are disjoint; their union ordered by (group, query) is pga_batch_align's list. */
int pga_batch_align_shard(pga_batch_t *batch, const pga_params_t *params, int32_t shard, int32_t n_shards, pga_result_t **out);
/* The exchange step of a multi-GPU build is a gather of match lists and nothing else; transport is the host's (RCCL / MPI point to point: the
 * CIGAR pool dominates the payload and only the owner of the graph needs it).  These two are the host logic either side of it (no device work;
 * pangraph_amd/dist.py holds the same for the Python host, tests/test_dist_cpu.py compares them):
 *   pga_shard_groups_balanced  deals n_groups groups to `world` ranks, heaviest first, each to the rank that is lightest so far (ties: lower
 *                              rank); rank_of_group[g] receives the owner.  Deterministic: every rank computes the same plan without talking.
 *   pga_merge_match_lists      puts the lists of n_parts ranks together as ONE rank would have produced them: group ids become global
 *                              (local_to_global[r][g], or unchanged where local_to_global or local_to_global[r] is NULL), CIGAR offsets point into
 *                              the concatenated pool, records ordered by (group, query, the aligner's own order inside a query) -- also when the
 *                              queries of one group were split over the ranks (pga_batch_align_shard).  out_matches holds sum n_matches records,
 *                              out_cigars sum n_cigar_words words; returns 0, -1 on a group id outside its table. */
void pga_shard_groups_balanced(int32_t n_groups, const double *weights, int32_t world, int32_t *rank_of_group);
int pga_merge_match_lists(int32_t n_parts, const pga_match_t *const *matches, const int64_t *n_matches, const uint32_t *const *cigars,
                          const int64_t *n_cigar_words, const int32_t *const *local_to_global, const int32_t *n_local_groups,
                          pga_match_t *out_matches, uint32_t *out_cigars);
void pga_batch_free(pga_batch_t *batch);
int64_t pga_result_n_matches(const pga_result_t *r);
const pga_match_t *pga_result_matches(const pga_result_t *r);
const uint32_t *pga_result_cigars(const pga_result_t *r, uint64_t *n_ops);
const pga_stats_t *pga_result_stats(const pga_result_t *r);
void pga_result_free(pga_result_t *r);
const char *pga_last_error(void);
/* number of visible HIP devices (<=0: none, the library cannot run) and selection of the one to use.  The selection holds for the PROCESS:
 * HIP's current device belongs to the host thread, so every entry point of the library (mm_map included) applies the selected device to
 * the thread it is called on -- worker threads of the host need not call pga_set_device themselves. */
int pga_device_count(void);
int pga_set_device(int dev);
/* optional: create n streams ahead of time for the batch handles a host keeps in flight at once (they land on different hardware queues) */
int pga_warm_streams(int32_t n);
/* Gives back what the library holds of the device between calls: the idle blocks of its device-memory cache and the scratch slabs of the DP launch-lane
 * sets no call is using at the moment (both are bought again, at hipMalloc's price, by the next calls that need them).  For a host that shares the device
 * with another process or is done aligning for a while; hipFree synchronises the device.  Returns the bytes released. */
int64_t pga_trim(void);
/* the library's device-memory cache (diagnostics): out[0..5] = hipMalloc calls behind the cache, ns spent in them, hipFree calls, ns, bytes handed
 * out at the moment, bytes idle in the cache.  A host that sees hipFree calls grow from batch to batch has filled the device: the cache gives
 * the blocks that have been idle longest back, down to 4 GB below its limit (PGA_CACHE_GB, 90 % of the device), and hipFree synchronises the
 * device each time. */
void pga_mem_stats(int64_t out[6]);

/* Stage taps for parity tests (same semantics as the reference functions named in each comment). */
/* mm_sketch (sketch.c:77): minimizers of n sequences; out arrays are malloc()ed, caller frees with pga_free */
int pga_stage_sketch(int32_t n, const char *const *seqs, const uint32_t *lens, int w, int k, uint64_t **mz_xy, uint64_t **seq_off);
/* collect_seed_hits + mg_lchain_rmq (map.c:168-204, lchain.c:250-368) of an all-vs-all group:
 * anchors (x,y pairs) per query, chains u[] and compacted anchors per query, as flat malloc()ed arrays */
int pga_stage_chain(const pga_params_t *params, int32_t n, const char *const *seqs, const uint32_t *lens, const char *const *names,
                    uint64_t **anchors_xy, uint64_t **anchor_off, int32_t **n_u, int32_t **n_v, uint64_t **u, uint64_t **chain_xy, int32_t **rep_len, int32_t *mid_occ);
/* ksw_extd2_sse (ksw2_extd2_sse.c:34) on explicit nt4 sequences; ez[12] = max,max_q,max_t,mqe,mqe_t,mte,mte_q,score,zdropped,reach_end,n_cigar,0 */
int pga_stage_extd2(int32_t n_jobs, const uint8_t *const *q, const int32_t *qlen, const uint8_t *const *t, const int32_t *tlen,
                    int a, int b, int sc_ambi, int gapo, int gape, int gapo2, int gape2, const int32_t *w, const int32_t *zdrop, const int32_t *end_bonus, const int32_t *flag,
                    int32_t *ez, uint32_t **cigars, uint64_t *cigar_off);
/* which kernel answered the DP problems of every call since the last one of this function (process-wide counters, copied out and zeroed):
 * by_class[c] = problems launched in class c of dp_run (pga_ksw.hip: 0,1 register tiles, 2-4,7 workgroup kernel, 5 single wave, 6 ksw_ll_i16,
 * 8 corridor, 9 strips, 10,11 lane kernels, 12 banded wave strips, 13 workgroup pipeline), second passes included; handed_back[0] = problems
 * the workgroup pipeline gave to the other banded kernels, handed_back[1] = problems a corridor / banded / strip kernel gave to the full-matrix
 * and workgroup kernels (no proof, a maximum outside 16 bits, a dry pool) */
void pga_stage_dp_routes(int64_t by_class[14], int64_t handed_back[2]);
/* mg_lchain_rmq (lchain.c:250-368) on anchors given as they are: n_seq queries, query q holding the anchors [q_aoff[q], q_aoff[q+1]) of anchors_xy
 * (two uint64 per anchor, in the order the reference's function would receive them), chained with the explicit parameters of cp.
 * mode 0: the reference's procedure as a batch runs it; 1: the same with the counting instantiation of the fast sweep kernel, whose counters
 * pga_stage_chain_routes hands out; 2: the tie-order-independent route (candidates of equal score in stable order) with need[q] != 0 where
 * an order event says the query needs the reference's procedure.  PGA_CHAIN_EXACT_ONLY=1 (read per call) sends every segment to the tree kernel.
 * Caller-allocated outputs: n_u, n_v, ev, need [n_seq]; u, f, p [n_a]; chain_xy [2 n_a].  Query q's chains are u[q_aoff[q] .. +n_u[q]), its
 * compacted anchors chain_xy[2 q_aoff[q] .. +2 n_v[q]); f[i], p[i]: score and query-local predecessor (-1: none) of EVERY anchor as the
 * backtrack reads them; ev[q]: the backtrack's order events (bit 0 a walk stopped at a mark of its own score, 1 a candidate marked by a chain
 * of its own score, 2 two chains start at one target position, 3 two chains from candidates of equal score, 4 bits 2 and 3 where it shows). */
typedef struct {
	int32_t max_gap, rmq_inner_dist, bw, max_chain_skip, rmq_size_cap, min_cnt, min_chain_score;
	float chain_gap_scale, chain_skip_scale;
	int32_t k;
} pga_chain_params_t;
int pga_stage_chain_anchors(int32_t n_seq, const uint64_t *q_aoff, const uint64_t *anchors_xy, const pga_chain_params_t *cp, int mode,
                            int32_t *n_u, int32_t *n_v, uint64_t *u, uint64_t *chain_xy, int32_t *f, int32_t *p, uint32_t *ev, uint32_t *need);
/* which branch of the chain sweep answered, summed over the mode-1 calls of pga_stage_chain_anchors since the last call of this function
 * (process-wide, copied out and zeroed): 0 segments swept by the fast kernel; 1-4 segments it handed to the tree kernel (ring overflow, tree-size
 * cap, tied minimum, too many inner candidates); 5 anchors taken by the co-linear stretch; 6 by the single-anchor shortcut; 7 inner scans
 * skipped by the f + span bound; 8 inner scans from registers; 9 in chunked form; 10 inner scans that re-ranked an unsorted window; 11 inner
 * scans stopped by max_chain_skip; 12 range-min answers taken from a block summary; 13 summary blocks scanned anchor by anchor; 14 window
 * reloads of the backtrack's walks */
#define PGA_N_CHAIN_ROUTES 15
void pga_stage_chain_routes(int64_t out[PGA_N_CHAIN_ROUTES]);
/* build_index_ex, mm_idx_cal_max_occ + mm_mapopt_update, and mm_seed_mz_flt / mm_collect_matches / collect_seed_hits (index.c:186-270, options.c:66-80,
 * seed.c:5-131, map.c:78-100,168-204) of a batch of n_grp all-vs-all groups on minimizers given as they are.  Sequence i has length lens[i] and name
 * names[i]; group g holds the sequences [grp_off[g], grp_off[g+1]); the minimizers of sequence i are mz_xy[2 mz_off[i] .. 2 mz_off[i+1]) in
 * mm_sketch's layout (x = hash << 8 | k, y = i << 32 | pos << 1 | strand).  own (or NULL): own[i] == 0 leaves query i unmapped while its
 * minimizers stay targets.  params: mid_occ > 0 is taken as given, 0 derives it per group from mid_occ_frac and the two clamps.
 * mode 0: every query's anchors in the reference's arrangement of equal keys (the replay of radix_sort_128x); 1: in stable order, as a batch
 * leaves them, with q_tie[q] != 0 where query q holds equal keys (q_tie is zeroed in mode 0).
 * Caller-allocated outputs: mid_occ [n_grp]; state [mz_off[n_seq]]: per minimizer 0 dropped by the query filter, 1 seed used, 2 seed filtered,
 * plus 4 for a tandem seed; rep_len, q_tie [n_seq]; anchor_off [n_seq + 1].  *anchors_xy (two uint64 per anchor, query q's at
 * anchor_off[q] .. anchor_off[q+1]) is freed with pga_free().
 * The kernels validate nothing, so the tap refuses by name, without a launch: a minimizer whose rid is not its sequence; positions that do not
 * ascend inside a sequence; a position outside [k - 1, len); a low byte of x other than k; a hash of 2k bits or more; duplicate names inside a
 * group; groups that are not contiguous; k or w outside the supported range; a flag bit other than the four skip_seed reads. */
typedef struct {
	int64_t flag;
	int32_t mid_occ, min_mid_occ, max_mid_occ, max_max_occ, occ_dist, w, k;
	float mid_occ_frac, q_occ_frac;
	int32_t pad;
} pga_seed_params_t;
int pga_stage_seed(int32_t n_seq, const uint32_t *lens, const char *const *names, int32_t n_grp, const int64_t *grp_off, const uint64_t *mz_off,
                   const uint64_t *mz_xy, const uint8_t *own, const pga_seed_params_t *params, int mode,
                   int32_t *mid_occ, uint8_t *state, int32_t *rep_len, uint64_t *anchor_off, uint64_t **anchors_xy, uint32_t *q_tie);
/* which branch of the stages in front of chaining answered, in every call of the process since the last call of this function (copied out and
 * zeroed): 0-3 sketch launches of k_sketch_tiles8<19>, k_sketch_tiles8<10>, k_sketch_tiles and k_sketch_serial (two per call: it counts, then
 * writes); 4 retries of the sketch's staging slabs; 5 index builds by one sort, 6 by two; 7 mid_occ batches answered by the histograms, 8 by the
 * sort; 9 queries sent through the sort replay (counted in calls of pga_stage_seed only).  Host-side counters: no launch or copy is added. */
#define PGA_N_FRONT_ROUTES 10
void pga_stage_front_routes(int64_t out[PGA_N_FRONT_ROUTES]);
/* The post-DP kernels (pga_post.hip) on explicit inputs.  Layout contract of the three device taps: sequences are base codes 0..4; they are packed
 * as the resident store is packed and laid out as pga_stage_extd2 lays them out -- request order, the FULL forward query of request i directly
 * followed by its FULL target, the first base at position 0 of the store with no padding in front (request 0 has q_off == 0, the only place
 * where the reverse-strand read below forward position 15 takes its own branch; later requests sit at whatever unaligned offsets the lengths
 * give), the tail padded with code 4.  q_start[i] is the window's start on the ALIGNED strand (q_rev[i] = 1: the reverse complement of the
 * forward query), t_start[i] its start on the target.  Request i's operation list is cigars[cigar_off[i] .. cigar_off[i+1]) (cigar_off has n + 1
 * entries; operations M, I, D, N); a list that leaves its windows is refused.  a, b, sc_ambi as pga_stage_extd2 takes them.
 * pga_stage_post_finish: mm_fix_cigar + mm_update_extra (align.c:91-167,240-289, log_gap = 1) through post_cigar_finish.  res[11 i ..] = n_cigar,
 *   qshift, tshift, blen, mlen, n_ambi, dp_max, n_gapo, n_gap, q_span, t_span; the final list of request i is written back to
 *   cigars[cigar_off[i] .. + n_cigar).
 * pga_stage_post_walk: the walk of mm_test_zdrop (align.c:32-68) through post_zdrop_walk.  res[5 i ..] = max_zdrop, t0, t1, q0, q1.
 * pga_stage_post_identity: probe i compares len[i] bases of the target from t_start[i] with len[i] bases of the aligned query strand from qs[i]
 *   through post_identity; res[i] = mismatches, or -1 for an ambiguous base or more than m_max mismatches. */
int pga_stage_post_finish(int32_t n, const uint8_t *const *q, const int32_t *qlen, const int32_t *q_start, const int32_t *q_rev,
                          const uint8_t *const *t, const int32_t *tlen, const int32_t *t_start, uint32_t *cigars, const uint64_t *cigar_off,
                          int a, int b, int sc_ambi, int gapo, int gape, int32_t *res);
int pga_stage_post_walk(int32_t n, const uint8_t *const *q, const int32_t *qlen, const int32_t *q_start, const int32_t *q_rev,
                        const uint8_t *const *t, const int32_t *tlen, const int32_t *t_start, const uint32_t *cigars, const uint64_t *cigar_off,
                        int a, int b, int sc_ambi, int gapo, int gape, int32_t *res);
int pga_stage_post_identity(int32_t n, const uint8_t *const *q, const int32_t *qlen, const int32_t *qs, const int32_t *q_rev,
                            const uint8_t *const *t, const int32_t *tlen, const int32_t *t_start, const int32_t *len, int m_max, int32_t *res);
/* the host's sufficient condition for mm_test_zdrop (align.c:47-89) to return 0 without a walk, from the gap costs, the match score, both
 * thresholds, the band w of the global pass (negative: none), its zdropped flag and score, and its operation list: 1 = the walk may be skipped.
 * A pass whose band does not cover its whole matrix is never skipped.  Host arithmetic, no device. */
int pga_stage_zdrop_impossible(int q, int e, int q2, int e2, int a, int zdrop, int zdrop_inv, int w, int zdropped, int score, int32_t n_cigar, const uint32_t *cigar);
/* The region planner (pga_plan.hip: what mm_align1 decides before its first DP call) on explicit inputs, through the production plan_regions.
 * The three records mirror PlanParams, PlanOut and PlanItem of pga_plan.h field by field.
 * Sequences are base codes 0..4, packed one behind the other in call order as the resident store is packed (sequence 0 at position 0, the tail
 * padded with code 4).  Sequences [base, n_seq) are the group: an anchor's target id t names sequence base + t.  Query j of the call is sequence
 * q_seq[j] (an index into the whole call, inside the group); its anchors are anchors_xy[2 anchor_off[j] .. 2 anchor_off[j+1]), two uint64 per
 * anchor (x = strand<<63 | target<<32 | target position, y = flags | span<<32 | query position on the aligned strand).  Region r is
 * regions[3r ..] = query index, as, cnt.  Every field of params is taken as given; the PGA_PLAN_G_MAX variable is not read, and g_max above 4096
 * is refused.
 * out[r] is the region's record; its items are (*items)[item_off[r] .. item_off[r+1]) (item_off has n_regions + 1 entries; a region whose status
 * is not 0 has none; *items is freed with pga_free()).  anchors_xy comes back as the kernels left it, flags included.
 * The kernels validate nothing, so the tap refuses by name, without a launch: a region outside its query's anchors; a cnt below 0 (cnt = 0 is
 * valid: status 3); an anchor whose target id is outside the group; an anchor whose position, or position minus k/2, falls outside its sequence;
 * a chain that is not strictly ascending on one target, strand and both coordinates. */
typedef struct {
	int32_t k, bw, bw_long, max_gap, min_cnt, min_chain_score, min_ksw_len, a, q, e, no_end_flt, probe_m_max;
	int32_t g_max, pad;
	int64_t max_sw_mat;
} pga_region_params_t;
typedef struct {
	int32_t status;                                          /* 0 ok, 2 more than g_max long gaps, 3 empty chain */
	int32_t rid, rev;
	int32_t r_rs, r_re, r_qs, r_qe, r_mlen, r_blen;
	int32_t as1, cnt1, rs, qs, rs0, qs0, re0, qe0, T_re, T_qe;
	uint32_t n_items; int32_t n_long_gaps;
} pga_region_out_t;
typedef struct {
	int32_t kind, i, rs, qs, re, qe, bw1, m, i_prev;         /* kind 0: a run of bw1 answered segments with m mismatches; 1 / 2: a segment for the DP */
	int32_t pad[3];
} pga_region_item_t;
int pga_stage_plan(int32_t n_seq, const uint8_t *const *seq, const int32_t *seq_len, int32_t base, int32_t n_q, const int32_t *q_seq,
                   const uint64_t *anchor_off, uint64_t *anchors_xy, int32_t n_regions, const int32_t *regions, const pga_region_params_t *params,
                   pga_region_out_t *out, pga_region_item_t **items, uint64_t *item_off);
/* radix_sort_128x (ksort.h:101-151, misc.c:155-159), the exact replay incl. the arrangement of equal keys: sorts every array
 * [seg_off[s], seg_off[s+1]) of the n_seg arrays in xy (two uint64 per record: x = key, y = payload) in place */
int pga_stage_sort(int32_t n_seg, const uint64_t *seg_off, uint64_t *xy);

/* ---- the step right behind find_matches (packages/pangraph/src/pangraph/graph_merging.rs:95-128 self_merge) ----
 * flags & 1: drop self matches (qry == ref inside a group, :107) and split every match at indels >= indel_len_threshold, with side
 * patches (pangraph/split_matches.rs:13-237; the reference's default threshold is 100, align/alignment_args.rs:8-11);
 * flags & 2: filter_matches per group (:187-216): alignment_energy2 (align/energy.rs:37-54, defaults alpha 100, beta 10) < 0, stable
 * sort by energy, greedy acceptance of matches whose query and reference intervals overlap no accepted interval of the same block.
 * Records come back in the same layout, group by group (ascending), accepted matches in energy order; ties keep the order of the
 * input records (the reference's tie order is that of its parallel aligner: undefined).  A CIGAR operation other than M I D = X
 * inside a kept stretch is an error, as in the reference (:62-65).  The result is freed with pga_result_free(). */
typedef struct { int32_t indel_len_threshold; int32_t flags; double alpha, beta; } pga_filter_params_t;
int pga_filter_matches(int64_t n, const pga_match_t *matches, const uint32_t *cigars, uint64_t n_ops, const pga_filter_params_t *fp, pga_result_t **out);
int pga_result_filter(const pga_result_t *res, const pga_filter_params_t *fp, pga_result_t **out);

/* ---- the guide tree (packages/pangraph/src/commands/build/build_run.rs:100 build_tree_using_neighbor_joining) ----
 * pga_mash_distance replaces distance/mash/mash_distance.rs:9-65 (minimizers_sketch of every sequence, minimizer.rs:49-160, with
 * MinimizersParams k, w -- the reference uses the defaults 15 and 100 -- then 1 - shared / own distinct minimizer values):
 * dist is n x n doubles, row major.  pga_guide_tree_nj replaces tree/neighbor_joining.rs:16-103: leaves are nodes 0..n-1 in input
 * order, join t (0-based) creates node n + t with children merges[2t] and merges[2t+1] (first the node that stood earlier in the
 * reference's node list); the last join is the root.  pga_guide_tree does both without moving the matrix through the host
 * (dist may be NULL).  A sequence without any minimizer is an error, as in the reference (it panics, mash_distance.rs:19-20).
 * No limit on n other than the n x n matrix in device memory (up to 2048 sequences the joining state lives in LDS, above that in
 * device memory).  pga_guide_tree_nj requires a SYMMETRIC matrix (what mash_distance produces) and returns -1 otherwise: the
 * reference's Q uses row sums and column sums, which the kernel takes from one pass.
 * Returns 0, or -1 with the message in pga_last_error(). */
int pga_mash_distance(int32_t n, const char *const *seqs, const uint32_t *lens, int k, int w, double *dist);
int pga_guide_tree_nj(int32_t n, const double *dist, int32_t *merges);
int pga_guide_tree(int32_t n, const char *const *seqs, const uint32_t *lens, int k, int w, double *dist, int32_t *merges);
/* The joining step picks the smallest Q (neighbor_joining.rs:77-96); its row and column sums are f64 sums taken in ndarray's order as
 * restated here (not pinned against ndarray itself).  pga_nj_near_ties() = the number of joins of the calling thread's
 * last pga_guide_tree_nj / pga_guide_tree call in which the Q of ANOTHER pair came within the error a different summation order can make
 * (8 m^2 2^-53 max|d| at m live nodes) of the chosen one; *first_join (may be NULL) = the first such join, -1 if none.  The joins at
 * m = 4 and m = 3 are left out of the count: there the Q of complementary pairs (at m = 3: of all pairs) are equal in exact arithmetic, so
 * the last two joins of EVERY tree -- the root and its children -- are decided by the rounding of these sums, in the reference as here.
 * 0 means no other join depends on the order the sums are taken in; otherwise a caller that needs the reference's tree bit for bit can
 * run its own joining on the distance matrix. */
int32_t pga_nj_near_ties(int32_t *first_join);
/* stage tap: the minimizers of every sequence in the reference's order (value = Minimizer.value, position = Minimizer.position with
 * the sequence's index as id); seq_off has n + 1 entries */
int pga_stage_mash_sketch(int32_t n, const char *const *seqs, const uint32_t *lens, int k, int w, uint64_t **value, uint64_t **position, uint64_t *seq_off);
/* ---- the re-alignment of a merged block's member sequences onto the anchor consensus ----
 * pga_map_variations replaces the loop of MergePromise::solve_promise (packages/pangraph/src/pangraph/reweave.rs:40-94) over
 * map_variations (packages/pangraph/src/align/map_variations.rs:39-77): align_with_nextclade (align/nextclade/align_with_nextclade.rs:
 * 24-75) = banded global alignment with free terminal gaps over simple_stripes(mean_shift, band_width + extra_band_width)
 * (align/nextclade/align/{band_2d.rs:36-57, score_matrix.rs:23-199, backtrace.rs:17-85}), the band doubled while the path touches
 * its boundary (align/nextclade/align/align.rs:55-62), then insertions_strip / find_nuc_changes and the terminal deletions.
 * One job per member sequence; ref and qry are upper-case IUPAC letters (not NUL-terminated); jobs that share a consensus should
 * pass the same pointer (it is uploaded once).  The caller keeps Edit::apply, reverse_complement and BandParameters::from_edits
 * (reweave.rs:53-75): the entry for hosts that already hold member sequences.  A host that holds a block as pangraph does, a consensus and
 * one edit list per member, calls pga_solve_promises below, which does those three on the way.  Per job: status 0, or the reference's error -- 1 the query is shorter than min_length (align.rs:42-46),
 * 2 a letter to_nuc rejects (alphabet/nuc.rs:99-121) or a literal '-' in ref / qry (to_nuc accepts it, the edit extraction of the reference would
 * read it as an alignment gap; block sequences never contain one, so it is rejected instead of reproduced), 3 the traceback left the band (the reference panics).  Substitutions in
 * reference order, deletions as the reference pushes them (internal ones ascending, then the leading, then the trailing one),
 * insertions ascending with pangraph's position convention (map_variations.rs:71-74).  The four arrays are freed with pga_free().
 * Returns 0, or -1 with the message in pga_last_error(). */
typedef struct {
	int32_t score_match, penalty_mismatch, penalty_gap_open, penalty_gap_extend;   /* NextalignParams::default(): 3, 1, 6, 0 (params.rs:142-170) */
	int32_t left_terminal_gaps_free, right_terminal_gaps_free, gap_align_left;     /* 1, 1, 1 */
	int32_t min_length, max_alignment_attempts, extra_band_width;                  /* map_variations.rs:45-52: 1, args (4), args (5) (build_args.rs:76-85) */
} pga_mapvar_params_t;
typedef struct { const char *ref, *qry; uint32_t ref_len, qry_len; int32_t mean_shift; uint32_t band_width; } pga_mapvar_job_t;
typedef struct { uint32_t pos, alt; } pga_sub_t;                    /* Sub { pos, alt }: alt is the query's letter */
typedef struct { uint32_t pos, len; } pga_del_t;                    /* Del { pos, len } */
typedef struct { uint32_t pos, len; uint64_t seq_off; } pga_ins_t;  /* Ins { pos, seq = ins_seq[seq_off .. seq_off + len) } */
typedef struct {
	int32_t status, score, attempts, hit_boundary;
	uint32_t n_subs, n_dels, n_inss, n_ins_bases;
	uint64_t sub_off, del_off, ins_off;                             /* first entry of the job in subs / dels / inss */
} pga_mapvar_res_t;
int pga_map_variations(int64_t n_jobs, const pga_mapvar_job_t *jobs, const pga_mapvar_params_t *params, pga_mapvar_res_t *res,
                       pga_sub_t **subs, pga_del_t **dels, pga_ins_t **inss, char **ins_seq);
void pga_free(void *p);

/* ---- reconsensus of the blocks a merge updated ----
 * pga_reconsensus replaces, for all updated blocks at once, analyze_blocks_for_reconsensus and the per-block work of reconsensus_graph
 * (packages/pangraph/src/reconsensus/reconsensus.rs:32-126): find_majority_edits (pangraph/pangraph_block.rs:191-256: an edit shared by more
 * than depth / 2 members), then per block either nothing (kind 0), apply_substitutions_to_block (kind 1: the consensus letters change, every
 * member's substitutions are reconciled, edits.rs:196-238) or edit_consensus_and_realign (kind 2, pangraph_block.rs:295-332: the majority
 * edits applied to the consensus, every member's sequence rebuilt with Edit::apply and re-aligned by map_variations with the band of
 * BandParameters::from_edits).  Counting, Edit::apply, reconciliation and the re-alignment run on the device; sequences built there feed the
 * aligner without leaving it.  detach_unaligned_nodes on the realigned blocks (reconsensus.rs:85) is pga_detach_unaligned below, fed from this
 * entry's output; the node / path maps (reconsensus.rs:76-88) are pga_close_round's, further down.
 * Input: the members of block b are the next blocks[b].n_members entries of members[] (the reference's BTreeMap order), the edits of a
 * member the next n_subs / n_dels / n_inss entries of subs / dels / inss (insertion letters: ins_seq[seq_off .. seq_off + len)).
 * Output (freed with pga_rc_free): per block its kind, its consensus afterwards and its majority edits; per member (input order) its edits
 * against that consensus as a pga_mapvar_res_t (offsets into out->subs / dels / inss; kind 0: the input edits).  A negative kind is the
 * reference's error for that block (-2 a majority letter equals the consensus letter, -3 empty consensus, -4 no aligned position,
 * -5 a member holds a substitution and a deletion, or two substitutions, at one position); a block with a negative kind comes back with its
 * ORIGINAL consensus and the original edits of every member (status: the member's own code).  Member status 7: no aligned position
 * (map_variations.rs:32), otherwise the codes of pga_map_variations -- a caller checks the member status also when kind == 2 (a member
 * without an aligned position does not fail its block).  Returns 0, or -1 with the message in pga_last_error(). */
typedef struct { const char *consensus; uint32_t cons_len, n_members; } pga_rc_block_t;
typedef struct { uint32_t n_subs, n_dels, n_inss; } pga_rc_member_t;
typedef struct {
	int32_t kind; uint32_t cons_len; uint64_t cons_off;                  /* consensus afterwards: out->cons[cons_off .. cons_off + cons_len) */
	uint32_t n_subs, n_dels, n_inss; uint64_t sub_off, del_off, ins_off; /* majority edits: out->m_subs / m_dels / m_inss (letters in out->m_ins_seq) */
} pga_rc_block_res_t;
typedef struct {
	pga_rc_block_res_t *blocks; pga_mapvar_res_t *members;
	pga_sub_t *subs; pga_del_t *dels; pga_ins_t *inss; char *ins_seq;
	pga_sub_t *m_subs; pga_del_t *m_dels; pga_ins_t *m_inss; char *m_ins_seq;
	char *cons;
} pga_rc_out_t;
int pga_reconsensus(int64_t n_blocks, const pga_rc_block_t *blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels,
                    const pga_ins_t *inss, const char *ins_seq, const pga_mapvar_params_t *params, pga_rc_out_t *out);
void pga_rc_free(pga_rc_out_t *out);

/* ---- SURVEY 8(f)-1, the whole step: MergePromise::solve_promise (packages/pangraph/src/pangraph/reweave.rs:40-94) for all promises of a merge ----
 * pga_solve_promises takes what a pangraph host holds -- per promise the two consensus sequences, the orientation and the CIGAR of the
 * match, per member of the append block its edits against the append consensus -- and returns every member's edits against the ANCHOR
 * consensus.  Member sequences are built on the device and feed the aligner there; what is handed over is the consensus sequences and the
 * edit lists.  Input layout as for pga_reconsensus: the members of promise p are the next promises[p].n_members entries of members[] (the
 * reference's BTreeMap order), a member's edits the next n_subs / n_dels / n_inss entries of subs / dels / inss.  Output layout as for
 * pga_map_variations: res[m] (one per member, input order) holds offsets into the four arrays, which are freed with pga_free(); the
 * arrays are packed member by member in input order.  Promises onto the same consensus should pass the same pointer (uploaded once).
 * Per member, in the reference's order (reweave.rs:46-81):
 *   1. the cigar band: BandParameters::from_edits(Edit::from_cigar(cigar), anchor_len) (edits.rs:538-566; M = X advance, I an insertion at
 *      the current position, D a deletion), once per promise.  No aligned position: status 8 for EVERY member of the promise, the empty
 *      ones included (the reference fails before its loop).
 *   2. seq = edits.apply(append consensus) (edits.rs:307-329, list-order rules as in pga_reconsensus).  An empty seq: status 0 and the
 *      single deletion (0, anchor_len); no alignment, no band, orientation ignored.
 *   3. reverse != 0: seq is reverse-complemented with the table of io/seq.rs:9-29 (ACGTYRWSKMDVHBN- and nothing else; lower case is
 *      rejected) and the band of step 4 is that of edits.reverse_complement(append_len) (edits.rs:257-276: sub len-pos-1, del
 *      len-pos-len, ins len-pos, each list stably sorted by position).  A rejected letter in the sequence or in an edit: status 9.
 *   4. the member band: BandParameters::from_edits(edits as oriented, append_len); no aligned position: status 7 (as pga_reconsensus).
 *      mean_shift and band_width are the sums of the cigar's and the member's (map_variations.rs:23-26).
 *   5. map_variations(anchor consensus, seq, band): status 1, 2, 3 as pga_map_variations; extra_band_width is added inside, as there.
 * A literal '-' in a consensus or in an insertion is handled as pga_reconsensus handles it: it is NOT stripped by the apply step (the
 * reference's Edit::apply would drop it with the gaps of its deletions, edits.rs:326), it stays in the sequence, and the alignment rejects
 * the member with status 2 (forward or reverse: '-' complements to itself).  Block sequences never contain one.
 * Malformed input fails the call (-1; the reference panics or hits unimplemented!): a CIGAR operation other than M I D = X, an edit
 * position or interval outside the append consensus, a NULL sequence with a non-zero length.
 * PGA_PROMISE_CHUNK_MB (default 2048) caps the built sequences held on the device at once; promises are processed in chunks under it
 * (a single promise is never split) and the result does not depend on it.  Returns 0, or -1 with the message in pga_last_error(). */
typedef struct {
	const char *anchor; uint32_t anchor_len;     /* anchor_block.consensus() */
	const char *append; uint32_t append_len;     /* append_block.consensus() */
	int32_t reverse;                             /* !orientation.is_forward() */
	const uint32_t *cigar; uint32_t n_cigar;     /* minimap2 packing: len << 4 | op, op in M(0) I(1) D(2) =(7) X(8) */
	uint32_t n_members;                          /* append_block.alignments(), BTreeMap order */
} pga_promise_t;
int pga_solve_promises(int64_t n_promises, const pga_promise_t *promises, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels,
                       const pga_ins_t *inss, const char *ins_seq, const pga_mapvar_params_t *params, pga_mapvar_res_t *res,
                       pga_sub_t **out_subs, pga_del_t **out_dels, pga_ins_t **out_inss, char **out_ins_seq);
/* stage tap: steps 1-4 alone.  Per member (input order) the status reached before alignment (0, 7, 8 or 9; 0 with an empty sequence
 * for the member of step 2), the summed band before extra_band_width (0, 0 where the status is not 0 or the sequence is empty) and the
 * oriented sequence as the aligner would read it: seqs[seq_off[m] .. seq_off[m + 1]), empty where the status is not 0.  seq_off has one
 * more entry than there are members; *seqs is freed with pga_free(). */
int pga_stage_promise_jobs(int64_t n_promises, const pga_promise_t *promises, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels,
                           const pga_ins_t *inss, const char *ins_seq, int32_t *status, int32_t *mean_shift, uint32_t *band_width, uint64_t *seq_off, char **seqs);

/* ---- between the two: block_slice (packages/pangraph/src/pangraph/slice.rs:12-202) for every interval a merge cuts its blocks into ----
 * pga_slice_blocks replaces the loop of reweave.rs:427-438 over split_block (reweave.rs:342-402): for every block that takes part in a
 * merge and every interval of it, every member's edits are filtered, clipped and shifted (slice.rs:12-53), its coordinates inside the
 * interval computed (interval_node_coords, slice.rs:103-127), from those the new node's position on its path and its strand
 * (new_position_circular / _non_circular, new_strandedness, slice.rs:55-101), and the member left out of the slice when its alignment has
 * become empty (Edit::is_empty_alignment, edits.rs:351-367).  The aligned slices are the append_block / anchor_block of the
 * MergePromises: pga_result_filter -> pga_plan_merge -> pga_slice_blocks -> pga_solve_promises is a merge in one data layout.
 * extract_intervals, the block ids and group_promises / update_cigar are pga_plan_merge below; the node ids and graph.update are
 * pga_apply_merge further below.
 * Input layout as for pga_reconsensus: the members of block b are the next blocks[b].n_members entries of members[] and of nodes[], its
 * intervals the next blocks[b].n_intervals entries of intervals[], a member's edits the next n_subs / n_dels / n_inss entries of subs /
 * dels / inss.  Insertion letters are not read (only pga_ins_t.len) and not copied: a sliced insertion keeps its seq_off into the
 * caller's ins_seq.  Consensus letters are not read either: the consensus of a slice is consensus + start, end - start letters.
 * Output (freed with pga_slice_free): slices[] ordered by (block, interval); the kept members of a slice are members[member_off ..
 * member_off + n_kept) in input member order, their edits packed in that order, so that counts + member_off and subs + sub_off /
 * dels + del_off / inss + ins_off of the slice's first kept member are what pga_solve_promises and pga_reconsensus take (pointer
 * arithmetic only; the caller's ins_seq goes with them unchanged); dropped[] holds, slice after slice (n_dropped each, starting at the sum of the n_dropped
 * before), the member indices whose slice is empty -- the None entries of node_updates (slice.rs:187-190).
 *   substitutions  kept iff start <= pos < end; pos -= start; list order kept
 *   deletions      kept iff end > pos && start < pos + len, clipped to the interval and shifted (a zero-length one strictly inside an
 *                  interval is kept, one at pos == start is not; a deletion appears in every interval it overlaps)
 *   insertions     kept iff start <= pos < end, or pos == cons_len == end; pos -= start
 *   coordinates    slice.rs:103-127 as written: node_start = start - D(start) + I(start), node_end = end - D(end) + I(end) plus the
 *                  insertions at cons_len when end == cons_len; D(x) = the deleted positions below x, a position that two deletions share
 *                  counted twice as there, I(x) = the letters inserted before x
 *   position       64-bit; circular paths modulo path_len (a node over its whole path comes out as (0, 0))
 *   emptiness      no inserted letter, deletion lengths >= end - start, and the union of the deletions covers the slice (what
 *                  apply(...).len() == 0 says; lengths that add up over a gap are not empty).  A literal '-' in a consensus or a
 *                  substitution to '-' is treated as the other entries treat it: NOT stripped (the reference's Edit::apply would drop it
 *                  with the gaps of its deletions); block sequences never contain one.
 * The intervals of a block are sorted by start, non-empty, disjoint and inside [0, cons_len]; the reference's tile the block
 * (pangraph_interval.rs:57-96), gaps between them are allowed here and receive nothing.  Malformed input fails the call (-1, message in
 * pga_last_error(); the reference panics or trips sanity_check): intervals that break that rule, an edit position or deletion end
 * beyond cons_len, cons_len == 0, a NULL list with a non-zero count, a circular node with path_len == 0, a reverse node whose pos_end
 * (plus path_len on a circular path) is smaller than its node_end, overlapping deletions that remove more positions than lie before an
 * interval boundary (usize underflow in slice.rs:108/112), more than 2^32 edits of one kind in one block. */
typedef struct { const char *consensus; uint32_t cons_len, n_members, n_intervals; } pga_slice_block_t;
typedef struct { uint32_t start, end; int32_t flip; } pga_slice_interval_t;   /* flip = aligned && !is_anchor && the orientation is reverse: new_strandedness reverses the strand */
typedef struct { uint64_t pos_start, pos_end, path_len; int32_t reverse, circular; } pga_slice_node_t;   /* the OLD node of a member: position(), its path's tot_len, strand, circular() */
typedef struct {
	uint32_t member;                  /* index of the member inside its block (input order) */
	int32_t  reverse;                 /* new strand */
	uint32_t node_start, node_end;    /* interval_node_coords */
	uint64_t pos_start, pos_end;      /* new position on the path */
	pga_rc_member_t counts;           /* n_subs, n_dels, n_inss of the sliced edit */
	uint64_t sub_off, del_off, ins_off;   /* its first entry in out->subs / dels / inss */
} pga_slice_member_t;
typedef struct { uint64_t member_off; uint32_t n_kept, n_dropped; } pga_slice_res_t;   /* one per (block, interval) */
typedef struct {
	pga_slice_res_t *slices; pga_slice_member_t *members;
	pga_rc_member_t *counts;          /* counts[k] == members[k].counts, packed: the members[] argument of pga_solve_promises / pga_reconsensus */
	uint32_t *dropped; pga_sub_t *subs; pga_del_t *dels; pga_ins_t *inss;
} pga_slice_out_t;
int pga_slice_blocks(int64_t n_blocks, const pga_slice_block_t *blocks, const pga_slice_interval_t *intervals, const pga_rc_member_t *members, const pga_slice_node_t *nodes,
                     const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss, pga_slice_out_t *out);
void pga_slice_free(pga_slice_out_t *out);

/* ---- back from a graph to its genomes: reconstruct (packages/pangraph/src/commands/reconstruct/reconstruct_run.rs:56-127) ----
 * pga_reconstruct rebuilds the sequence of every path -- the whole of `pangraph reconstruct`, the check behind `pangraph build --verify`
 * (build_run.rs:37-64, 174-178) and the debug check after every merge (build_run.rs:141-148) -- and, in verify mode, compares it on the
 * device with the sequence the caller expects, so that only a verdict per path comes back.  Blocks, members and edits in the layout of
 * pga_reconsensus (members numbered globally in block order); the nodes of path p are the next paths[p].n_nodes entries of nodes[].
 * Per path, as the reference does it:
 *   1. every node, in order: Edit::apply of its member's edits to the block's consensus (edits.rs:307-329, list-order rules as in
 *      pga_reconsensus), reverse-complemented when nodes[].reverse != 0 (io/seq.rs:9-33: ACGTYRWSKMDVHBN- and nothing else, lower case is
 *      rejected).  The letters of a forward node are not checked.  Two nodes may name the same member.
 *   2. the concatenation must have paths[p].tot_len letters;
 *   3. it is rotated right by first_pos (Vec::rotate_right: letter j moves to (j + first_pos) mod len); no other node's position is read,
 *      and neither is `circular`;
 *   4. a path without nodes is the empty sequence (tot_len and first_pos are not read).
 * res[p].status, the first that applies (the reference's own order, this entry's refusal 3 behind the reference's Err 2):
 *   0  built
 *   2  a reverse node emits a letter the complement table rejects (the reference's Err)
 *   3  a '-' would be emitted, from the consensus, an insertion or a substitution that no deletion hides: Edit::apply strips every '-'
 *      (edits.rs:326) where pga_reconsensus and pga_solve_promises keep it; block sequences never hold one, so this entry does neither and refuses
 *   1  the built length differs from tot_len (the reference's Err)
 *   4  first_pos exceeds the built length (the reference panics)
 *   5  verify mode only: the built length differs from expected_len[p]; nothing is compared
 * A substitution under a deletion is never emitted and triggers neither 2 nor 3.  A path with status 1 or 4 is still built (unrotated),
 * so that 2 and 3 are found.  The other paths of the call are not affected by any status.  res[p].len is always the built length.
 * Write mode (out_seq != NULL): *out_seq is one malloc()ed buffer, freed with pga_free(); the sequence of a path with status 0 is
 * (*out_seq)[seq_off .. seq_off + len) (every seq_off is a multiple of 16; the letters between two paths are padding).  A path with another
 * status returns no letters: its seq_off is 0 and nothing is to be read for it.
 * Verify mode (expected != NULL, and then expected_len != NULL): path p is compared with the expected_len[p] letters at expected[p] (not
 * NUL-terminated).  first_mismatch is the index, in the final rotated sequence, of the first differing letter, or -1; n_mismatch the
 * number of differing letters.  Both are -1 / 0 where status != 0.  No sequence is downloaded unless out_seq is given as well, and in
 * verify-only mode none is stored on the device either.  Without verify mode first_mismatch is -1 and n_mismatch 0.
 * Both modes may be given in one call; a call with neither fails.
 * Malformed input fails the call (-1, message in pga_last_error(); nothing has run on the device by then): a NULL list with a non-zero
 * count, a NULL consensus with a non-zero length, a consensus of 2^30 letters or more, an edit position or interval beyond its consensus
 * (the rules of pga_solve_promises), a substitution letter outside one byte, a node whose member is out of range, a member or a path longer
 * than 2^31 letters, a NULL expected[p] with a non-zero length.
 * PGA_RECON_CHUNK_MB (default 2048) caps the built letters held on the device at once: paths are processed in chunks under it (a longer
 * single path is a chunk of its own), `expected` is uploaded chunk by chunk, and of the graph only what the chunk's nodes read goes to
 * the device: their runs (worked out on the host from the edits), the distinct consensus sequences and the insertion letters.  The result
 * does not depend on the chunking.  Measurement: the kernel's intervals are logged as family 15 of pga_busy_begin / pga_busy_end.
 * Returns 0, or -1 with the message in pga_last_error(). */
typedef struct { uint64_t tot_len, first_pos; uint32_t n_nodes, pad; } pga_recon_path_t;   /* path.tot_len(), position().0 of the FIRST node, path.nodes.len() */
typedef struct { uint64_t member; int32_t reverse, pad; } pga_recon_node_t;                 /* global index into members[]; strand().is_reverse() */
typedef struct { int32_t status, pad; uint64_t len, seq_off; int64_t first_mismatch, n_mismatch; } pga_recon_res_t;
int pga_reconstruct(int64_t n_blocks, const pga_rc_block_t *blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels,
                    const pga_ins_t *inss, const char *ins_seq, int64_t n_paths, const pga_recon_path_t *paths, const pga_recon_node_t *nodes,
                    const char *const *expected, const uint64_t *expected_len, pga_recon_res_t *res, char **out_seq);

/* ---- the exports of a finished graph, streamed: export block-sequences (pangraph_block.rs:135-189) and export core-genome
 * (export_core_genome.rs:53-141) ----
 * Both build ROWS of letters on the device from blocks, members and edits in the layout of pga_reconstruct and hand them to a SINK of the
 * caller's tile by tile; the library keeps no row and downloads letters into its cached pinned blocks only.
 *   pga_block_sequences  one row per member (global member order): aligned != 0: Edit::apply_aligned of its edits to the block's
 *                        consensus (edits.rs:331-347: substitutions, then '-' at every deleted position, insertions missing; the row has
 *                        cons_len letters); aligned == 0: Edit::apply WITHOUT the stripping of '-' (edits.rs:307-329, as pga_reconstruct).
 *   pga_core_alignment   one row per path: the core blocks (Pangraph::core_block_ids, pangraph.rs:235-255: present exactly once in each
 *                        path; member_path[m] is the path of global member m) in the order the guide nodes name them, each the sequence
 *                        of the path's member of that block as above, reverse-complemented (io/seq.rs:9-33) where the guide node is
 *                        reverse.  *core (malloc()ed, freed with pga_free(), *n_core entries) lists them with their first column.
 * res[r] (r: the row's own index, whatever `order` is): len is the built length; status, the first that applies:
 *   0  built
 *   2  a reverse piece emits a letter the complement table rejects (the reference's Err)
 *   3  unaligned mode only: a '-' is emitted, from the consensus, an insertion or a substitution (Edit::apply would strip it)
 * order: NULL, or a permutation of the rows: they are built and delivered in that order (the record order of the reference's output, say).
 * sink == NULL, verdict mode: statuses and lengths only, nothing but flags leaves the device.  A caller that must emit nothing when a row
 * fails (the reference's export returns Err) calls this first.
 * sink != NULL: called on the calling thread, once per tile of at most PGA_EXPORT_TILE_KB KB (default 16384; a multiple of 4, read at
 * every call), tiles in delivery order: letters [row_off, row_off + n) of row segs[i].row are letters[segs[i].tile_off ..]; the segments of
 * a call are in delivery order, exclude the padding between rows and empty rows, and over the calls tile every non-empty row exactly once.
 * `letters` and `segs` are the library's and valid during the call only.  Letters are delivered AS BUILT, whatever the row's status
 * turns out to be: res[] is complete when the entry returns.  A sink that returns non-zero stops the export: what is in flight is
 * drained, no further call is made, the entry returns -1 ("sink stopped the export").
 * PGA_EXPORT_RUNS_KB (default 262144, at least 1, read at every call) caps the run tables held at once: rows are processed in chunks under
 * it (a single larger row is a chunk of its own).  Neither knob changes a result.
 * Malformed input fails the call (-1, message in pga_last_error(); nothing has run on the device by then): what fails pga_reconstruct, a
 * row over 2^31 letters, an `order` that is no permutation, a member_path or guide_path naming no path, a guide node whose member does
 * not exist or is not on guide_path, a core block the guide nodes name twice or not at all.  n_paths == 0 gives no row and no core block.
 * Measurement: the kernel's intervals are logged as family 16 of pga_busy_begin / pga_busy_end. */
typedef struct { uint64_t row, row_off, tile_off; uint32_t n, pad; } pga_export_seg_t;
typedef int (*pga_export_sink_t)(void *ctx, int64_t n_seg, const pga_export_seg_t *segs, const char *letters);
typedef struct { int32_t status, pad; uint64_t len; } pga_export_res_t;
typedef struct { uint32_t block; int32_t reverse; uint64_t col; uint32_t cons_len, pad; } pga_core_block_t;   /* col: the first column of the block in every row */
int pga_block_sequences(int64_t n_blocks, const pga_rc_block_t *blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels,
                        const pga_ins_t *inss, const char *ins_seq, int aligned, const uint64_t *order, pga_export_res_t *res /* one per member */,
                        pga_export_sink_t sink, void *ctx);
int pga_core_alignment(int64_t n_blocks, const pga_rc_block_t *blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels,
                       const pga_ins_t *inss, const char *ins_seq, const uint32_t *member_path, int64_t n_paths, int64_t guide_path, int64_t n_guide_nodes,
                       const pga_recon_node_t *guide_nodes, int aligned, const uint64_t *order, pga_export_res_t *res /* one per path */,
                       pga_core_block_t **core, int64_t *n_core, pga_export_sink_t sink, void *ctx);

/* ---- simplify: the block concatenations of remove_transitive_edges (packages/pangraph/src/circularize/merge_blocks.rs:92-148) ----
 * pga_merge_blocks performs any number of independent concatenations in one call: per edge concatenate_alignments of the left and the right
 * block, each taken as it is or through PangraphBlock::reverse_complement (pangraph_block.rs:63-75) first.  orient_merging_edge,
 * find_node_pairings, the node ids and the path / node updates are not part of this call: pga_plan_simplify (below) does them for a whole
 * round and hands over `edges` and `partner` as this call takes them; pangraph_amd/simplify.py also keeps them as host functions.  Blocks,
 * members and edits in the layout of pga_reconstruct; a block may be named by several edges, inputs are only read.
 * partner: for edge e the next blocks[left].n_members entries; entry k is the index, inside the right block, of the member joined with
 * the k-th member of the left block (node_map of concatenate_alignments) -- a permutation of the right block's members.
 * Per edge, exactly as the reference (the list order is observable: its Edit compares Vecs):
 *   X' = X, or with *_rc the consensus reverse-complemented (io/seq.rs:9-33) and every member's edit Edit::reverse_complement(len)
 *        (edits.rs:257-276): sub pos -> len-pos-1, alt complemented; del pos -> len-pos-len_d; ins pos -> len-pos, letters
 *        reverse-complemented; each list then STABLY sorted by position
 *   consensus  left' ++ right'
 *   member k   e_left'.concat(e_right'.shift(L_left)) (edits.rs:278-304): subs and dels the left list followed by the shifted right list,
 *        not re-sorted; inss the left list, then every right insertion in order either appended to the FIRST insertion already in the
 *        accumulated list with the same position (its letters extended) or pushed -- a left insertion at L_left and a right one at 0 become
 *        one, right insertions that share a position become one, equal positions inside the left list stay separate
 * Output (freed with pga_merge_free) in the same layout, so that out->blocks, out->members, out->subs / dels / inss and out->ins_seq are
 * the first arguments of the next pga_merge_blocks call or of pga_reconstruct (n_blocks = n_edges) by pointer arithmetic only: blocks[e]
 * has its consensus in out->cons (every consensus at a multiple of 16), cons_len = L_left + L_right and the left block's n_members;
 * members[] edge after edge in the LEFT block's member order (edges[e].member_off is the edge's first), the edits packed in that order.
 * out->ins_seq holds new letters: every output insertion's seq_off points into it (a member's letters start at a multiple of 16), none
 * into the caller's buffer.
 * edges[e].status: 0 built; 2 a block taken with *_rc holds a letter the complement table rejects (the reference's Err) -- in its
 * consensus, an insertion or a substitution's alt, also one that lies under a deletion.  A status-2 edge keeps its slots: counts and
 * offsets do not depend on a status; its letters are as built and not to be used.  Other edges are not affected.
 * Malformed input fails the call before anything is launched (-1, message in pga_last_error()): what fails pga_reconstruct, an edge that
 * names a block out of range, two blocks of different depth, a partner that is no permutation, L_left + L_right >= 2^30, more than 2^30
 * inserted letters in one member.  cons_len == 0 and n_members == 0 are legal.  n_edges == 0 returns empty lists without a device call. */
typedef struct { uint32_t left, right; int32_t left_rc, right_rc; } pga_merge_edge_t;   /* block indices; *_rc: reverse_complement first */
typedef struct { int32_t status, pad; uint64_t member_off; } pga_merge_res_t;          /* one per edge */
typedef struct {
	pga_merge_res_t *edges;
	pga_rc_block_t  *blocks;     /* one per edge */
	pga_rc_member_t *members;    /* edge after edge, in the left block's member order */
	pga_sub_t *subs; pga_del_t *dels; pga_ins_t *inss; char *ins_seq; char *cons;
} pga_merge_out_t;
int pga_merge_blocks(int64_t n_blocks, const pga_rc_block_t *blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels,
                     const pga_ins_t *inss, const char *ins_seq, int64_t n_edges, const pga_merge_edge_t *edges, const uint32_t *partner, pga_merge_out_t *out);
void pga_merge_free(pga_merge_out_t *out);

/* ---- simplify: the path side of one round of remove_transitive_edges (circularize/circularize.rs:11-76 find_transitive_edges / count_edges,
 * circularize/merge_blocks.rs:33-89 orient_merging_edge / find_node_pairings, :196-234 graph_merging_update_paths / _nodes) ----
 * pga_plan_simplify counts the edges of every path, lists the transitive ones, chooses a round of disjoint edges, orients them, pairs the
 * nodes of every chosen edge, makes the new nodes with their ids and rewrites the paths: what pga_merge_blocks leaves to its caller, for all
 * edges of the round in one call.  Input flat and only read:
 *   blocks[n_blocks]   the alive ones in strictly ascending block_id, so that index order is the reference's BTreeMap order; entries with
 *                      alive == 0 are skipped and no node may name one.  depth = alignments.len().
 *   paths[n_paths]     ascending path_id; its nodes are nodes[node_off .. node_off + n_nodes), node_off the running sum; n_nodes == 0 is legal.
 *   nodes[n_nodes]     path after path.  block: index into blocks; member: the node's slot in that block's member order, the numbering of
 *                      the block arrays given to pga_merge_blocks.  Every (block, member) slot is named by exactly one node.
 *   sched[n_sched]     NULL: the defined round -- the transitive edges in sorted order, each taken while both of its blocks are unused in
 *                      the round.  Otherwise the round's edges, in either orientation; each must be transitive and no block named twice.
 *   flags              PGA_TOPO_EDGES_ONLY: stop behind the transitive list.  PGA_TOPO_COUNTS: also return every counted edge (edge_counts).
 * An EDGE is the pair (block, strand) -> (block, strand) of a node and its successor on the path (the first node behind the last of a
 * circular path), in Edge::conventional_orientation: as it stands when b1 < b2 (b1 == b2: when s1 is forward), else inverted
 * ((b2, !s2), (b1, !s1)).  Strands: 0 forward, 1 reverse.  An edge is transitive when b1 != b2 and count == depth[b1] == depth[b2].
 * Output (freed with pga_topo_free), all exact integers:
 *   transitive[]       by (b1, b2, s1, s2), block indices.  Two different edges between the same two blocks both appear.
 *   edge_counts[]      (PGA_TOPO_COUNTS) every edge seen, the same order, self-loops included.
 *   round[]            one per chosen edge in the order chosen: the oriented edge, anchor first (the longer consensus, on a tie the smaller
 *                      block_id), its index in transitive[], `merge` = (left, right, left_rc, right_rc) by merge_blocks.rs:100-111
 *                      ((anchor, other, 0, rc) when the anchor's strand is forward, else (other, anchor, rc, 0), rc = the strands
 *                      differ) as block indices of THIS graph, and partner_off.
 *   partner[]          edge after edge; entry partner_off + k is the slot in the right block joined with slot k of the left block: the
 *                      partner argument of pga_merge_blocks in the same edge order.
 *   new_nodes[]        same indexing: node_id = XXH64, seed 0, of the five little-endian u64 words (anchor block_id, path_id, reverse,
 *                      pos0, pos1) (PangraphNode::new(None, ..)); block the anchor's index, member k, reverse the strand of the pair's
 *                      anchor-block node, (pos0, pos1) = (pos0 of the pair's first node in path order, pos1 of its second).
 *                      old_left[] / old_right[]: the ids of the left-block and the right-block node it replaces.
 *   paths, nodes, blocks   the graph behind the round in the input layout (n_paths, n_nodes_out, n_blocks entries): the anchor-block node
 *                      of a pair replaced in place by the new node, the other dropped; the anchor block with cons_len the sum and its
 *                      depth, the other block alive = 0, depth = 0, cons_len = 0.  They are the next call's input by pointer.
 *                      With n_round == 0 the three are NULL: the graph is unchanged.
 * The transitive list comes back to the host, the round is chosen there (sequential by definition, O(transitive edges)), and the pairing
 * and the splice follow on the device.
 * Malformed input fails the call (-1, message in pga_last_error(), no output).  Before anything is launched: alive block ids not strictly
 * ascending, path ids not ascending, a node naming a block out of range or a dead block, member >= depth, n_nodes of the paths not summing
 * to the node count or node_off not the running sum, 2^31 or more nodes, blocks or paths, a merged consensus of 2^32 letters or more, a
 * sched edge that is not transitive or names a block twice, n_sched == 0 with a non-NULL sched.  On the device, before any index derived
 * from it is used: a (block, member) slot named by no node or by two, nodes of a block not summing to its depth; behind the pairing: a slot of
 * a partner list left unwritten.  n_paths == 0 or n_nodes == 0 returns empty lists without a device call. */
#define PGA_TOPO_EDGES_ONLY 1u
#define PGA_TOPO_COUNTS 2u
#define PGA_TOPO_TILE 1024       /* path positions per workgroup of the splice's scan */
typedef struct { uint64_t block_id; uint32_t cons_len, depth; int32_t alive, pad; } pga_topo_block_t;
typedef struct { uint64_t path_id, node_off; uint32_t n_nodes; int32_t circular; } pga_topo_path_t;
typedef struct { uint64_t node_id, pos0, pos1; uint32_t block, member; int32_t reverse, pad; } pga_topo_node_t;
typedef struct { uint32_t b1; int32_t s1; uint32_t b2; int32_t s2; } pga_topo_sched_t;          /* ((block, reverse), (block, reverse)) */
typedef struct { uint32_t b1, b2; int32_t s1, s2; uint32_t count, pad; } pga_topo_edge_t;
typedef struct {
	uint32_t anchor, other; int32_t anchor_rev, other_rev;    /* the oriented edge */
	uint32_t transitive, pad;
	pga_merge_edge_t merge;
	uint64_t partner_off;
} pga_topo_round_t;
typedef struct {
	int64_t n_transitive, n_counts, n_round, n_partner, n_blocks, n_paths, n_nodes;
	pga_topo_edge_t *transitive, *edge_counts;
	pga_topo_round_t *round;
	uint32_t *partner;
	pga_topo_node_t *new_nodes; uint64_t *old_left, *old_right;
	pga_topo_path_t *paths; pga_topo_node_t *nodes; pga_topo_block_t *blocks;
} pga_topo_out_t;
int pga_plan_simplify(int64_t n_blocks, const pga_topo_block_t *blocks, int64_t n_paths, const pga_topo_path_t *paths, int64_t n_nodes,
                      const pga_topo_node_t *nodes, int64_t n_sched, const pga_topo_sched_t *sched, uint32_t flags, pga_topo_out_t *out);
void pga_topo_free(pga_topo_out_t *out);

/* ---- self-merge: detach_unaligned_nodes (packages/pangraph/src/pangraph/detach_unaligned.rs:24-114) ----
 * pga_detach_unaligned takes the members without an aligned position out of their blocks and makes each a singleton block of its own
 * sequence.  The reference runs it on the merged blocks right after solve_promise (graph_merging.rs:154) and on the realigned blocks inside
 * reconsensus_graph (reconsensus/reconsensus.rs:85): pga_solve_promises -> pga_detach_unaligned -> pga_reconsensus -> pga_detach_unaligned
 * is that chain in one data layout.  The node map (same node id, new block id, forward strand, position kept) is pga_close_round's on the
 * flat graph; a caller that keeps dicts (pangraph_amd/detach.py) reads it off orphans[] and member_map[] without a search.
 * Blocks, members and edits in the layout of pga_reconstruct; who[m] belongs to global member m.  Inputs are only read.
 *   unaligned      Edit::aligned_count(cons_len) == 0 (edits.rs:439-442): cons_len.saturating_sub(the SUM of the deletion lengths), added
 *                  in 64 bits -- the plain sum, not the union of the intervals.  The validation admits deletions that overlap (each must
 *                  lie inside the consensus, nothing else is asked), so two deletions over the same half of a consensus make a member
 *                  unaligned although half of the consensus is in its sequence; that is the reference's rule and it is kept.  cons_len == 0
 *                  makes every member of the block unaligned, one without edits included.  Insertions and substitutions play no part.
 *   blocks[b], b < n_blocks (input)   the input block without its unaligned members: the caller's consensus pointer (nothing is copied),
 *                  n_members the number kept.  A block left without a member stays, as in the reference.
 *   members[]      the kept members of block 0, then those of block 1, ... in input order, their three lists packed in that order; a kept
 *                  insertion keeps its seq_off into the caller's ins_seq (the rule of pga_slice_blocks), the call owns no insertion letters:
 *                  the next call takes out->blocks, out->members, out->subs, out->dels, out->inss and the caller's own ins_seq.  Behind the
 *                  kept members one member per singleton block with the counts 0, 0, 0 (PangraphBlock::from_consensus).
 *   blocks[n_blocks (input) + k]   one per unaligned member in the reference's push order (block after block, inside a block in member
 *                  order): the letters are Edit::apply of the member's edits to its block's consensus (edits.rs:307-329, list-order rules
 *                  as in pga_reconstruct), reverse-complemented (io/seq.rs:9-33) when who[m].reverse != 0; consensus points into out->cons
 *                  (every sequence at a multiple of 16), n_members = 1; an empty sequence gives cons_len = 0.
 *   orphans[k]     member: the global input member; block: its index in out->blocks; len: the sequence length; node_id: copied from who;
 *                  block_id: id((node_id, &seq)) of utils/id.rs -- XXH64, seed 0, over node_id as a little-endian u64, the length as a
 *                  little-endian u64, then the letters (the derived Hash of NodeId(usize), Seq { Vec<AsciiChar> }, AsciiChar(u8) and std's
 *                  length prefix of a slice); computed on the host from the downloaded letters.
 *                  status, the first that applies: 0 built; 2 a reverse orphan holds a letter the complement table rejects (the
 *                  reference's Err); 3 a literal '-' came out (Edit::apply would strip it; as pga_reconstruct).  With a non-zero status
 *                  block_id is 0 and the letters are as built and not to be used.  Counts and offsets never depend on a status and other
 *                  orphans are not affected.
 *   member_map[m]  the index in out->members of input member m, kept or detached.
 * When no member is unaligned out->cons and out->orphans are NULL, no letter is built, and the output equals the input.
 * Malformed input fails the call before anything is launched (-1, message in pga_last_error()): what fails pga_reconstruct, a NULL `who`
 * with members present, NULL insertion letters with a non-zero length, a detached member longer than 2^31 letters.  n_blocks == 0 returns
 * empty lists without a device call.  Freed with pga_detach_free. */
typedef struct { uint64_t node_id; int32_t reverse, pad; } pga_detach_member_t;   /* per input member: its NodeId; old node's strand().is_reverse() */
typedef struct { uint64_t member, node_id, block_id; uint32_t block, len; int32_t status, pad; } pga_detach_orphan_t;
typedef struct {
	int64_t n_blocks, n_orphans;               /* n_blocks = input n_blocks + n_orphans */
	pga_rc_block_t  *blocks;
	pga_rc_member_t *members;                  /* as many as the input has */
	pga_sub_t *subs; pga_del_t *dels; pga_ins_t *inss;
	char *cons;                                /* letters of the new singleton blocks only */
	int64_t *member_map;
	pga_detach_orphan_t *orphans;
} pga_detach_out_t;
int pga_detach_unaligned(int64_t n_blocks, const pga_rc_block_t *blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels,
                         const pga_ins_t *inss, const char *ins_seq, const pga_detach_member_t *who, pga_detach_out_t *out);
void pga_detach_free(pga_detach_out_t *out);
/* ---- self-merge: the front half of reweave (packages/pangraph/src/pangraph/reweave.rs:132-340, 408-443 over pangraph_interval.rs:98-255 and
 * align/bam/cigar.rs:26-96) ----
 * pga_plan_merge turns the filtered matches of a tree level into what the next two calls consume: the interval table of pga_slice_blocks and
 * the (anchor, append, orientation, CIGAR) of every MergePromise.  pga_batch_align -> pga_result_filter -> pga_plan_merge -> pga_slice_blocks
 * -> pga_solve_promises -> pga_detach_unaligned -> pga_reconsensus is self_merge (graph_merging.rs:95-172) in one data layout; node ids and
 * the path bookkeeping of graph.update are pga_apply_merge below (pangraph_amd/apply.py; the host loop of pangraph_amd/reweave.py is its restatement).
 * Input: groups as pga_batch_align has them; the blocks of group g are blocks[group_off[g] .. group_off[g + 1]) in any order, block_id
 * unique inside a group, depth = alignments.len().  matches / cigars / n_ops as pga_filter_matches takes them; qry and ref index the blocks of
 * the match's group.  thr_len = indel_len_threshold (graph_merging.rs:142).  batch (may be NULL) with seq_index: blocks[i] is sequence
 * seq_index[i] (hand-over order) of the resident batch, and its "not ACGT" bit plane stands in for the letters where it can.
 * In the reference's order:
 *   ids        aligned: XXH64, seed 0, of the six little-endian u64 words (qry block_id, qry_start, qry_end, ref block_id, ref_start, ref_end)
 *              (reweave.rs:132-140; utils/id.rs over the derived Hash of BlockId(usize) and Interval { start, end }); an unaligned gap: XXH64 of
 *              the three words (block_id, start, end) with the gap as created, before refinement (pangraph_interval.rs:98-132).
 *   anchor     (reweave.rs:144-172) the deeper block; at equal depth the side with fewer bytes equal to 'N' (no other letter, no lower case)
 *              inside its interval, ref on a tie.  route 0: depth decided.  route 1: the bit plane of the batch holds no set bit in either
 *              interval -- it marks every letter outside ACGT, so both counts are 0 and ref wins.  route 2: the letters of both intervals
 *              were uploaded and counted (every equal-depth match when batch == NULL).  anchor, ref_n and qry_n never depend on whether a
 *              batch was given; route and the counters do.  ref_n = qry_n = 0 on route 0.
 *   hits       (extract_hits, reweave.rs:202-248) a ref-side anchor keeps the match's CIGAR; a qry-side anchor gets it reversed when the
 *              match is reverse, then I and D exchanged; the other side has none.
 *   intervals  (create_intervals, pangraph_interval.rs:135-156) the hits of a block by ascending start; a gap before a hit where its start
 *              is beyond the end of the hit before (or 0), a trailing gap where the last hit ends before cons_len.
 *   refinement (pangraph_interval.rs:158-235) every decision reads the lengths of the UNREFINED list: an interval shorter than thr_len joins
 *              its left neighbour iff left_len >= right_len (a missing neighbour has length 0), else its right one; an aligned interval can
 *              receive from both sides.  status of a block, from the first offending interval in list order and there in the order of
 *              check_interval_conditions: 1 the short interval is aligned, 3 its left neighbour is shorter than thr_len, 5 its right
 *              neighbour is.  (The two "neighbour not aligned" errors cannot arise: create_intervals never emits two gaps in a row.  Nor
 *              can 3 come first in a list it made: that left neighbour is aligned, is visited before the gap and fails with 1.)
 *              fail_interval is that interval's index in the block's unrefined list, -1 with status 0.  The reference's reweave fails as a
 *              whole: when any block fails, n_failed > 0, blocks[] carries status and fail_interval (n_intervals and first_interval 0),
 *              intervals, slice_intervals, promises and cigars are NULL and their counts and the counters behind them 0.
 *   promises   (group_promises, reweave.rs:306-340) one per match, group by group, inside a group by ascending new_block_id.  The CIGAR is
 *              update_cigar (reweave.rs:271-304) over add_flanking_indel (cigar.rs:60-96), each step on the result of the one before:
 *              1 anchor extend_left: D leading; 2 anchor extend_right: D trailing; 3 append extend_left: I leading if forward, else trailing;
 *              4 append extend_right: I trailing if forward, else leading.  add_flanking_indel as written: walking from that end up to the
 *              first M / = / X (or through the whole CIGAR when it has none), the LAST operation of the wanted kind met is lengthened;
 *              where there is none a new operation goes to the very end of that side.  At most n_cigar + 4 operations come out.
 * Output (freed with pga_plan_free), all exact integers:
 *   matches[m]       one per input match: new_block_id, anchor (0 ref, 1 qry), route, ref_n, qry_n.
 *   blocks[]         one per block with a hit, group by group and inside a group by ascending block_id (the BTreeMap order of target_blocks,
 *                    reweave.rs:177-193, 427): block = its index in the input, its intervals are intervals[first_interval .. + n_intervals).
 *   intervals[]      block after block, ascending start: match = the input match of an aligned interval, -1 for a gap (is_anchor, reverse 0);
 *                    extend_left / extend_right: 0 means None (a gap is never empty, Some(0) cannot arise).  slice_intervals[] is the same
 *                    list in the layout of pga_slice_interval_t (flip = aligned && !is_anchor && reverse): with blocks[].n_intervals it is
 *                    the intervals argument of pga_slice_blocks, nothing is copied.
 *   promises[]       anchor / append as (block index in the input, index into intervals[]); the CIGAR is cigars[cigar_off .. + n_cigar)
 *                    (minimap2 packing).  A pga_promise_t is pointer arithmetic: consensus + start, end - start.
 *   counters         matches by route, hits (2 per match), intervals before and after refinement, CIGAR operations in and out.
 * Malformed input fails the call (-1, message in pga_last_error()); all but the three marked (device) before anything is launched: a match
 * with qry == ref (self_merge filters those), an index outside its group, an empty hit or one outside its block, a CIGAR range outside the
 * pool, NULL letters with cons_len > 0, two blocks of a group with one block_id, seq_index outside the batch or a length that differs from
 * the batch's; two hits on one block that overlap (device, on the sorted list; filter_matches guarantees they do not), two matches of a
 * group with one new_block_id (device), a CIGAR operation other than M I D = X or an operation length that would reach 2^28 after a flank
 * (device).  Nothing the device reads depends on these being absent.  n_matches == 0 returns empty lists without a device call.
 * The call waits for the device once.  The exception: with a batch, matches whose bit plane is not empty need their letters; they are
 * known after that wait, are counted in a second pass and the lists are built again (a consensus with N, R, Y ... inside aligned intervals). */
typedef struct { uint64_t block_id; const char *consensus; uint32_t cons_len, depth; } pga_plan_block_t;
typedef struct { uint64_t new_block_id; int32_t anchor, route; uint32_t ref_n, qry_n; } pga_plan_match_t;
typedef struct { uint64_t first_interval; int64_t fail_interval; uint32_t block, n_intervals; int32_t status, pad; } pga_plan_block_res_t;
typedef struct {
	uint64_t new_block_id; int64_t match;
	uint32_t start, end;
	int32_t aligned, is_anchor, reverse;
	uint32_t extend_left, extend_right, pad;
} pga_plan_interval_t;
typedef struct {
	uint64_t new_block_id; int64_t match;
	uint64_t anchor_interval, append_interval, cigar_off;
	uint32_t anchor_block, append_block, n_cigar; int32_t reverse;
} pga_plan_promise_t;
typedef struct { uint64_t by_depth, by_mask, by_letters, hits, intervals_before, intervals_after, cigar_in, cigar_out; } pga_plan_counters_t;
typedef struct {
	int64_t n_matches, n_blocks, n_intervals, n_promises, n_failed; uint64_t n_cigar;
	pga_plan_match_t *matches; pga_plan_block_res_t *blocks;
	pga_plan_interval_t *intervals; pga_slice_interval_t *slice_intervals;
	pga_plan_promise_t *promises; uint32_t *cigars;
	pga_plan_counters_t counters;
} pga_plan_out_t;
int pga_plan_merge(int32_t n_groups, const int64_t *group_off, const pga_plan_block_t *blocks, int64_t n_matches, const pga_match_t *matches,
                   const uint32_t *cigars, uint64_t n_ops, uint32_t thr_len, const pga_batch_t *batch, const int64_t *seq_index, pga_plan_out_t *out);
void pga_plan_free(pga_plan_out_t *out);

/* ---- self-merge: the graph update behind the slices (split_block's n_new / b_new, reweave.rs:359-401; Pangraph::update, pangraph.rs:68-107,
 * applied block after block, reweave.rs:445-450; the insertion of the merged blocks, graph_merging.rs:156-165) ----
 * pga_apply_merge replaces, on the flat graph of pga_plan_simplify, every node of a cut block by the nodes of its kept slices, makes those
 * nodes with their ids, and builds the block table behind the round with the member slots of every new block.
 * The graph (the first six arguments) is that of pga_plan_simplify, with its rules.  The cut is what the two calls before produced, as it stands:
 *   cut[n_cut]     one per plan.blocks[k]: block = its index in THIS graph, first_interval / n_intervals the record's own (first_interval is
 *                  the running sum of n_intervals: intervals[] is numbered as slices[] is).
 *   intervals      plan.intervals; read: new_block_id, start, end, aligned, is_anchor.
 *   slices, members   the output of the pga_slice_blocks call whose blocks were given in the order of plan.blocks[]; the member order of that
 *                  call is the block's member order, the `member` slot of the graph's nodes.
 * Output (freed with pga_apply_free), all exact integers:
 *   new_nodes[k]   belongs to slice.members[k]: node_id = XXH64, seed 0, of the five little-endian u64 words (new_block_id, path_id, reverse,
 *                  pos_start, pos_end), reverse and the position the slice member's; block / member: its place in the graph after.
 *                  old_node[k]: the id of the node it replaces.
 *   paths, nodes   a node of a block that is not cut stays (with its slot, its block index translated); a node (block b, member m) of a cut
 *                  block is replaced in place by the new nodes of the kept members with .member == m over b's intervals in interval order,
 *                  in reversed order when the OLD node is reverse; no kept member: the position disappears, a path may become empty.
 *                  path_id and circular unchanged, node_off the new running sum.
 *   blocks[]       the table after, alive blocks only, strictly ascending block_id (unsigned): the surviving alive blocks, one block per
 *                  unaligned interval (cons_len = end - start; depth 0 when its slice kept no member), one per new_block_id of an aligned
 *                  anchor / append pair (cons_len of the anchor interval, depth = kept members of both).  block_map[old index] = new index,
 *                  UINT32_MAX for a cut block and for a dead entry (dead entries are dropped).
 *   new_blocks[]   the blocks the call made, by ascending id: block = index in blocks[]; kind 0 an unaligned slice (interval_a; interval_b 0),
 *                  kind 1 a merged block (interval_a the anchor, interval_b the append).  A node's member in a new block is the rank of its
 *                  node_id among the block's, ascending (the BTreeMap order of alignment_insert); member_src[member_off + s] is the index
 *                  into slice.members[] that fills slot s: the gather list for the block arrays.
 *   (n_blocks, blocks, n_paths, paths, n_nodes, nodes) are the first six arguments of pga_plan_simplify and of the next pga_apply_merge.
 * n_cut == 0 returns zero counts and NULL arrays: the graph is unchanged.
 * Malformed input fails the call (-1, message in pga_last_error(), no output).  Before anything is launched: what pga_plan_simplify refuses
 * about the graph on the host, depths that do not sum to the node count, a cut block out of range, dead or named twice, n_intervals == 0,
 * first_interval not the running sum, intervals of a block not ascending and disjoint (or empty), an aligned interval without its partner
 * of the same new_block_id and the opposite is_anchor, member_off of a slice not the running sum of n_kept or n_kept above the block's
 * depth (n_kept not matching members[]), 2^31 or more nodes, blocks, intervals or members-times-intervals after.  On the device, before any
 * index derived from it is used: a (block, member) slot named by no node or by two, a slice member with member >= depth of its block, a
 * member kept twice in one interval, a new block_id equal to a surviving one or to another new one (the reference panics "Conflicting
 * key"), two equal node ids inside one block after.  The call waits for the device three times: the checks, the splice's total, the output. */
typedef struct { uint32_t block, n_intervals; uint64_t first_interval; } pga_apply_cut_t;
typedef struct { uint32_t block; int32_t kind; uint64_t interval_a, interval_b, member_off; } pga_apply_block_t;
typedef struct {
	int64_t n_new_nodes, n_new_blocks, n_blocks, n_paths, n_nodes;
	pga_topo_node_t *new_nodes; uint64_t *old_node;          /* one per kept slice member, indexed as slice.members[] */
	pga_apply_block_t *new_blocks; uint64_t *member_src;     /* per new block, slot after slot: index into slice.members[] */
	uint32_t *block_map;                                     /* old block index -> new index, UINT32_MAX for a cut block */
	pga_topo_path_t *paths; pga_topo_node_t *nodes; pga_topo_block_t *blocks;   /* the graph after, input layout */
} pga_apply_out_t;
int pga_apply_merge(int64_t n_blocks, const pga_topo_block_t *blocks, int64_t n_paths, const pga_topo_path_t *paths,
                    int64_t n_nodes, const pga_topo_node_t *nodes,
                    int64_t n_cut, const pga_apply_cut_t *cut, const pga_plan_interval_t *intervals,
                    const pga_slice_res_t *slices, const pga_slice_member_t *members, pga_apply_out_t *out);
void pga_apply_free(pga_apply_out_t *out);

/* ---- simplify: the removal of the paths that are not focal (commands/simplify/simplify_run.rs:23-38 over Pangraph::remove_path,
 * pangraph/pangraph.rs:110-132) ----
 * pga_remove_paths is remove_path for every path p with keep[p] == 0, in any order (the result does not depend on it), on the flat graph of
 * pga_plan_simplify AND the block arrays of pga_merge_blocks at once.  Input, only read:
 *   blocks, paths, nodes   the three arrays of pga_plan_simplify, with its rules.
 *   rc_blocks, members, subs, dels, inss, ins_seq   the arrays of pga_reconsensus / pga_merge_blocks / pga_reconstruct in the same block index
 *                      order: rc_blocks[i] is blocks[i], n_members == depth for an alive block and 0 for a dead one.  The member of a node is
 *                      global member first_member[block] + member, first_member the running sum of n_members.
 *   keep[n_paths]      non-zero: the path stays.
 *   flags              PGA_REMOVE_COMPACT_LETTERS, see below.
 * Output (freed with pga_remove_free), all exact integers:
 *   blocks[n_blocks]   block indices do not move.  A block keeps block_id; depth = its kept members; a block left without a member has
 *                      alive = 0, depth = 0, cons_len = 0, as pga_plan_simplify leaves a dead block, and so has a block that was dead.  (An
 *                      alive block given with depth 0 stays as it is; the reference never holds one.)  n_dead_blocks counts alive == 0.
 *   rc_blocks[n_blocks]   consensus and cons_len as given (no consensus letter moves), n_members = the kept members (0 for a dead block).
 *   paths, nodes       the kept paths in input order, node_off the running sum again; their nodes with id, strand, positions and order
 *                      unchanged, block unchanged, member = the node's rank among the kept members of its block.
 *   members, subs, dels, inss   the kept members in input order (so in their relative order inside every block), their three lists copied
 *                      in that order into dense arrays.
 *   member_map[m]      the place in members[] after of input member m, -1 for a removed one.  path_map[p]: the same for paths.
 *   insertion letters  without PGA_REMOVE_COMPACT_LETTERS seq_off stays as given, ins_seq is not read and may be NULL, out->ins_seq is
 *                      NULL and the caller's buffer goes on serving (the arrangement of pga_detach_unaligned).  With it the letters of
 *                      the kept insertions are gathered in output order into out->ins_seq (n_ins_letters of them) and seq_off becomes the
 *                      running sum of len; the seq_off given may be in any order and may overlap.
 *   (n_blocks, blocks, n_paths, paths, n_nodes, nodes) are the first six arguments of pga_plan_simplify and the graph of pga_apply_merge;
 *   (n_blocks, rc_blocks, members, subs, dels, inss, ins_seq -- the caller's or out->ins_seq) the first seven of pga_merge_blocks,
 *   pga_reconstruct and the two exports: pointers only.
 * keep all non-zero gives the input, copied; keep all zero the empty graph: 0 paths, 0 nodes, every block dead.  n_paths == 0 returns
 * without a device call.
 * Malformed input fails the call (-1, message in pga_last_error(), out zeroed).  Before anything is launched: every refusal pga_plan_simplify
 * makes on the host for the three graph arrays (alive block ids not strictly ascending, path ids not ascending, a node naming a block out of
 * range or a dead block, member >= depth, n_nodes of the paths not summing to the node count or node_off not the running sum, 2^31 or more
 * nodes, blocks, paths or members), a NULL array with a non-zero count, NULL keep with n_paths > 0, an unknown flag,
 * rc_blocks[i].n_members != blocks[i].depth or a dead block with members, edit counts that overflow 2^63, members without a single path.
 * On the device, before any index derived from it is used: a (block, member) slot named by no node or by two, nodes of a block not summing
 * to its depth; with PGA_REMOVE_COMPACT_LETTERS, before a letter is read: NULL ins_seq while a kept insertion has letters, seq_off + len >
 * ins_seq_len of a kept insertion.  The path table after is made on the host (O(paths)).  The call waits for the device twice, three times
 * with the flag: the checks and totals, the letter total, the output. */
#define PGA_REMOVE_COMPACT_LETTERS 1u
typedef struct {
	int64_t n_blocks, n_paths, n_nodes, n_members, n_dead_blocks;      /* n_blocks == the input's: block indices do not move */
	uint64_t n_subs, n_dels, n_inss, n_ins_letters;
	pga_topo_block_t *blocks; pga_topo_path_t *paths; pga_topo_node_t *nodes;            /* the graph after, pga_plan_simplify's layout */
	pga_rc_block_t *rc_blocks; pga_rc_member_t *members; pga_sub_t *subs; pga_del_t *dels; pga_ins_t *inss; char *ins_seq;   /* the block arrays after */
	int64_t *member_map;     /* [input members] place in members[] after, or -1 */
	int32_t *path_map;       /* [input paths]   place in paths[] after, or -1 */
} pga_remove_out_t;
int pga_remove_paths(int64_t n_blocks, const pga_topo_block_t *blocks, int64_t n_paths, const pga_topo_path_t *paths, int64_t n_nodes, const pga_topo_node_t *nodes,
                     const pga_rc_block_t *rc_blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss,
                     const char *ins_seq, uint64_t ins_seq_len, const uint8_t *keep /* [n_paths], non-zero: the path stays */, uint32_t flags, pga_remove_out_t *out);
void pga_remove_free(pga_remove_out_t *out);
/* Measurement only: the stream's clock over the last pga_remove_paths call of the calling thread that reached the device, in ms:
 * ms[0] the uploads, ms[1] the kernels with the waits between them, ms[2] the downloads. */
void pga_remove_last_ms(double *ms /* 3 */);

/* ---- self-merge: the block arrays behind a round (solve_promise's tail, reweave.rs:88-93 alignment_insert; the insertion of the merged
 * blocks, graph_merging.rs:156-165; the blocks split_block leaves, reweave.rs:359-401) ----
 * pga_assemble_blocks executes the gather list of pga_apply_merge: it builds the consensus pointers, member counts, three edit lists and
 * insertion letters of every block of the graph that pga_apply_merge returns, from what the calls before it returned, as it stands.  With it
 * pga_plan_merge -> pga_slice_blocks -> pga_apply_merge / pga_solve_promises -> pga_assemble_blocks -> pga_detach_unaligned -> pga_reconsensus
 * (or pga_reconstruct, pga_plan_simplify + pga_merge_blocks, the exports, the next round) is one chain by pointer.  Input, only read:
 *   rc_blocks, members, subs, dels, inss, ins_seq   the block arrays of the graph BEFORE in the arrangement of pga_remove_paths: rc_blocks[i] is
 *                      blocks[i] of the graph given to pga_apply_merge, n_members == depth for an alive block and 0 for a dead one.
 *   cut, intervals     as given to pga_apply_merge.  promises: plan.promises.  slice: the pga_slice_blocks output.
 *   res, p_subs, p_dels, p_inss, p_ins_seq   the pga_solve_promises output of the call whose promise p is plan.promises[p] with the kept members
 *                      of slice promises[p].append_interval, in that order: their results are res[first_res[p] ..), first_res the running sum
 *                      of those n_kept over the promises in order.
 *   applied            the pga_apply_merge output.
 * Everything else is derived: the slice count is the sum of cut[].n_intervals, the slice members and their edit totals come from the last
 * slice and its last member, the totals of the promise results from the last res[] entry.
 * Output (freed with pga_assemble_free), all exact integers.  Default mode: block i is applied->blocks[i], n_members == depth, from one of
 *   a survivor         (block_map[old] == i) the caller's consensus pointer, members and lists, copied in order;
 *   an unaligned slice (new_blocks[].kind == 0) consensus = the cut block's pointer + interval.start, end - start letters (no consensus letter
 *                      is copied, the rule of pga_slice_blocks); the members named by member_src in slot order with their sliced edits
 *                      (slice->subs / dels / inss);
 *   a merged block     (kind == 1) the consensus of the anchor interval; slot s is slice.members[member_src[member_off + s]]: a member of the
 *                      anchor slice (interval_a) brings its sliced edits, one of the append slice (interval_b) those of its res[] entry
 *                      (counts and offsets into p_subs / p_dels / p_inss).
 *   insertion letters  always gathered in output order into out->ins_seq (n_ins_letters of them), seq_off the running sum of len.  Sources:
 *                      the caller's ins_seq (survivors, sliced edits) and p_ins_seq (promise results); a source seq_off may be in any order
 *                      and may overlap.  One buffer, which the next call takes by pointer.
 *   who[m]             node id and strand of member m after, scattered from applied->nodes (who[first_member[block] + member] = (node_id,
 *                      reverse)): the who argument of pga_detach_unaligned, and the member-to-node map pga_reconstruct, pga_export_json and
 *                      pga_remove_paths assume.
 *   origin[m]          >= 0: the global member before (a survivor's); -(1 + k): slice.members[k].
 * PGA_ASSEMBLE_MERGED_ONLY: only the kind == 1 blocks, in new_blocks[] order, with the same members, lists, letters, who and origin: what
 * pga_detach_unaligned -> pga_reconsensus take after a round.
 * (out->n_blocks, blocks, members, subs, dels, inss, ins_seq) are the first seven arguments of pga_detach_unaligned, pga_reconsensus,
 * pga_reconstruct, pga_merge_blocks, pga_remove_paths (rc side) and the exports: pointers only.
 * n_cut == 0 (applied is all zero then): the default mode returns the input copied with compacted letters, who NULL (no node moved, the
 * caller's map stands), origin the identity; merged-only returns empty lists.  n_blocks == 0: no device call.
 * Malformed input fails the call (-1, message in pga_last_error(), out zeroed).  Before anything is launched: a NULL array with a non-zero
 * count, an unknown flag, cut / intervals / slice tables that pga_apply_merge refuses on the host (a cut block out of range or named twice,
 * n_intervals == 0, first_interval not the running sum, intervals not ascending and disjoint, member_off not the running sum of n_kept) or
 * an interval beyond its block's consensus, applied->n_new_nodes, n_blocks, block_map or new_blocks[] inconsistent with the tables (a block
 * after named twice or by nobody, depth != the kept members of its slices, member_off not the running sum), a kind == 1 block whose
 * interval_b is no promise's append_interval, a promise whose anchor_interval / append_interval disagree with new_blocks[], a survivor whose
 * rc_blocks[].n_members != depth after, a block neither cut nor mapped that has members, 2^31 or more members or blocks, edit totals that
 * overflow 2^63.  On the device, before any index derived from it is used: a member_src entry outside its block's two slices or used twice,
 * a res[] entry of a used append member with status != 0 (the reference's solve_promise returns Err and the merge fails; the message names
 * the promise and the member), a source offset + count beyond its list, seq_off + len beyond ins_seq_len / p_ins_seq_len (before a letter
 * is read; a NULL buffer has length 0), a node of applied->nodes naming a slot twice, outside its block or leaving one unfilled.
 * The call waits for the device three times: the checks and list totals, the letter checks and total, the output. */
#define PGA_ASSEMBLE_MERGED_ONLY 1u
#define PGA_ASSEMBLE_TILE 1024   /* positions per workgroup of the scans and of the element copies */
typedef struct {
	int64_t n_blocks, n_members; uint64_t n_subs, n_dels, n_inss, n_ins_letters;
	pga_rc_block_t *blocks; pga_rc_member_t *members; pga_sub_t *subs; pga_del_t *dels; pga_ins_t *inss; char *ins_seq;
	pga_detach_member_t *who;   /* per member after: node id and strand */
	int64_t *origin;            /* per member after: >= 0 the global member before (a survivor); -(1 + k): slice.members[k] */
} pga_assemble_out_t;
int  pga_assemble_blocks(
	int64_t n_blocks, const pga_rc_block_t *rc_blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels,
	const pga_ins_t *inss, const char *ins_seq, uint64_t ins_seq_len,                          /* the graph BEFORE, pga_remove_paths' arrangement */
	int64_t n_cut, const pga_apply_cut_t *cut, const pga_plan_interval_t *intervals,
	int64_t n_promises, const pga_plan_promise_t *promises,                                    /* plan output, as it stands */
	const pga_slice_out_t *slice,                                                              /* pga_slice_blocks output, as it stands */
	const pga_mapvar_res_t *res, const pga_sub_t *p_subs, const pga_del_t *p_dels, const pga_ins_t *p_inss,
	const char *p_ins_seq, uint64_t p_ins_seq_len,                                             /* pga_solve_promises output, as it stands */
	const pga_apply_out_t *applied,                                                            /* pga_apply_merge output, as it stands */
	uint32_t flags, pga_assemble_out_t *out);
void pga_assemble_free(pga_assemble_out_t *out);
/* Measurement only: the stream's clock over the last pga_assemble_blocks call of the calling thread that reached the device, in ms:
 * ms[0] the uploads, ms[1] the kernels with the waits between them, ms[2] the downloads. */
void pga_assemble_last_ms(double *ms /* 3: uploads, kernels with their waits, downloads */);

/* ---- self-merge: the tail of a round on the two flat layouts (self_merge, graph_merging.rs:153-169; reconsensus_graph,
 * reconsensus/reconsensus.rs:46-91; detach_unaligned_nodes, detach_unaligned.rs:24-114) ----
 * pga_close_round folds what pga_detach_unaligned -> pga_reconsensus -> pga_detach_unaligned returned for the merged blocks back into the
 * flat graph of pga_plan_simplify AND the block arrays of pga_remove_paths: unaligned members leave their blocks and become singleton blocks,
 * their nodes keep id, path and position and get the new block and the forward strand, every merged block gets its consensus and its member
 * edits after the reconsensus.  Its output is the input of the next round.  Input, only read, taken as it stands:
 *   blocks, paths, nodes   the graph of pga_apply_merge's output, with the rules of pga_plan_simplify.
 *   rc_blocks, members, subs, dels, inss, ins_seq, who   the default output of pga_assemble_blocks: rc_blocks[i] is blocks[i], n_members == depth
 *                      (0 for a dead entry); who[m] belongs to global member m = first_member[block] + member.
 *   upd[n_upd]         the graph index of the j-th updated block: applied.new_blocks[].block of the kind-1 entries in new_blocks[] order, the
 *                      block order of PGA_ASSEMBLE_MERGED_ONLY.  Slot s of that output's block j is slot s of graph block upd[j]: merged
 *                      member m (block j, slot s) is global member first_member[upd[j]] + s.  The call relies on this.
 *   detached           pga_detach_unaligned on the merged-only arrays (n_upd input blocks); read: blocks, member_map, orphans and the
 *                      letters of the singleton blocks.
 *   rc                 pga_reconsensus on detached's arrays, over the first n_upd blocks or all of them; read: blocks[j] for j < n_upd, the
 *                      status of members[m1] for the members the first detach kept, cons, ins_seq.  rc_ins_seq_len: the sum of the
 *                      n_ins_bases of those members (as p_ins_seq_len is for pga_assemble_blocks).
 *   redetached         the second pga_detach_unaligned, on the arguments pga_rc_detach_args builds from rc (its subs, dels, inss and ins_seq
 *                      are rc's own arrays by pointer: they are already dense in member order), over all n_upd blocks (the
 *                      reference runs it on the kind-2 blocks only; a kind-0 or kind-1 block keeps cons_len and every deletion and the
 *                      first detach has taken its unaligned members, so the result is the same, and an orphan of redetached in a block
 *                      whose kind is not 2 fails the call); read: blocks, members, subs, dels, inss, member_map, orphans, the letters.
 * The member chain: detached->member_map[m] is an orphan or member m1 of the second stage, redetached->member_map[m1] an orphan or a final
 * member; a final member's slot is its rank among the members of block j that redetached kept (relative order, so node-id order, is kept).
 * Output (freed with pga_close_free), all exact integers:
 *   blocks[]           alive blocks only, strictly ascending unsigned block_id, dead entries dropped (as pga_apply_merge drops them), the
 *                      singleton blocks merged in by id.  An updated block keeps its id; cons_len = rc->blocks[j].cons_len, depth = the
 *                      members redetached kept (a block left without a member stays alive with depth 0, as in the reference).  A singleton:
 *                      block_id and len of the orphan record, depth 1.  block_map[input index] = index after, UINT32_MAX for a dead entry.
 *   paths[]            copied.  nodes[]: same count and order; a node of a block that is not updated keeps its slot (block translated by
 *                      block_map), a final member's node gets its slot, an orphan's node block = the singleton's index, member = 0,
 *                      reverse = 0; node_id, pos0 and pos1 never change.
 *   rc_blocks, members, subs, dels, inss   rc_blocks[i] is blocks[i] after; members block after block, the three lists dense in that order.
 *                      Survivors are copied from the arrays given, an updated block's members and lists come from redetached, a singleton
 *                      has one member with the counts 0, 0, 0.
 *   ins_seq            always gathered in output order (n_ins_letters), seq_off the running sum of len.  Sources: the caller's ins_seq and
 *                      rc->ins_seq (redetached's insertions point into it); a source seq_off may be in any order and may overlap.
 *   cons               the consensus letters this call owns, every sequence at a multiple of 16 (n_cons_letters: the bytes used, padding
 *                      included), in block order after: the updated blocks of kind 1 and 2 (from rc->cons) and the singletons (from
 *                      detached->cons / redetached->cons).  A kind-0 block and every other block keep the pointer they had.
 *                      PGA_CLOSE_COPY_CONSENSUS: every alive block's letters are copied there (a host copy on the library's thread ranges);
 *                      afterwards only `out` must live on.  Without it the caller's consensus buffers go on serving.
 *   who[m], origin[m]  every member after is exactly one member before: origin[m] its global member in the arrays given, who[m] that
 *                      member's entry, with reverse = 0 for an orphan.
 *   kinds[j]           rc->blocks[j].kind.  orphans[]: the records of detached, then of redetached, with member = the global member in the
 *                      arrays given and block = the singleton's index after.
 *   (n_blocks, blocks, n_paths, paths, n_nodes, nodes) are the first six arguments of the next pga_apply_merge, of pga_plan_simplify,
 *   pga_remove_paths and the exports; (n_blocks, rc_blocks, members, subs, dels, inss, ins_seq) with n_ins_letters the first arguments of the
 *   next pga_assemble_blocks, of pga_reconstruct, pga_merge_blocks, pga_remove_paths and pga_export_json; who is the member-to-node map those
 *   entries assume: pointers only.
 * n_upd == 0 (detached, rc, redetached may be NULL) returns the input copied, with compacted letters, dead entries dropped and the identity
 * maps.  n_blocks == 0: no device call.
 * Malformed input fails the call (-1, message in pga_last_error(), out zeroed).  Before anything is launched: what pga_plan_simplify refuses
 * about the graph on the host, rc_blocks[i].n_members != depth or rc_blocks[i].cons_len != blocks[i].cons_len of an alive block, a kind-0 block
 * whose rc cons_len is not the one it had, an orphan record k of a stage whose block is not n_upd + k or whose len is not that block's
 * cons_len (the letters of orphan k are read there), a NULL array with a non-zero count, an unknown flag, upd[j] out of range,
 * dead or named twice, detached->n_blocks != n_upd + detached->n_orphans (the same for redetached), kept members plus orphans of a stage
 * not summing to the members it was given, rc->blocks[j].kind < 0 (the reference's Err; the message names the block and the kind), a
 * rc->members[] entry of a read member with status != 0 (edit_consensus_and_realign returns Err; the message names block and member), an
 * orphan record with status != 0 (create_new_node_and_block's Err), 2^31 or more blocks, members or nodes after, edit totals that overflow
 * 2^63.  On the device, before any index derived from it is used: kept members plus orphans of block j not equal to its depth, in either
 * stage; a member_map that is no bijection onto the stage's places or does not keep the order; an orphan of the second stage in a block
 * whose kind is not 2; a singleton block_id equal to a surviving block's or another singleton's (the reference panics "Conflicting key" on
 * the first route and would overwrite on the second; both are refused); a graph slot named by no node or by two; seq_off + len beyond
 * ins_seq_len / rc_ins_seq_len (before a letter is read; a NULL buffer has length 0).
 * The call waits for the device three times: the checks and list totals, the letter checks and total, the output. */
#define PGA_CLOSE_COPY_CONSENSUS 1u
typedef struct {
	int64_t n_blocks, n_paths, n_nodes, n_members, n_orphans;
	uint64_t n_subs, n_dels, n_inss, n_ins_letters, n_cons_letters;
	pga_topo_block_t *blocks; pga_topo_path_t *paths; pga_topo_node_t *nodes;      /* the graph after, pga_plan_simplify's layout */
	pga_rc_block_t *rc_blocks; pga_rc_member_t *members; pga_sub_t *subs; pga_del_t *dels; pga_ins_t *inss; char *ins_seq;
	char *cons;                      /* consensus letters this call owns, every sequence at a multiple of 16 */
	pga_detach_member_t *who;        /* per member after: node id, strand */
	int64_t *origin;                 /* per member after: its global member in the block arrays given */
	uint32_t *block_map;             /* [input blocks] index after, UINT32_MAX for a dead entry */
	int32_t *kinds;                  /* [n_upd] the reconsensus kind of every updated block */
	pga_detach_orphan_t *orphans;    /* [n_orphans] first detach's, then second's; member = global member of the arrays given, block = index after */
} pga_close_out_t;
int  pga_close_round(int64_t n_blocks, const pga_topo_block_t *blocks, int64_t n_paths, const pga_topo_path_t *paths, int64_t n_nodes, const pga_topo_node_t *nodes,
                     const pga_rc_block_t *rc_blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss,
                     const char *ins_seq, uint64_t ins_seq_len, const pga_detach_member_t *who,
                     int64_t n_upd, const uint32_t *upd,
                     const pga_detach_out_t *detached, const pga_rc_out_t *rc, uint64_t rc_ins_seq_len, const pga_detach_out_t *redetached,
                     uint32_t flags, pga_close_out_t *out);
void pga_close_free(pga_close_out_t *out);
/* Measurement only: the stream's clock over the last pga_close_round call of the calling thread that reached the device, in ms. */
void pga_close_last_ms(double *ms /* 3: uploads, kernels with their waits, downloads */);
/* pga_rc_detach_args (host only) fills the first arguments of the SECOND pga_detach_unaligned call from a pga_rc_out_t:
 * blocks[j] = {rc->cons + cons_off, cons_len, detached->blocks[j].n_members} for j < n_upd, members[m1] = the three counts of rc->members[m1]
 * for the members the first detach kept, who2[detached->member_map[m]] = who_merged[m] for every kept m.  rc->subs, dels, inss and ins_seq
 * are already dense in member order (pga_reconsensus.hip, the pack loop) and go into that call by pointer, as they stand.
 * Returns 0, or -1 with the message in pga_last_error(). */
int pga_rc_detach_args(int64_t n_upd, const pga_detach_out_t *detached, const pga_detach_member_t *who_merged, const pga_rc_out_t *rc,
                       pga_rc_block_t *blocks /* [n_upd] */, pga_rc_member_t *members /* [kept members] */, pga_detach_member_t *who2);

/* ---- graph_join on the two flat layouts (graph_merging.rs:74-93: the first line of merge_graphs at every internal node of the guide tree) ----
 * pga_join_graphs puts n_parts graphs into one: the union of their blocks, paths and nodes in the order the reference's BTreeMaps give, a
 * "Conflicting key" refusal on a shared block, path or node id.  A part is one graph in both layouts, exactly as pga_close_out_t hands it on,
 * and is only read:
 *   n_blocks, blocks, n_paths, paths, n_nodes, nodes   the graph in pga_plan_simplify's layout and under its rules; dead entries are allowed.
 *   rc_blocks, members, subs, dels, inss, ins_seq, ins_seq_len, who   the block arrays: rc_blocks[i] is blocks[i], n_members == depth (0 for a
 *                      dead entry), the three lists dense in member order, who[m] belongs to global member m.
 * Output (freed with pga_join_free), all exact integers:
 *   blocks[]           the alive blocks of all parts in strictly ascending unsigned block_id, dead entries dropped.  block_map[] runs over the
 *                      input blocks of all parts behind each other (part p's at block_map_off[p], block_map_off[n_parts] entries in all):
 *                      the index after, UINT32_MAX for a dead entry.
 *   paths[]            ascending path_id, node_off the running sum; path_map[] / path_map_off[] in the same way.
 *   nodes[]            path after path in that order, each path's nodes in their own order; block is translated by block_map, member,
 *                      reverse, node_id, pos0 and pos1 are unchanged.
 *   rc_blocks, members, subs, dels, inss   rc_blocks[i] is blocks[i] after; members block after block, inside a block the slots as they were
 *                      (a block belongs to one part); the three lists dense in that order.
 *   ins_seq            always gathered in output order (n_ins_letters), seq_off the running sum of len; a source seq_off may be in any order
 *                      and may overlap.
 *   cons               by default empty: every consensus pointer is the part's own, so the parts' letters go on serving.
 *                      PGA_JOIN_COPY_CONSENSUS: every block's letters are copied there, every sequence at a multiple of 16 (a host copy on
 *                      the library's thread ranges); afterwards only `out` must live on.  No consensus letter goes to the device.
 *   who[m], origin_part[m], origin[m]   member m after is global member origin[m] of part origin_part[m]; who[m] is that member's entry.
 *   (n_blocks, blocks, n_paths, paths, n_nodes, nodes) and (n_blocks, rc_blocks, members, subs, dels, inss, ins_seq) with n_ins_letters and
 *   who are, by pointer, the first arguments of pga_apply_merge, pga_assemble_blocks, pga_plan_simplify, pga_remove_paths, pga_reconstruct,
 *   the exports -- and a part of the next pga_join_graphs.
 * n_parts == 1 gives the compacted copy with the identity origin.  A part with n_blocks == 0 is legal; when no part has a block or a path
 * there is no device call.
 * Malformed input fails the call (-1, message in pga_last_error(), out zeroed); every message names the part.  Before anything is launched,
 * per part: what pga_plan_simplify refuses about the graph on the host (ids not ascending, a node naming a dead or out-of-range block,
 * member >= depth, node_off not the running sum), rc_blocks[i].n_members != depth or a cons_len mismatch of an alive block, a NULL array with
 * a non-zero count; an unknown flag, n_parts < 1, 2^31 or more blocks, members, nodes or paths, edit totals that overflow 2^63.  On the
 * device, before any index derived from it is used: a block id, a path id or a node id present twice, across parts or within one (the
 * reference's "Conflicting key" panic; the message names the kind, the smallest such id and the parts); a (block, member) slot of a part
 * named by no node or by two; seq_off + len of an insertion beyond its own part's ins_seq_len (a NULL buffer has length 0), so an insertion
 * of one part never reads another part's letters.
 * The call waits for the device three times: the checks and list totals, the letter checks and total, the output. */
#define PGA_JOIN_COPY_CONSENSUS 1u
typedef struct {
	int64_t n_blocks; const pga_topo_block_t *blocks; int64_t n_paths; const pga_topo_path_t *paths; int64_t n_nodes; const pga_topo_node_t *nodes;
	const pga_rc_block_t *rc_blocks; const pga_rc_member_t *members; const pga_sub_t *subs; const pga_del_t *dels; const pga_ins_t *inss;
	const char *ins_seq; uint64_t ins_seq_len; const pga_detach_member_t *who;
} pga_join_part_t;
typedef struct {
	int64_t n_blocks, n_paths, n_nodes, n_members, n_parts;
	uint64_t n_subs, n_dels, n_inss, n_ins_letters, n_cons_letters;
	pga_topo_block_t *blocks; pga_topo_path_t *paths; pga_topo_node_t *nodes;      /* the graph after, pga_plan_simplify's layout */
	pga_rc_block_t *rc_blocks; pga_rc_member_t *members; pga_sub_t *subs; pga_del_t *dels; pga_ins_t *inss; char *ins_seq;
	char *cons;                      /* PGA_JOIN_COPY_CONSENSUS: every block's letters, every sequence at a multiple of 16 */
	pga_detach_member_t *who;        /* per member after: node id, strand */
	int32_t *origin_part;            /* per member after: the part it came from */
	int64_t *origin;                 /* per member after: its global member in that part's block arrays */
	uint32_t *block_map;             /* [block_map_off[n_parts]] index after, UINT32_MAX for a dead entry */
	uint64_t *block_map_off;         /* [n_parts + 1] */
	uint32_t *path_map;              /* [path_map_off[n_parts]] index after */
	uint64_t *path_map_off;          /* [n_parts + 1] */
} pga_join_out_t;
int  pga_join_graphs(int32_t n_parts, const pga_join_part_t *parts, uint32_t flags, pga_join_out_t *out);
void pga_join_free(pga_join_out_t *out);
/* Measurement only: the stream's clock over the last pga_join_graphs call of the calling thread that reached the device, in ms. */
void pga_join_last_ms(double *ms /* 3: uploads, kernels with their waits, downloads */);

/* ---- export gfa (io/gfa.rs:79-279 gfa_write / convert_pangraph_to_gfa, Edge of circularize/circularize_utils.rs:46-102) ----
 * pga_export_gfa writes, for the flat graph of pga_plan_simplify (blocks, paths, nodes: its rules, only read) and GfaWriteParams, the bytes
 * gfa_write_str gives, and returns the tables behind them.  By the reference:
 *   segments   (gfa.rs:264-279 graph_to_gfa_segment) one candidate per alive block: length = cons_len, depth = blocks[].depth, duplicated =
 *              two of its nodes lie on one path (PangraphBlock::is_duplicated), on the unfiltered graph.
 *   filter     (gfa.rs:239-262 gfa_filter_path) a node stays when its block has min_len <= length <= max_len and min_depth <= depth <=
 *              max_depth, bounds inclusive (absent bounds: 0 and UINT64_MAX), and with no_duplicated is not duplicated.
 *   paths      (gfa.rs:176-183, :218-237) in input order (ascending path_id), `circular` kept as it was; a path with no node left is
 *              dropped, one that was empty before too.
 *   emitted segments   (gfa.rs:185-190) the blocks some kept node names, in ascending block index (ascending id).
 *   links      (gfa.rs:201-216 gfa_paths_to_links) on the FILTERED paths: every two consecutive kept nodes, and the last followed by the
 *              first on a circular path (one kept node: the self link (n, n); a linear path has no wrap link).  An edge equals its
 *              inversion ((b2, !s2), (b1, !s1)) (circularize_utils.rs:51-56, :82-86); it is emitted in conventional_orientation
 *              (circularize_utils.rs:65-71: as it stands when b1 < b2, or b1 == b2 and s1 forward, else inverted), sorted by (b1, b2, s1,
 *              s2) with forward = 0 (gfa.rs:108-114), one record per distinct edge with its count: the keys of pga_plan_simplify.
 *   text       (gfa.rs:79-137), exactly:  "H\tVN:Z:1.0\n";  if any segment "# blocks\n" and per segment
 *              "S\t{id}\t{consensus or *}\tRC:i:{depth*length}\tLN:i:{length}" ["\tTP:Z:duplicated"] "\n";  if any link "# edges\n" and per
 *              link "L\t{id1}\t{+|-}\t{id2}\t{+|-}\t*\tRC:i:{count}\n";  if any path "# paths\n" and per path
 *              "P\t{name}\t{id}{+|-},{id}{+|-}...\t*" ["\tTP:Z:circular"] "\n".  Ids are block_id in decimal (u64, up to 20 digits), RC of
 *              a segment is the 64-bit product.
 * Input besides the graph:
 *   cons[n_blocks]     per block cons_len letters; read only with include_sequences, and only for emitted blocks.
 *   names, name_len    per input path its name as raw bytes (no NUL needed); read only for emitted paths.
 *   p                  the parameters; flags: PGA_GFA_STEPS also returns steps[].
 * Output (freed with pga_gfa_free): segments[] (block: index into blocks; byte_off: of its S line in the file), links[] (block indices),
 * paths[] (path: index into the input paths; its steps are steps[step_off .. step_off + n_steps); byte_off: of its P line), steps[] (with
 * PGA_GFA_STEPS: the kept nodes path after path, 8 bytes each; otherwise NULL), n_steps (always), n_bytes: the length of the file.
 * sink == NULL is verdict mode: the tables and n_bytes, no text byte is produced.  sink != NULL: called on the calling thread with
 * consecutive pieces of the file in file order, each at most PGA_EXPORT_TILE_KB KB (default 16384; a multiple of 4, read at every call);
 * their concatenation is the file, n_bytes long.  A sink that returns non-zero stops the export: what is in flight is drained, no further
 * call is made and the entry returns -1 ("sink stopped the export").  The whole text is never held on the device or the host: the library
 * keeps the tables, one or two tiles and its cached pinned blocks.  Consensus letters and path names never go to the device: the kernel
 * leaves their byte ranges of a tile unwritten and the host copies them from the caller's buffers into the pinned tile (piecewise where
 * one is longer than a tile), O(segments + paths) per call plus the bytes copied.
 * Malformed input fails the call (-1, message in pga_last_error(), out zeroed).  Before anything is launched: every refusal
 * pga_plan_simplify makes on the host for the three arrays, p == NULL, min > max in either pair, an unknown flag, include_sequences with
 * cons == NULL.  On the device, before any index derived from it is used: a (block, member) slot named by no node or by two, nodes of a
 * block not summing to its depth.  Behind the first wait, before a text byte is made: a NULL consensus of an emitted block of non-zero
 * length (include_sequences), names == NULL or a NULL name with a non-zero length for an emitted path, a file of 2^63 bytes or more (held
 * against an upper bound that exceeds the true length by less than 2^41).  n_paths == 0 or n_nodes == 0 gives the header line only,
 * without a device call. */
typedef struct { uint64_t min_len, max_len, min_depth, max_depth; int32_t no_duplicated, include_sequences; } pga_gfa_params_t;
typedef struct { uint32_t block, depth, cons_len; int32_t duplicated; uint64_t byte_off; } pga_gfa_segment_t;  /* byte_off: of its S line in the file */
typedef struct { uint32_t path, n_steps; uint64_t step_off, byte_off; } pga_gfa_path_t;                         /* path: index into the input paths */
typedef struct { uint32_t block; int32_t reverse; } pga_gfa_step_t;
typedef struct { int64_t n_segments, n_links, n_paths, n_steps; uint64_t n_bytes;
                 pga_gfa_segment_t *segments; pga_topo_edge_t *links; pga_gfa_path_t *paths; pga_gfa_step_t *steps; } pga_gfa_out_t;
typedef int (*pga_gfa_sink_t)(void *ctx, const char *bytes, int64_t n);
#define PGA_GFA_STEPS 1u      /* also return steps[] (8 bytes per kept node); otherwise NULL */
int  pga_export_gfa(int64_t n_blocks, const pga_topo_block_t *blocks, int64_t n_paths, const pga_topo_path_t *paths, int64_t n_nodes, const pga_topo_node_t *nodes,
                    const char *const *cons /* per block, cons_len letters; read only with include_sequences */,
                    const char *const *names, const uint32_t *name_len /* per path, raw bytes, no NUL needed */,
                    const pga_gfa_params_t *p, uint32_t flags, pga_gfa_out_t *out, pga_gfa_sink_t sink, void *ctx);
void pga_gfa_free(pga_gfa_out_t *out);
/* Measurement only: the last pga_export_gfa call of the calling thread that reached the device, in ms: ms[0] the stream's clock from the
 * first upload to the tables (the table kernels and their waits), ms[1] the union of the tile kernels on the stream's clock, ms[2] the
 * host's copies of consensus letters and names into the tiles (host clock), ms[3] the time spent inside the sink (host clock). */
void pga_gfa_last_ms(double *ms /* 4 */);

/* ---- the pangraph JSON (serde_json::to_writer_pretty of Pangraph: build_run.rs:78 and simplify_run.rs:20 write it with JsonPretty(true)) ----
 * pga_export_json writes, for the flat graph of pga_plan_simplify (blocks, paths, nodes: its rules, only read) and the block arrays of
 * pga_reconsensus, the bytes of the reference's graph file, and returns where its parts start.  The text, exactly:
 *   layout     two-space indent, ": " behind a key, every entry of a non-empty map or list on a line of its own, an empty list "[]", an empty
 *              map "{}", no trailing newline.  The top level holds "paths", "blocks", "nodes" in that order; map keys are the ids as decimal
 *              strings.  Fields: path id, nodes, tot_len, circular, name, desc; block id, consensus, alignments; alignment subs, dels, inss;
 *              Sub pos, alt; Del pos, len; Ins pos, seq; node id, block_id, path_id, strand ("+" / "-"), position [pos0, pos1].
 *   orders     the reference's BTreeMaps: paths by ascending path_id (input order), alive blocks by ascending block_id (index order), the
 *              "nodes" map by ascending node_id, the alignments of a block by ascending node_id of the node that names the slot, whatever
 *              order the slots are in.  Both come from a device sort of the node ids, by id and then stably by block.  The edits of a
 *              member stay in input order, the nodes of a path in path order.
 * Input besides the graph:
 *   cons[n_blocks]     per block cons_len letters, copied verbatim: the caller's contract, as in pga_export_gfa, is that they need no
 *                      escaping (no '"', no '\', no byte below 0x20).  Read for alive blocks only.
 *   members, subs, dels, inss, ins_seq   one pga_rc_member_t per slot, block after block (blocks[b].depth entries in member order, dead
 *                      blocks none), the three lists member after member; ins_seq_len: the letters at ins_seq.  seq_off may be in any order
 *                      and insertions may share letters.  alt and every insertion letter must be printable ASCII other than '"' and '\'.
 *   tot_len, names, name_len, descs, desc_len   per path; names[i] == NULL / descs[i] == NULL is JSON null, otherwise raw bytes (no NUL
 *                      needed) that are escaped by serde's rules: \" \\ \b \f \n \r \t, other bytes below 0x20 as \u00xx with lower-case
 *                      hex, everything else verbatim (0x7f and bytes >= 0x80 too).
 *   flags              none defined: must be 0.
 * Output (freed with pga_json_free): n_bytes the length of the file; section_off[3] the offsets of the opening quotes of "paths", "blocks"
 * and "nodes"; path_off[n_paths] / block_off[n_blocks] the offset of the opening quote of every path's / block's key (UINT64_MAX for a
 * dead block); node_order[n_nodes] the positions in ascending node_id, the order of the "nodes" map.
 * sink == NULL is verdict mode: the tables and n_bytes, no text byte is produced.  sink != NULL: as pga_export_gfa, consecutive pieces of
 * at most PGA_EXPORT_TILE_KB KB on the calling thread; a sink that returns non-zero stops the export (-1, "sink stopped the export").  The
 * whole text is never held on the device or the host.  The device writes all structure, all numbers, alt and the insertion letters (ins_seq
 * is uploaded once); consensus letters, names and descriptions never go to the device: the kernel leaves their byte ranges unwritten and
 * the host copies them (names and descriptions escaped) into the pinned tile, O(blocks + paths) per call plus the bytes copied.
 * Malformed input fails the call (-1, message in pga_last_error(), out zeroed).  Before anything is launched: every refusal
 * pga_plan_simplify makes on the host for the three arrays, an unknown flag, NULL members with a slot, a NULL edit list with a non-zero
 * count, NULL ins_seq with a non-zero ins_seq_len, NULL tot_len, names, name_len, descs or desc_len with n_paths > 0, a NULL consensus of an alive block
 * of non-zero length.  On the device, before any index derived from it is used: a (block, member) slot named by no node or by two, nodes
 * of a block not summing to its depth, two nodes with one node_id, an alt or an insertion letter outside 0x20..0x7e or equal to '"' or
 * '\', an insertion whose seq_off + len runs past ins_seq_len.  A file of 2^63 bytes or more is refused (held against an upper bound that
 * exceeds the true length by less than 2^9 bytes per path, block, node and edit).  n_blocks == n_paths == n_nodes == 0 gives the three
 * empty maps without a device call. */
typedef struct { uint64_t n_bytes, section_off[3]; int64_t n_paths, n_blocks, n_nodes; uint64_t *path_off, *block_off; uint32_t *node_order; } pga_json_out_t;
int  pga_export_json(int64_t n_blocks, const pga_topo_block_t *blocks, int64_t n_paths, const pga_topo_path_t *paths, int64_t n_nodes, const pga_topo_node_t *nodes,
                     const char *const *cons /* per block, cons_len letters that need no escaping */,
                     const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss, const char *ins_seq, uint64_t ins_seq_len,
                     const uint64_t *tot_len, const char *const *names, const uint32_t *name_len, const char *const *descs, const uint32_t *desc_len /* per path; NULL: null */,
                     uint32_t flags, pga_json_out_t *out, pga_gfa_sink_t sink, void *ctx);
void pga_json_free(pga_json_out_t *out);
/* Measurement only, as pga_gfa_last_ms: ms[0] from the first upload to the layout, ms[1] the union of the tile kernels, ms[2] the host's
 * copies of consensus letters, names and descriptions into the tiles, ms[3] the time spent inside the sink. */
void pga_json_last_ms(double *ms /* 4 */);
int pga_stats_version(void);   /* == PGA_STATS_VERSION of the header the library was built with */
/* Measurement only (no reference interface behind it): the kern_ms sums of pga_stats_t count overlapping launches on different streams
 * and batches several times.  Between pga_busy_begin() and pga_busy_end() every event-bracketed launch of the process leaves its interval
 * on the device clock; pga_busy_end writes, for each of the PGA_N_KERNELS kernel families of pga_stats_t (same order), the length in ms of
 * the UNION of its intervals, and in busy_ms[PGA_N_KERNELS] the union over all families (n >= PGA_N_KERNELS + 1).  Returns the number of
 * intervals seen, -1 on error.  Families that pga_stats_t does not count follow the union where n has room for them: busy_ms[PGA_N_KERNELS + 1 + j]
 * is family PGA_N_KERNELS + j, j < PGA_N_BUSY_EXTRA (family 16: k_rows<false> of the exports). */
#define PGA_N_KERNELS 16
#define PGA_N_BUSY_EXTRA 1
int pga_busy_begin(void);
int pga_busy_end(double *busy_ms, int32_t n);
#ifdef __cplusplus
}
#endif
#endif
