/* ref_map_shim.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The reference keeps collect_seed_hits and skip_seed static in map.c.  This file includes that translation unit as
 * it stands and exports one wrapper, so that the tests can call the reference's own anchor generation on explicit
 * query minimizers against an index built by ref_index_shim.c.  Nothing of the reference is restated here.
 * It is linked in place of map.o into oracle/_ref/libmm2ref_seed.so (oracle/Makefile).
 */
#include "map.c"

/* collect_seed_hits of one query: its minimizers mv[0 .. n_mv) as mm_map_frag hands them over (after mm_seed_mz_flt;
 * y = pos << 1 | strand, the segment id in the upper half is 0), against mi with max_occ = opt->mid_occ.
 * Returns the number of anchors; the first cap of them, sorted by radix_sort_128x, are copied to out. */
int64_t pgref_collect_seed_hits(const mm_mapopt_t *opt, int max_occ, const mm_idx_t *mi, const char *qname, int n_mv, mm128_t *mv, int qlen,
                                int *rep_len, mm128_t *out, int64_t cap)
{
	mm128_v v;
	int64_t n_a = 0;
	int n_mini_pos = 0;
	uint64_t *mini_pos = 0;
	mm128_t *a;
	v.n = v.m = (size_t)n_mv, v.a = mv;
	a = collect_seed_hits(0, opt, max_occ, mi, qname, &v, qlen, &n_a, rep_len, &n_mini_pos, &mini_pos);
	if (n_a > 0 && out) memcpy(out, a, (size_t)(n_a < cap ? n_a : cap) * sizeof(mm128_t));
	kfree(0, a); kfree(0, mini_pos);
	return n_a;
}
