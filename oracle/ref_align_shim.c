/* ref_align_shim.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The reference keeps mm_update_extra, mm_fix_cigar, mm_test_zdrop, mm_fix_bad_ends, mm_filter_bad_seeds,
 * mm_filter_bad_seeds_alt and mm_align1 static in align.c.  This file includes that translation unit as it
 * stands and exports wrappers, so that the tests can call the reference's own code on explicit sequences,
 * operation lists and anchor arrays.  Nothing of the reference is restated here.
 *
 * The file is compiled twice (oracle/Makefile).  libmm2ref_align.so is the plain build: the reference's
 * align.c with its own DP and the two post-DP wrappers.  libmm2ref_plan.so is the build with
 * -DPGREF_PLAN_TRACE, for the region planner's tests, and IN THAT LIBRARY THE DP IS REPLACED: before the
 * include, the two extension entry points that align.c calls (ksw_extd2_sse, ksw_extz2_sse) are renamed
 * to logging stand-ins defined below.
 *
 * Everything mm_align1 decides before and between its DP calls -- the end trimming, the seed filters, the extension
 * windows, the greedy cut into gap-fill segments -- is inline in that function; the only way to read those
 * decisions off the reference's own code is the list of DP calls it makes.  A stand-in records
 * (strand, query offset, qlen, tlen, w, zdrop, end_bonus, flag), resets ez and returns without aligning
 * and without a z-drop, so mm_align1 walks the whole chain.  An extension (KSW_EZ_EXTZ_ONLY) gets no
 * operation list.  A gap-fill call gets a BOOKKEEPING list -- min(qlen, tlen) M and the rest as one gap --
 * because mm_align1 adds to r->p->dp_score after every segment (r->p exists only once a list was appended)
 * and mm_update_extra asserts that the lists span the region; the list is no alignment and nothing reads
 * it.  libmm2ref_plan.so must therefore never be used to ALIGN; libmm2ref.so is the library for that.
 */
#ifdef PGREF_PLAN_TRACE
#define ksw_extd2_sse pgref_log_extd2
#define ksw_extz2_sse pgref_log_extz2
#endif
#include "align.c"

/* mm_update_extra (with mm_fix_cigar inside) of a forward-strand region that spans the whole of both
 * sequences; the list is edited in place.  out = n_cigar, qs, rs, blen, mlen, n_ambi, dp_max. */
int pgref_update_extra(int qspan, const uint8_t *qseq, int tspan, const uint8_t *tseq, uint32_t n_cigar, uint32_t *cigar_inout,
                       const int8_t *mat, int q, int e, int32_t out[7])
{
	mm_reg1_t r;
	mm_extra_t *p = (mm_extra_t*)calloc(sizeof(mm_extra_t) / 4 + n_cigar + 1, 4);
	memset(&r, 0, sizeof(r));
	r.qs = r.rs = 0, r.qe = qspan, r.re = tspan, r.rev = 0;
	p->capacity = (uint32_t)(sizeof(mm_extra_t) / 4) + n_cigar + 1;
	p->n_cigar = n_cigar;
	memcpy(p->cigar, cigar_inout, (size_t)n_cigar * 4);
	r.p = p;
	mm_update_extra(&r, qseq, tseq, mat, (int8_t)q, (int8_t)e, 0, 1);
	p = r.p;
	memcpy(cigar_inout, p->cigar, (size_t)p->n_cigar * 4);
	out[0] = (int32_t)p->n_cigar, out[1] = r.qs, out[2] = r.rs, out[3] = r.blen, out[4] = r.mlen, out[5] = (int32_t)p->n_ambi, out[6] = p->dp_max;
	free(p);
	return out[0];
}

int pgref_test_zdrop(const mm_mapopt_t *opt, const uint8_t *qseq, const uint8_t *tseq, uint32_t n_cigar, uint32_t *cigar, const int8_t *mat)
{
	return mm_test_zdrop(0, opt, qseq, tseq, n_cigar, cigar, mat);
}

#ifdef PGREF_PLAN_TRACE
/* ---- the region planner's expectation: wrappers around the reference's own chain trimming, seed filters and mm_align1 ---- */

/* mm_gen_regs (hit.c) of ONE chain, a[as .. as + cnt): out = rid, rev, rs, re, qs, qe, mlen, blen.  r->as is set to `as` afterwards. */
static void pgref_reg_of_chain(int qlen, mm128_t *a, int as, int cnt, mm_reg1_t *r)
{
	uint64_t u = (uint64_t)cnt;             /* score 0: nothing here reads it */
	mm_reg1_t *g = mm_gen_regs(0, 0, qlen, 1, &u, a + as, 0);
	*r = *g; free(g);
	r->as = as;
}

void pgref_chain_extent(int qlen, mm128_t *a, int as, int cnt, int32_t out[8])
{
	mm_reg1_t r;
	pgref_reg_of_chain(qlen, a, as, cnt, &r);
	out[0] = r.rid, out[1] = r.rev, out[2] = r.rs, out[3] = r.re, out[4] = r.qs, out[5] = r.qe, out[6] = r.mlen, out[7] = r.blen;
}

/* what mm_align1 runs on a chain before its windows (align.c: mm_fix_bad_ends unless no_end_flt, then both seed filters), on the caller's
 * anchor array, which keeps the flags: out = as1, cnt1 */
void pgref_trim_and_filter(int qlen, mm128_t *a, int as, int cnt, int bw, int min_chain_score, int max_gap, int no_end_flt, int32_t out[2])
{
	mm_reg1_t r;
	int32_t as1 = as, cnt1 = cnt;
	pgref_reg_of_chain(qlen, a, as, cnt, &r);
	if (!no_end_flt) mm_fix_bad_ends(&r, a, bw, min_chain_score * 2, &as1, &cnt1);
	mm_filter_bad_seeds(0, as1, cnt1, a, 10, 40, max_gap >> 1, 10);
	mm_filter_bad_seeds_alt(0, as1, cnt1, a, 30, max_gap >> 1);
	out[0] = as1, out[1] = cnt1;
}

/* the log of the stand-ins: eight values per DP call */
#define PGREF_LOG_W 8
static int32_t *pgref_log; static int64_t pgref_log_n, pgref_log_cap;
static const uint8_t *pgref_qbuf; static int pgref_qlen;

static void pgref_log_call(int qlen, const uint8_t *query, int tlen, int w, int zdrop, int end_bonus, int flag, ksw_extz_t *ez)
{
	/* the query strands lie in one buffer, forward at 0 and reverse complement at qlen + 1: the pointer says which strand and where */
	int64_t off = query - pgref_qbuf; int strand = 0;
	if (off > pgref_qlen) strand = 1, off -= pgref_qlen + 1;
	if (pgref_log_n < pgref_log_cap) {
		int32_t *p = pgref_log + pgref_log_n * PGREF_LOG_W;
		p[0] = strand, p[1] = (int32_t)off, p[2] = qlen, p[3] = tlen, p[4] = w, p[5] = zdrop, p[6] = end_bonus, p[7] = flag;
	}
	++pgref_log_n;
	ksw_reset_extz(ez);
	if (!(flag & KSW_EZ_EXTZ_ONLY)) {       /* the bookkeeping list of a gap-fill call (see the header comment) */
		int m = qlen < tlen ? qlen : tlen;
		ez->score = 0;
		if (m > 0) ez->cigar = ksw_push_cigar(0, &ez->n_cigar, &ez->m_cigar, ez->cigar, KSW_CIGAR_MATCH, m);
		if (qlen > m) ez->cigar = ksw_push_cigar(0, &ez->n_cigar, &ez->m_cigar, ez->cigar, KSW_CIGAR_INS, qlen - m);
		if (tlen > m) ez->cigar = ksw_push_cigar(0, &ez->n_cigar, &ez->m_cigar, ez->cigar, KSW_CIGAR_DEL, tlen - m);
	}
}

void pgref_log_extd2(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat,
                     int8_t q, int8_t e, int8_t q2, int8_t e2, int w, int zdrop, int end_bonus, int flag, ksw_extz_t *ez)
{
	pgref_log_call(qlen, query, tlen, w, zdrop, end_bonus, flag, ez);
}

void pgref_log_extz2(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat,
                     int8_t q, int8_t e, int w, int zdrop, int end_bonus, int flag, ksw_extz_t *ez)
{
	pgref_log_call(qlen, query, tlen, w, zdrop, end_bonus, flag, ez);
}

/* mm_align1 of the chain a[as .. as + cnt) of a query (forward base codes q, qlen) against an index built with mm_idx_str, with the DP replaced
 * by the stand-ins.  The anchors keep the flags.  Returns the number of DP calls made; the first log_cap of them are in log (eight values each). */
int64_t pgref_align1_trace(const mm_mapopt_t *opt, const mm_idx_t *mi, int qlen, const uint8_t *q, int n_a, mm128_t *a, int as, int cnt,
                           int32_t *log, int64_t log_cap)
{
	mm_reg1_t r, r2;
	ksw_extz_t ez;
	uint8_t *buf = (uint8_t*)malloc(2 * (size_t)qlen + 2), *qseq0[2];
	int i;
	qseq0[0] = buf, qseq0[1] = buf + qlen + 1;
	buf[qlen] = buf[2 * qlen + 1] = 4;
	for (i = 0; i < qlen; ++i) qseq0[0][i] = q[i], qseq0[1][qlen - 1 - i] = q[i] < 4 ? 3 - q[i] : 4;
	pgref_qbuf = buf, pgref_qlen = qlen, pgref_log = log, pgref_log_n = 0, pgref_log_cap = log_cap;
	memset(&ez, 0, sizeof(ez)); memset(&r2, 0, sizeof(r2));
	if (cnt > 0) pgref_reg_of_chain(qlen, a, as, cnt, &r);
	else { memset(&r, 0, sizeof(r)); r.as = as; }
	mm_align1(0, opt, mi, qlen, qseq0, &r, &r2, n_a, a, &ez, 0);
	free(ez.cigar); free(r.p); free(r2.p); free(buf);
	pgref_log = 0;
	return pgref_log_n;
}
#endif /* PGREF_PLAN_TRACE */
