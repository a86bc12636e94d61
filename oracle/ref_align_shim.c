/* ref_align_shim.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The reference keeps mm_update_extra, mm_fix_cigar and mm_test_zdrop static in align.c.  This file
 * includes that translation unit as it stands and exports two wrappers, so that the tests can call the
 * reference's own code on explicit sequences and operation lists (oracle/Makefile: libmm2ref_align.so).
 * Nothing of the reference is restated here.
 */
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
