/* ref_index_shim.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The reference keeps mm_idx_add and mm_idx_post static in index.c.  This file includes that translation unit as it
 * stands and exports one wrapper, so that the tests can build the reference's own index from minimizers given as they
 * are (occurrence counts chosen by a test, not produced by sketching).  Nothing of the reference is restated here.
 * It is linked in place of index.o into oracle/_ref/libmm2ref_seed.so (oracle/Makefile), next to ref_map_shim.c;
 * index.c and map.c both define pipeline_t, step_t and worker_pipeline, so the two cannot share a translation unit.
 */
#include "index.c"

/* mm_idx_init + mm_idx_add + mm_idx_post (one thread) of the n minimizers a[], then the sequence table that skip_seed
 * reads: n_seq names and lengths.  No bases are stored (mi->S stays empty).  Freed with mm_idx_destroy. */
mm_idx_t *pgref_idx_of_minimizers(int w, int k, int n, const mm128_t *a, int n_seq, const char *const *name, const uint32_t *len)
{
	int i;
	mm_idx_t *mi = mm_idx_init(w, k, 14, 0);
	mm_idx_add(mi, n, a);
	mm_idx_post(mi, 1);
	mi->n_seq = n_seq;
	mi->seq = (mm_idx_seq_t*)kcalloc(mi->km, n_seq > 0 ? n_seq : 1, sizeof(mm_idx_seq_t));
	for (i = 0; i < n_seq; ++i) {
		mi->seq[i].name = (char*)kmalloc(mi->km, strlen(name[i]) + 1);
		strcpy(mi->seq[i].name, name[i]);
		mi->seq[i].len = len[i];
	}
	return mi;
}
