"""pga_reconstruct at build scale, end to end (validation, run tables, host-to-device, kernel, device-to-host: wall time of the C call alone),
verify-only and write mode, beside a plain single-threaded host loop with the reference's structure (reconstruct_run.rs:78-127 over
Edit::apply, edits.rs:307-329: per node copy the consensus, substitute, overwrite deletions with '-', insert from the back, strip the gaps,
reverse-complement, append; rotate the genome at the end), compiled from the C below with gcc -O2.  Shape: n_paths paths that each visit all
of n_blocks blocks of block_len letters (+-20 %) once, in an order of their own, so every block has depth n_paths; ~0.1 % edits per
member (a third each substitutions, deletions of 1..20, insertions of 1..20), 5 % of the nodes on the reverse strand, a random rotation.
The three times are taken alternating on the same input; the kernel's own time comes from the library's busy log (HIP events).
usage: dev/recon_bench.py [n_paths=200] [n_blocks=500] [block_len=10000] [repeats=5]      (200 x 500 x 10000 = 1 G letters; scale down with n_paths)"""
import sys, os, time, json, subprocess, tempfile, ctypes as C
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from pangraph_amd import reconstruct as rc

HBM_PEAK_GBS = 8000.0     # what bench.py's roofline uses

HOST_C = r"""
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "pga_align.h"
/* the reference's loops; path p is written to out + seq_off[p]; returns the letters written, -1 on a rejected complement */
int64_t host_reconstruct(int64_t n_blocks, const pga_rc_block_t *blocks, const pga_rc_member_t *mem, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss,
                         const char *ins_seq, int64_t n_paths, const pga_recon_path_t *paths, const pga_recon_node_t *nodes, const uint64_t *seq_off, char *out)
{
	static unsigned char comp[256];
	const char *from = "ACGTYRWSKMDVHBN-", *to = "TGCARYWSMKHBDVN-";
	for (int i = 0; i < 16; ++i) comp[(unsigned char)from[i]] = (unsigned char)to[i];
	uint64_t n_mem = 0, max_len = 0;
	for (int64_t b = 0; b < n_blocks; ++b) n_mem += blocks[b].n_members;
	uint32_t *blk_of = (uint32_t*)malloc(n_mem * sizeof(uint32_t));
	uint64_t *s0 = (uint64_t*)malloc((n_mem + 1) * 8), *d0 = (uint64_t*)malloc((n_mem + 1) * 8), *i0 = (uint64_t*)malloc((n_mem + 1) * 8);
	s0[0] = d0[0] = i0[0] = 0;
	for (uint64_t b = 0, m = 0; b < (uint64_t)n_blocks; ++b) for (uint32_t k = 0; k < blocks[b].n_members; ++k, ++m) {
		blk_of[m] = (uint32_t)b; s0[m + 1] = s0[m] + mem[m].n_subs; d0[m + 1] = d0[m] + mem[m].n_dels; i0[m + 1] = i0[m] + mem[m].n_inss;
		uint64_t l = blocks[b].cons_len; for (uint64_t t = i0[m]; t < i0[m + 1]; ++t) l += inss[t].len;
		if (l > max_len) max_len = l;
	}
	char *buf = (char*)malloc(max_len + 1);
	int64_t total = 0; uint64_t k = 0;
	for (int64_t p = 0; p < n_paths; ++p) {
		char *genome = out + seq_off[p]; uint64_t g = 0;
		for (uint32_t j = 0; j < paths[p].n_nodes; ++j, ++k) {
			const uint64_t m = nodes[k].member; const pga_rc_block_t B = blocks[blk_of[m]];
			uint64_t len = B.cons_len;
			memcpy(buf, B.consensus, len);                                                          /* Edit::apply */
			for (uint64_t t = s0[m]; t < s0[m + 1]; ++t) buf[subs[t].pos] = (char)subs[t].alt;
			for (uint64_t t = d0[m]; t < d0[m + 1]; ++t) memset(buf + dels[t].pos, '-', dels[t].len);
			for (uint64_t t = i0[m + 1]; t-- > i0[m];) {                                            /* sorted by position: from the back */
				memmove(buf + inss[t].pos + inss[t].len, buf + inss[t].pos, len - inss[t].pos);
				memcpy(buf + inss[t].pos, ins_seq + inss[t].seq_off, inss[t].len); len += inss[t].len;
			}
			uint64_t w = 0;
			for (uint64_t r = 0; r < len; ++r) if (buf[r] != '-') buf[w++] = buf[r];
			len = w;
			if (nodes[k].reverse) {                                                                 /* reverse_complement */
				for (uint64_t r = 0; r < len; ++r) { const unsigned char c = comp[(unsigned char)buf[len - 1 - r]]; if (!c) return -1; genome[g + r] = (char)c; }
			} else memcpy(genome + g, buf, len);
			g += len;
		}
		if (g != paths[p].tot_len || paths[p].first_pos > g) return -2;
		if (g && paths[p].first_pos % g) {                                                        /* rotate_right */
			const uint64_t r = paths[p].first_pos % g;
			char *tmp = (char*)malloc(r);
			memcpy(tmp, genome + g - r, r); memmove(genome + r, genome, g - r); memcpy(genome, tmp, r);
			free(tmp);
		}
		total += (int64_t)g;
	}
	free(buf); free(blk_of); free(s0); free(d0); free(i0);
	return total;
}
"""


if __name__ == "__main__":
    n_paths = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    n_blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 500
    L = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
    repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    rng = np.random.default_rng(20261018)
    dll = C.CDLL(os.path.join(ROOT, "pangraph_amd", "libpgalign.so"))
    rc._bind(dll)
    dll.pga_busy_begin.restype = C.c_int
    dll.pga_busy_end.restype = C.c_int
    dll.pga_busy_end.argtypes = [C.POINTER(C.c_double), C.c_int32]
    # ---- the graph: every block has one member per path; per member 10 strata of its consensus, one edit in each ----
    lens = (L * rng.uniform(0.8, 1.2, n_blocks)).astype(np.int64)
    cons_off = np.concatenate(([0], np.cumsum(lens)))
    cons = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(cons_off[-1]))].copy()
    B = (rc.rc_block_t * n_blocks)()
    for b in range(n_blocks):
        B[b].consensus = C.cast(cons.ctypes.data + int(cons_off[b]), C.c_char_p); B[b].cons_len = int(lens[b]); B[b].n_members = n_paths
    n_mem = n_blocks * n_paths
    L_of = np.repeat(lens, n_paths)
    n_edit = np.maximum(L_of // 1000, 1)                                        # ~0.1 %: one edit per stratum of ~1000 letters
    tot_e = int(n_edit.sum())
    member_of = np.repeat(np.arange(n_mem), n_edit)
    rank = np.arange(tot_e) - np.repeat(np.cumsum(n_edit) - n_edit, n_edit)
    stratum = L_of[member_of] // n_edit[member_of]
    pos = (rank * stratum + (rng.random(tot_e) * (stratum - 40)).astype(np.int64)).astype(np.uint32)   # >= 40 apart: no edit reaches the next
    kind = rng.integers(0, 3, tot_e)
    M = np.zeros(n_mem, dtype=[("n_subs", "u4"), ("n_dels", "u4"), ("n_inss", "u4")])
    for k, f in enumerate(("n_subs", "n_dels", "n_inss")):
        M[f] = np.bincount(member_of[kind == k], minlength=n_mem)
    S = np.zeros(int((kind == 0).sum()), dtype=[("pos", "u4"), ("alt", "u4")]); S["pos"] = pos[kind == 0]
    S["alt"] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, len(S))]
    D = np.zeros(int((kind == 1).sum()), dtype=[("pos", "u4"), ("len", "u4")]); D["pos"] = pos[kind == 1]; D["len"] = rng.integers(1, 21, len(D))
    I = np.zeros(int((kind == 2).sum()), dtype=[("pos", "u4"), ("len", "u4"), ("seq_off", "u8")]); I["pos"] = pos[kind == 2]; I["len"] = rng.integers(1, 21, len(I))
    I["seq_off"] = np.cumsum(I["len"], dtype=np.uint64) - I["len"]
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(I["len"].sum()) + 1)].copy()
    # ---- the paths: path p visits every block once, as member p of it ----
    N = np.zeros(n_paths * n_blocks, dtype=[("member", "u8"), ("reverse", "i4"), ("pad", "i4")])
    for p in range(n_paths):
        N["member"][p * n_blocks:(p + 1) * n_blocks] = rng.permutation(n_blocks) * n_paths + p
    N["reverse"] = rng.random(len(N)) < 0.05
    Pt = np.zeros(n_paths, dtype=[("tot_len", "u8"), ("first_pos", "u8"), ("n_nodes", "u4"), ("pad", "u4")])
    Pt["n_nodes"] = n_blocks
    R = (rc.recon_res_t * n_paths)()
    graph = (n_blocks, B, M.ctypes.data, S.ctypes.data, D.ctypes.data, I.ctypes.data, letters.ctypes.data, n_paths, Pt.ctypes.data, N.ctypes.data)
    out = C.POINTER(C.c_char)()

    def call(expected, write):
        return dll.pga_reconstruct(*graph, exp_p if expected else None, exp_n if expected else None, R, C.byref(out) if write else None)
    # the built lengths come from a first call (status 1: tot_len is still 0); then tot_len and a rotation
    exp_p = exp_n = None
    assert call(False, True) == 0, dll.pga_last_error()
    dll.pga_free(C.cast(out, C.c_void_p))
    Pt["tot_len"] = [R[p].len for p in range(n_paths)]
    Pt["first_pos"] = (rng.random(n_paths) * Pt["tot_len"]).astype(np.uint64)
    total = int(Pt["tot_len"].sum())
    # ---- the host loop, compiled here; the two routes agree byte for byte before anything is timed ----
    tmp = tempfile.mkdtemp()
    open(os.path.join(tmp, "host_recon.c"), "w").write(HOST_C)
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "host_recon.c"), "-o", os.path.join(tmp, "host_recon.so")], check=True)
    host = C.CDLL(os.path.join(tmp, "host_recon.so"))
    host.host_reconstruct.restype = C.c_int64
    host.host_reconstruct.argtypes = [C.c_int64] + [C.c_void_p] * 6 + [C.c_int64] + [C.c_void_p] * 4
    assert call(False, True) == 0, dll.pga_last_error()
    assert all(R[p].status == 0 for p in range(n_paths)), [R[p].status for p in range(n_paths)][:10]
    seq_off = np.array([R[p].seq_off for p in range(n_paths)], dtype=np.uint64)
    span = int(seq_off[-1] + Pt["tot_len"][-1])
    hbuf = np.zeros(span + 16, dtype=np.uint8)
    assert host.host_reconstruct(*graph[:7], n_paths, Pt.ctypes.data, N.ctypes.data, seq_off.ctypes.data, hbuf.ctypes.data) == total
    dev = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), shape=(span,))
    same = all(np.array_equal(dev[int(o):int(o) + int(n)], hbuf[int(o):int(o) + int(n)]) for o, n in zip(seq_off, Pt["tot_len"]))
    # the expected sequences of verify mode: the host loop's
    exp_p = (C.c_void_p * n_paths)(*[hbuf.ctypes.data + int(o) for o in seq_off])
    exp_n = (C.c_uint64 * n_paths)(*[int(n) for n in Pt["tot_len"]])
    dll.pga_free(C.cast(out, C.c_void_p))
    t_verify, t_write, t_host, k_verify, k_write = [], [], [], [], []
    busy = (C.c_double * 17)()
    for it in range(repeats + 1):                                             # the first round of all three is the warm-up
        dll.pga_busy_begin()
        t0 = time.perf_counter()
        assert call(True, False) == 0, dll.pga_last_error()
        t1 = time.perf_counter()
        dll.pga_busy_end(busy, 17); kv = busy[15]
        assert all(R[p].status == 0 and R[p].n_mismatch == 0 for p in range(n_paths))
        dll.pga_busy_begin()
        t2 = time.perf_counter()
        assert call(False, True) == 0, dll.pga_last_error()
        t3 = time.perf_counter()
        dll.pga_busy_end(busy, 17); kw = busy[15]
        dll.pga_free(C.cast(out, C.c_void_p))
        t4 = time.perf_counter()
        host.host_reconstruct(*graph[:7], n_paths, Pt.ctypes.data, N.ctypes.data, seq_off.ctypes.data, hbuf.ctypes.data)
        t5 = time.perf_counter()
        if it:
            t_verify.append(t1 - t0); t_write.append(t3 - t2); t_host.append(t5 - t4); k_verify.append(kv); k_write.append(kw)
    med = lambda t: float(np.median(t))
    stat = lambda t: dict(median=round(med(t), 4), min=round(min(t), 4), max=round(max(t), 4))
    print(json.dumps(dict(paths=n_paths, blocks=n_blocks, block_len=L, members=n_mem, nodes=len(N), edits=tot_e, letters=total, repeats=repeats, identical=bool(same),
                          verify_only_s=stat(t_verify), write_mode_s=stat(t_write), host_loop_s=stat(t_host),
                          letters_per_s=dict(verify_only=round(total / med(t_verify)), write_mode=round(total / med(t_write)), host_loop=round(total / med(t_host))),
                          kernel_ms=dict(verify_only=round(med(k_verify), 3), write_mode=round(med(k_write), 3)),
                          # verify: the source letters and the expected letters are read; write: the source letters are read, the built ones written
                          kernel_gb_s=dict(verify_only=round(2 * total / med(k_verify) / 1e6, 1), write_mode=round(2 * total / med(k_write) / 1e6, 1), hbm_peak=HBM_PEAK_GBS))))
