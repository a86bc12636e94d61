"""pga_slice_blocks at merge scale, end to end (validation, host-to-device, kernels, device-to-host: wall time of the C call alone), beside a
plain single-threaded host loop with the reference's structure (slice.rs:136-202 inside reweave.rs:427-438: block after block, interval after
interval, member after member, every list scanned again for every interval and once more for the coordinates), compiled from the C below
with gcc -O2.  Shape: n_blocks blocks of block_len letters (+-20 %), `depth` members each, ~0.1 % edits per member (a third each
substitutions, deletions of 1..20, insertions of 1..20, lists sorted by position), 3 to 5 intervals per block that tile it.
usage: dev/slice_bench.py [n_blocks=2000] [depth=500] [block_len=10000] [repeats=5]"""
import sys, os, time, json, subprocess, tempfile, ctypes as C
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from pangraph_amd import slice as sl

HOST_C = r"""
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "pga_align.h"
/* the reference's loops, nothing shared between intervals; returns kept members, totals in tot[5] = kept, dropped, subs, dels, inss */
int64_t host_slice(int64_t n_blocks, const pga_slice_block_t *blocks, const pga_slice_interval_t *iv, const pga_rc_member_t *mem, const pga_slice_node_t *nodes,
                   const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss, pga_slice_member_t *om, pga_sub_t *os, pga_del_t *od, pga_ins_t *oi, uint64_t *tot)
{
	uint64_t m0 = 0, i0 = 0, s0 = 0, d0 = 0, n0 = 0, k = 0, ns = 0, nd = 0, ni = 0, dropped = 0;
	for (int64_t b = 0; b < n_blocks; ++b) {
		const uint32_t L = blocks[b].cons_len;
		uint8_t *gone = (uint8_t*)malloc(L);
		for (uint32_t j = 0; j < blocks[b].n_intervals; ++j) {
			const pga_slice_interval_t X = iv[i0 + j];
			uint64_t s1 = s0, d1 = d0, n1 = n0;
			for (uint32_t m = 0; m < blocks[b].n_members; ++m) {
				const pga_rc_member_t c = mem[m0 + m]; const pga_slice_node_t N = nodes[m0 + m];
				const uint64_t ks = ns, kd = nd, ki = ni;
				uint64_t dl = 0, il = 0, s = X.start, e = X.end;
				for (uint32_t t = 0; t < c.n_subs; ++t) if (subs[s1 + t].pos >= X.start && subs[s1 + t].pos < X.end) { os[ns].pos = subs[s1 + t].pos - X.start; os[ns++].alt = subs[s1 + t].alt; }
				for (uint32_t t = 0; t < c.n_dels; ++t) {
					const uint32_t p = dels[d1 + t].pos, q = p + dels[d1 + t].len;
					if (X.end > p && X.start < q) { const uint32_t a = p > X.start ? p : X.start, z = q < X.end ? q : X.end; od[nd].pos = a - X.start; od[nd++].len = z - a; dl += z - a; }
				}
				for (uint32_t t = 0; t < c.n_inss; ++t) {
					const pga_ins_t x = inss[n1 + t];
					if ((x.pos >= X.start && x.pos < X.end) || (x.pos == L && X.end == L)) { oi[ni] = x; oi[ni++].pos = x.pos - X.start; il += x.len; }
				}
				for (uint32_t t = 0; t < c.n_dels; ++t) {                       /* interval_node_coords */
					const uint32_t p = dels[d1 + t].pos, q = p + dels[d1 + t].len;
					if (p <= X.start) s -= (q < X.start ? q : X.start) - p;
					if (p < X.end) e -= (q < X.end ? q : X.end) - p;
				}
				for (uint32_t t = 0; t < c.n_inss; ++t) {
					const pga_ins_t x = inss[n1 + t];
					if (x.pos < X.start) s += x.len;
					if (x.pos < X.end) e += x.len;
					if (x.pos == X.end && x.pos == L) e += x.len;
				}
				int empty = 0;
				if (il == 0 && dl >= X.end - X.start) {                          /* is_empty_alignment: apply, then look */
					memset(gone, 0, X.end - X.start);
					for (uint64_t t = kd; t < nd; ++t) memset(gone + od[t].pos, 1, od[t].len);
					empty = 1;
					for (uint32_t t = 0; t < X.end - X.start; ++t) if (!gone[t]) { empty = 0; break; }
				}
				if (empty) { ns = ks; nd = kd; ni = ki; ++dropped; }
				else {
					pga_slice_member_t o; memset(&o, 0, sizeof(o));
					o.member = m; o.reverse = (N.reverse != 0) != (X.flip != 0); o.node_start = (uint32_t)s; o.node_end = (uint32_t)e;
					if (N.circular) { if (!N.reverse) { o.pos_start = (N.pos_start + s) % N.path_len; o.pos_end = (N.pos_start + e) % N.path_len; }
					                  else { o.pos_start = (N.pos_end + N.path_len - e) % N.path_len; o.pos_end = (N.pos_end + N.path_len - s) % N.path_len; } }
					else if (!N.reverse) { o.pos_start = N.pos_start + s; o.pos_end = N.pos_start + e; }
					else { o.pos_start = N.pos_end - e; o.pos_end = N.pos_end - s; }
					o.counts.n_subs = (uint32_t)(ns - ks); o.counts.n_dels = (uint32_t)(nd - kd); o.counts.n_inss = (uint32_t)(ni - ki);
					o.sub_off = ks; o.del_off = kd; o.ins_off = ki;
					om[k++] = o;
				}
				s1 += c.n_subs; d1 += c.n_dels; n1 += c.n_inss;
			}
			if (j + 1 == blocks[b].n_intervals) { s0 = s1; d0 = d1; n0 = n1; }
		}
		if (blocks[b].n_intervals == 0) for (uint32_t m = 0; m < blocks[b].n_members; ++m) { s0 += mem[m0 + m].n_subs; d0 += mem[m0 + m].n_dels; n0 += mem[m0 + m].n_inss; }
		free(gone);
		m0 += blocks[b].n_members; i0 += blocks[b].n_intervals;
	}
	tot[0] = k; tot[1] = dropped; tot[2] = ns; tot[3] = nd; tot[4] = ni;
	return (int64_t)k;
}
"""


def edit_list(rng, counts, L_of_member, kind):
    """one of the three lists for all members: positions sorted inside every member"""
    member_of = np.repeat(np.arange(len(counts)), counts)
    pos = (rng.random(len(member_of)) * L_of_member[member_of]).astype(np.uint32)
    order = np.lexsort((pos, member_of))
    pos = pos[order]; member_of = member_of[order]
    if kind == "subs":
        a = np.zeros(len(pos), dtype=[("pos", "u4"), ("alt", "u4")]); a["alt"] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, len(pos))]
    elif kind == "dels":
        a = np.zeros(len(pos), dtype=[("pos", "u4"), ("len", "u4")]); a["len"] = np.minimum(rng.integers(1, 21, len(pos)), L_of_member[member_of] - pos)
    else:
        a = np.zeros(len(pos), dtype=[("pos", "u4"), ("len", "u4"), ("seq_off", "u8")]); a["len"] = rng.integers(1, 21, len(pos))
        a["seq_off"] = np.cumsum(a["len"], dtype=np.uint64) - a["len"]
    a["pos"] = pos
    return a


if __name__ == "__main__":
    n_blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    depth = int(sys.argv[2]) if len(sys.argv) > 2 else 500
    L = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
    repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    rng = np.random.default_rng(20261018)
    dll = C.CDLL(os.path.join(ROOT, "pangraph_amd", "libpgalign.so"))
    sl._bind(dll)
    lens = (L * rng.uniform(0.8, 1.2, n_blocks)).astype(np.uint32)
    cons = b"A" * int(lens.max())                                             # never read
    B = (sl.slice_block_t * n_blocks)()
    ivs = []
    for b in range(n_blocks):
        n_int = int(rng.integers(3, 6))
        cuts = [0] + sorted(int(x) for x in rng.choice(np.arange(1, lens[b]), n_int - 1, replace=False)) + [int(lens[b])]
        ivs += [(a, z, int(rng.integers(0, 2))) for a, z in zip(cuts, cuts[1:])]
        B[b].consensus = cons; B[b].cons_len = int(lens[b]); B[b].n_members = depth; B[b].n_intervals = n_int
    V = np.array(ivs, dtype=[("start", "u4"), ("end", "u4"), ("flip", "i4")])
    n_mem = n_blocks * depth
    L_of_member = np.repeat(lens, depth).astype(np.int64)
    M = np.zeros(n_mem, dtype=[("n_subs", "u4"), ("n_dels", "u4"), ("n_inss", "u4")])
    for f in ("n_subs", "n_dels", "n_inss"):
        M[f] = rng.poisson(L_of_member * 0.001 / 3)
    S, D, I = (edit_list(rng, M[f].astype(np.int64), L_of_member, k) for f, k in (("n_subs", "subs"), ("n_dels", "dels"), ("n_inss", "inss")))
    N = np.zeros(n_mem, dtype=[("pos_start", "u8"), ("pos_end", "u8"), ("path_len", "u8"), ("reverse", "i4"), ("circular", "i4")])
    N["pos_start"] = rng.integers(0, 10 ** 6, n_mem); N["pos_end"] = N["pos_start"] + 2 * L_of_member.astype(np.uint64); N["path_len"] = 4 * 10 ** 6
    N["reverse"] = rng.integers(0, 2, n_mem); N["circular"] = rng.integers(0, 2, n_mem)
    n_edits = len(S) + len(D) + len(I)
    args = (n_blocks, B, V.ctypes.data, M.ctypes.data, N.ctypes.data, S.ctypes.data, D.ctypes.data, I.ctypes.data)
    # ---- the host loop, compiled here ----
    tmp = tempfile.mkdtemp()
    open(os.path.join(tmp, "host_slice.c"), "w").write(HOST_C)
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "host_slice.c"), "-o", os.path.join(tmp, "host_slice.so")], check=True)
    host = C.CDLL(os.path.join(tmp, "host_slice.so"))
    host.host_slice.restype = C.c_int64
    host.host_slice.argtypes = [C.c_int64] + [C.c_void_p] * 12
    n_pairs = depth * len(V)
    om = np.zeros(n_pairs, dtype=np.dtype((np.void, C.sizeof(sl.slice_member_t))))
    os_, od, oi = np.zeros(len(S) + 1, dtype=S.dtype), np.zeros(5 * len(D) + 1, dtype=D.dtype), np.zeros(len(I) + 1, dtype=I.dtype)
    tot = (C.c_uint64 * 5)()
    t_dev, t_host, same = [], [], None
    for it in range(repeats + 1):                                             # the first round of both is the warm-up
        out = sl.slice_out_t()
        t0 = time.perf_counter()
        rc = dll.pga_slice_blocks(*args, C.byref(out))
        t1 = time.perf_counter()
        assert rc == 0, dll.pga_last_error()
        host.host_slice(*args, om.ctypes.data, os_.ctypes.data, od.ctypes.data, oi.ctypes.data, tot)
        t2 = time.perf_counter()
        if it == 0:                                                           # the two routes agree: every record and every sliced edit, as bytes
            kept, ns, nd, ni = tot[0], tot[2], tot[3], tot[4]
            dev_kept = sum(out.slices[s].n_kept for s in range(len(V)))
            same = (dev_kept == kept and C.string_at(out.members, kept * C.sizeof(sl.slice_member_t)) == om[:kept].tobytes()
                    and C.string_at(out.subs, ns * 8) == os_[:ns].tobytes() and C.string_at(out.dels, nd * 8) == od[:nd].tobytes() and C.string_at(out.inss, ni * 16) == oi[:ni].tobytes())
        else:
            t_dev.append(t1 - t0); t_host.append(t2 - t1)
        dll.pga_slice_free(C.byref(out))
    med = lambda t: float(np.median(t))
    print(json.dumps(dict(blocks=n_blocks, depth=depth, block_len=L, members=n_mem, intervals=len(V), pairs=n_pairs, edits=n_edits, repeats=repeats,
                          kept=int(tot[0]), dropped=int(tot[1]),
                          slice_blocks_s=dict(median=round(med(t_dev), 4), min=round(min(t_dev), 4), max=round(max(t_dev), 4)),
                          host_loop_s=dict(median=round(med(t_host), 4), min=round(min(t_host), 4), max=round(max(t_host), 4)),
                          edits_per_s=dict(slice_blocks=round(n_edits / med(t_dev)), host_loop=round(n_edits / med(t_host))),
                          identical=bool(same))))
