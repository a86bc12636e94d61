"""pga_core_alignment at build scale, end to end (validation, core selection, row tables, host-to-device, kernel, device-to-host through the
pinned tiles, the sink: wall time of the C call alone) in sink mode and in verdict mode, beside a plain single-threaded host loop with the
reference's structure (core_block_aln, export_core_genome.rs:53-107, over Edit::apply_aligned, edits.rs:331-347: per core block and member
copy the consensus, substitute, overwrite deletions with '-', reverse-complement where the guide is reverse, append to the member's
record), compiled from the C below with gcc -O2.  The sink is C too: it copies every segment of a tile to its place in one preallocated
array of n_paths rows.  Shape: n_paths paths that each hold every one of n_blocks blocks of block_len letters (+-20 %) once, so every block
is core; ~0.1 % edits per member (a third each substitutions, deletions of 1..20, insertions of 1..20, which the aligned rows ignore), 5 % of
the guide's nodes reverse.  The three times are taken alternating on the same input, the median of `repeats` rounds after a warm-up; the
kernel's own time comes from the library's busy log (HIP events).
The timed work runs in a CHILD process that this script starts fresh, under a time limit; the parent reports when the child's results
were printed and when the child exited, separately (a process that has its results and does not end is a finding of its own).
usage: dev/export_bench.py [n_paths=200] [n_blocks=500] [block_len=2000] [repeats=5]      (200 x 500 x 2000 = 200 M letters)"""
import sys, os, time, json, subprocess, tempfile, ctypes as C
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

CHILD_LIMIT_S = 900       # the child as a whole
EXIT_LIMIT_S = 120        # from its results to its exit

HOST_C = r"""
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "pga_align.h"
typedef struct { char *out; uint64_t stride; uint64_t tiles, letters; } sink_ctx_t;
/* the sink: row r lies at out + r * stride */
int sink_copy(void *ctx, int64_t n_seg, const pga_export_seg_t *segs, const char *letters)
{
	sink_ctx_t *c = (sink_ctx_t*)ctx;
	for (int64_t i = 0; i < n_seg; ++i) { memcpy(c->out + segs[i].row * c->stride + segs[i].row_off, letters + segs[i].tile_off, segs[i].n); c->letters += segs[i].n; }
	++c->tiles;
	return 0;
}
/* the reference's loops over the core blocks in guide order; member j of a block lies on path j; returns the letters written, -1 on a rejected complement */
int64_t host_core_alignment(const pga_rc_block_t *blocks, const pga_rc_member_t *mem, const pga_sub_t *subs, const pga_del_t *dels, int64_t n_mem, int64_t n_paths,
                            int64_t n_core, const pga_core_block_t *core, char *out, uint64_t stride)
{
	static unsigned char comp[256];
	const char *from = "ACGTYRWSKMDVHBN-", *to = "TGCARYWSMKHBDVN-";
	for (int i = 0; i < 16; ++i) comp[(unsigned char)from[i]] = (unsigned char)to[i];
	uint64_t *s0 = (uint64_t*)malloc((n_mem + 1) * 8), *d0 = (uint64_t*)malloc((n_mem + 1) * 8), max_len = 0;
	s0[0] = d0[0] = 0;
	for (int64_t m = 0; m < n_mem; ++m) { s0[m + 1] = s0[m] + mem[m].n_subs; d0[m + 1] = d0[m] + mem[m].n_dels; }
	for (int64_t c = 0; c < n_core; ++c) if (core[c].cons_len > max_len) max_len = core[c].cons_len;
	char *buf = (char*)malloc(max_len + 1);
	int64_t total = 0;
	for (int64_t c = 0; c < n_core; ++c) {
		const pga_rc_block_t B = blocks[core[c].block];
		const uint64_t len = B.cons_len;
		for (int64_t p = 0; p < n_paths; ++p) {
			const uint64_t m = (uint64_t)core[c].block * n_paths + p;
			char *dst = out + p * stride + core[c].col;
			memcpy(buf, B.consensus, len);                                                          /* Edit::apply_aligned */
			for (uint64_t t = s0[m]; t < s0[m + 1]; ++t) buf[subs[t].pos] = (char)subs[t].alt;
			for (uint64_t t = d0[m]; t < d0[m + 1]; ++t) memset(buf + dels[t].pos, '-', dels[t].len);
			if (core[c].reverse) {                                                                  /* reverse_complement */
				for (uint64_t r = 0; r < len; ++r) { const unsigned char x = comp[(unsigned char)buf[len - 1 - r]]; if (!x) return -1; dst[r] = (char)x; }
			} else memcpy(dst, buf, len);
			total += (int64_t)len;
		}
	}
	free(buf); free(s0); free(d0);
	return total;
}
"""


def child(n_paths, n_blocks, L, repeats):
    import numpy as np
    from pangraph_amd import export as ex, reconstruct as rc
    rng = np.random.default_rng(20261018)
    dll = C.CDLL(os.path.join(ROOT, "pangraph_amd", "libpgalign.so"))
    ex._bind(dll)
    dll.pga_busy_begin.restype = C.c_int
    dll.pga_busy_end.restype = C.c_int
    dll.pga_busy_end.argtypes = [C.POINTER(C.c_double), C.c_int32]
    # ---- the graph: every block has one member per path (member j on path j); per member one edit in each stratum of ~1000 letters ----
    lens = (L * rng.uniform(0.8, 1.2, n_blocks)).astype(np.int64)
    cons_off = np.concatenate(([0], np.cumsum(lens)))
    cons = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(cons_off[-1]))].copy()
    B = (rc.rc_block_t * n_blocks)()
    for b in range(n_blocks):
        B[b].consensus = C.cast(cons.ctypes.data + int(cons_off[b]), C.c_char_p); B[b].cons_len = int(lens[b]); B[b].n_members = n_paths
    n_mem = n_blocks * n_paths
    L_of = np.repeat(lens, n_paths)
    n_edit = np.maximum(L_of // 1000, 1)
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
    member_path = (np.arange(n_mem) % n_paths).astype(np.uint32)
    G = np.zeros(n_blocks, dtype=[("member", "u8"), ("reverse", "i4"), ("pad", "i4")])              # the guide: path 0, the blocks in an order of its own
    G["member"] = rng.permutation(n_blocks) * n_paths
    G["reverse"] = rng.random(n_blocks) < 0.05
    cols = int(lens.sum())
    total = cols * n_paths
    R = (ex.export_res_t * n_paths)()
    core_p, n_core = C.POINTER(ex.core_block_t)(), C.c_int64(0)
    # ---- the host loop and the sink, compiled here ----
    tmp = tempfile.mkdtemp()
    open(os.path.join(tmp, "host_export.c"), "w").write(HOST_C)
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "host_export.c"), "-o", os.path.join(tmp, "host_export.so")], check=True)
    host = C.CDLL(os.path.join(tmp, "host_export.so"))
    host.host_core_alignment.restype = C.c_int64
    host.host_core_alignment.argtypes = [C.c_void_p] * 4 + [C.c_int64] * 3 + [C.c_void_p, C.c_void_p, C.c_uint64]

    class sink_ctx_t(C.Structure):
        _fields_ = [("out", C.c_void_p), ("stride", C.c_uint64), ("tiles", C.c_uint64), ("letters", C.c_uint64)]
    dev_rows = np.zeros((n_paths, cols), dtype=np.uint8)
    host_rows = np.zeros((n_paths, cols), dtype=np.uint8)
    ctx = sink_ctx_t(dev_rows.ctypes.data, cols, 0, 0)
    sink = C.cast(host.sink_copy, C.c_void_p)

    def call(with_sink):
        if core_p:
            dll.pga_free(C.cast(core_p, C.c_void_p))
        ctx.tiles = ctx.letters = 0
        rc_ = dll.pga_core_alignment(n_blocks, B, M.ctypes.data, S.ctypes.data, D.ctypes.data, I.ctypes.data, letters.ctypes.data, member_path.ctypes.data, n_paths, 0, n_blocks,
                                     G.ctypes.data, 1, None, R, C.byref(core_p), C.byref(n_core), sink if with_sink else None, C.addressof(ctx) if with_sink else None)
        assert rc_ == 0, dll.pga_last_error()
        assert all(R[p].status == 0 and R[p].len == cols for p in range(n_paths)) and n_core.value == n_blocks

    def host_loop():
        return host.host_core_alignment(B, M.ctypes.data, S.ctypes.data, D.ctypes.data, n_mem, n_paths, n_core.value, core_p, host_rows.ctypes.data, cols)
    # ---- the two routes agree byte for byte before anything is timed ----
    call(True)
    assert ctx.letters == total, (ctx.letters, total)
    assert host_loop() == total
    same = bool(np.array_equal(dev_rows, host_rows))
    assert same, "the device rows differ from the host loop's"
    tiles = int(ctx.tiles)
    t_sink, t_verdict, t_host, k_sink, k_verdict = [], [], [], [], []
    busy = (C.c_double * 18)()
    for it in range(repeats + 1):                                             # the first round of all three is the warm-up
        dll.pga_busy_begin()
        t0 = time.perf_counter()
        call(True)
        t1 = time.perf_counter()
        dll.pga_busy_end(busy, 18); ks = busy[17]
        dll.pga_busy_begin()
        t2 = time.perf_counter()
        call(False)
        t3 = time.perf_counter()
        dll.pga_busy_end(busy, 18); kv = busy[17]
        t4 = time.perf_counter()
        host_loop()
        t5 = time.perf_counter()
        if it:
            t_sink.append(t1 - t0); t_verdict.append(t3 - t2); t_host.append(t5 - t4); k_sink.append(ks); k_verdict.append(kv)
    med = lambda t: float(np.median(t))
    stat = lambda t: dict(median=round(med(t), 4), min=round(min(t), 4), max=round(max(t), 4))
    print("RESULT " + json.dumps(dict(paths=n_paths, blocks=n_blocks, block_len=L, members=n_mem, edits=tot_e, letters=total, tiles=tiles, repeats=repeats, identical=same,
                                      sink_s=stat(t_sink), verdict_s=stat(t_verdict), host_loop_s=stat(t_host),
                                      letters_per_s=dict(sink=round(total / med(t_sink)), verdict=round(total / med(t_verdict)), host_loop=round(total / med(t_host))),
                                      sink_gb_s=round(total / med(t_sink) / 1e9, 2),
                                      kernel_ms=dict(sink=round(med(k_sink), 3), verdict=round(med(k_verdict), 3)))), flush=True)
    dll.pga_free(C.cast(core_p, C.c_void_p))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*[int(x) for x in sys.argv[2:6]])
        sys.exit(0)
    args = [int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 200), (2, 500), (3, 2000), (4, 5))]
    t_start = time.monotonic()
    proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"] + [str(a) for a in args], stdout=subprocess.PIPE, text=True)
    import threading
    t_result = [None]

    def reader():
        for line in proc.stdout:
            if line.startswith("RESULT "):
                t_result[0] = time.monotonic()
                print(line[len("RESULT "):].rstrip(), flush=True)
            else:
                print("child: " + line.rstrip(), flush=True)
    th = threading.Thread(target=reader, daemon=True)
    th.start()
    exited = None
    while time.monotonic() - t_start < CHILD_LIMIT_S:
        if proc.poll() is not None:
            exited = time.monotonic()
            break
        if t_result[0] is not None and time.monotonic() - t_result[0] > EXIT_LIMIT_S:
            break
        time.sleep(0.05)
    if exited is None:
        proc.kill(); proc.wait()
    th.join(5)
    if t_result[0] is not None:
        print(f"results printed: {t_result[0] - t_start:.2f} s after the child was started")
    else:
        print("results printed: never")
    if exited is not None:
        since = f", {exited - t_result[0]:.2f} s after its results" if t_result[0] is not None else ""
        print(f"child exited: status {proc.returncode}, {exited - t_start:.2f} s after it was started{since}")
    else:
        print(f"child exited: NO -- killed {time.monotonic() - t_start:.0f} s after it was started")
    sys.exit(0 if exited is not None and proc.returncode == 0 and t_result[0] is not None else 3)
