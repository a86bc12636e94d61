"""The host side of the two exports of a finished graph, export block-sequences (PangraphBlock::sequences,
packages/pangraph/src/pangraph/pangraph_block.rs:135-189) and export core-genome (core_block_aln with concatenate_records,
commands/export/export_core_genome.rs:53-141): the loader that turns a pangraph JSON and a guide strain into the arrays a core alignment is
built from, in the layout of pangraph_amd.reconstruct, and the mirrors of the two device entries `pga_block_sequences` and `pga_core_alignment`
(include/pga_align.h; pga_export.hip): rows of letters are built on the device and handed, tile by tile, to a ctypes sink that collects them
in numpy.  ctypes only; the HIP library does the work."""
import ctypes as C

import numpy as np

from . import batch
from .reconstruct import _Packed, graph_from_json, recon_node_t


class export_seg_t(C.Structure):
    _fields_ = [("row", C.c_uint64), ("row_off", C.c_uint64), ("tile_off", C.c_uint64), ("n", C.c_uint32), ("pad", C.c_uint32)]


class export_res_t(C.Structure):
    _fields_ = [("status", C.c_int32), ("pad", C.c_int32), ("len", C.c_uint64)]


class core_block_t(C.Structure):
    _fields_ = [("block", C.c_uint32), ("reverse", C.c_int32), ("col", C.c_uint64), ("cons_len", C.c_uint32), ("pad", C.c_uint32)]


SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.POINTER(export_seg_t), C.POINTER(C.c_ubyte))
SEG_DTYPE = np.dtype([("row", "<u8"), ("row_off", "<u8"), ("tile_off", "<u8"), ("n", "<u4"), ("pad", "<u4")])
assert SEG_DTYPE.itemsize == C.sizeof(export_seg_t)


def _bind(dll):
    dll.pga_block_sequences.restype = C.c_int
    dll.pga_block_sequences.argtypes = [C.c_int64] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    dll.pga_core_alignment.restype = C.c_int
    dll.pga_core_alignment.argtypes = [C.c_int64] + [C.c_void_p] * 6 + [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                       C.POINTER(C.POINTER(core_block_t)), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]
    dll.pga_last_error.restype = C.c_char_p
    dll.pga_free.argtypes = [C.c_void_p]


class Collector:
    """a sink that keeps every tile: one callback per tile, one numpy copy of its segments and one of its letters.  `tiles` counts the
    calls; stop_at=k makes call number k (from 1) return 1, which stops the export."""

    def __init__(self, stop_at=None):
        self.segs, self.letters, self.tiles, self.stop_at, self.error = [], [], 0, stop_at, None
        self.fn = SINK(self._call)

    def _call(self, ctx, n_seg, segs, letters):
        try:
            self.tiles += 1
            if self.stop_at is not None and self.tiles >= self.stop_at:
                return 1
            if n_seg:
                s = np.ctypeslib.as_array(C.cast(segs, C.POINTER(C.c_ubyte)), shape=(n_seg * SEG_DTYPE.itemsize,)).view(SEG_DTYPE).copy()
                end = int(s["tile_off"][-1]) + int(s["n"][-1])
                self.segs.append(s)
                self.letters.append(np.ctypeslib.as_array(letters, shape=(end,)).copy())
            return 0
        except BaseException as e:                                       # (an exception must not cross the C frames)
            self.error = e
            return 1

    def rows(self, res):
        """the letters of every row as bytes, assembled from the segments: they must tile each non-empty row exactly once, in order"""
        out = [bytearray() for _ in res]
        for s, t in zip(self.segs, self.letters):
            for row, row_off, tile_off, n, _ in s.tolist():
                if len(out[row]) != row_off or n == 0:
                    raise batch.PgaError(f"export sink: segment of row {row} at {row_off} does not follow the {len(out[row])} letters delivered")
                out[row] += t[tile_off:tile_off + n].tobytes()
        for r, o in zip(res, out):
            if len(o) != r.len:
                raise batch.PgaError(f"export sink: a row of {r.len} letters was delivered {len(o)}")
        return out


def _order_arg(order, n):
    if order is None:
        return None
    order = list(order)
    if len(order) != n:
        raise ValueError("order: one entry per row")
    return (C.c_uint64 * max(n, 1))(*order)


def _rows(res, n, sink):
    R = res[:n]
    if sink is None:
        return [dict(status=r.status, len=r.len, seq=None) for r in R]
    seqs = sink.rows(R)
    return [dict(status=r.status, len=r.len, seq=s.decode("latin-1") if r.status == 0 else None) for r, s in zip(R, seqs)]


def block_sequences_packed(K, aligned=True, order=None, want_seqs=True, dll=None, sink=None):
    """the call itself over packed arrays (a reconstruct._Packed); sink: a Collector of the caller's (a test's) in place of a fresh one"""
    dll = dll or batch.lib()
    _bind(dll)
    R = (export_res_t * max(K.n_mem, 1))()
    sink = (sink or Collector()) if want_seqs else None
    rc = dll.pga_block_sequences(K.n_blocks, K.B, K.M, K.S, K.D, K.I, K.L, 1 if aligned else 0, _order_arg(order, K.n_mem), R, sink.fn if sink else None, None)
    if sink is not None and sink.error is not None:
        raise sink.error
    if rc != 0:
        raise batch.PgaError(dll.pga_last_error().decode())
    return _rows(R, K.n_mem, sink)


def block_sequences(blocks, aligned=True, order=None, want_seqs=True, dll=None):
    """export block-sequences: blocks as reconstruct takes them -> one dict per member in global member order (or, with `order`, still
    indexed by member: `order` only sets the order in which the rows are built and delivered): status (0 built, 3 a literal '-' in unaligned
    mode), len, seq (str; None unless want_seqs and status == 0).  aligned: Edit::apply_aligned (gaps, no insertions) instead of
    Edit::apply.  want_seqs=False: verdict mode, no letter leaves the device."""
    return block_sequences_packed(_Packed(blocks, []), aligned, order, want_seqs, dll)


def core_alignment_packed(K, member_path, n_paths, guide_path, guide_members, aligned=True, order=None, want_seqs=True, dll=None, sink=None):
    """the call itself: guide_members = [(global member index, reverse)]"""
    dll = dll or batch.lib()
    _bind(dll)
    R = (export_res_t * max(n_paths, 1))()
    MP = (C.c_uint32 * max(len(member_path), 1))(*member_path)
    N = (recon_node_t * max(len(guide_members), 1))()
    for k, (m, rev) in enumerate(guide_members):
        N[k].member = m; N[k].reverse = 1 if rev else 0
    core_p, n_core = C.POINTER(core_block_t)(), C.c_int64(0)
    sink = (sink or Collector()) if want_seqs else None
    rc = dll.pga_core_alignment(K.n_blocks, K.B, K.M, K.S, K.D, K.I, K.L, MP, n_paths, guide_path, len(guide_members), N, 1 if aligned else 0, _order_arg(order, n_paths),
                                R, C.byref(core_p), C.byref(n_core), sink.fn if sink else None, None)
    try:
        if sink is not None and sink.error is not None:
            raise sink.error
        if rc != 0:
            raise batch.PgaError(dll.pga_last_error().decode())
        core = [dict(block=c.block, reverse=bool(c.reverse), col=c.col, cons_len=c.cons_len) for c in core_p[:n_core.value]]
        return _rows(R, n_paths, sink), core
    finally:
        if core_p:
            dll.pga_free(C.cast(core_p, C.c_void_p))


def core_alignment(blocks, member_path, n_paths, guide_path, guide_nodes, aligned=True, order=None, want_seqs=True, dll=None):
    """export core-genome, in the arguments core_from_json returns: -> (rows, core); rows: one dict per path (status: 0 built, 2 a reverse
    piece with a letter the complement rejects, 3 a literal '-' in unaligned mode; len; seq as in block_sequences), core: the core blocks in
    guide order as dict(block, reverse, col, cons_len).  order: the order in which the rows are built and delivered (rows stay indexed by
    path).  A guide node that names no member of the graph is passed on as one (the call fails)."""
    K = _Packed(blocks, [])
    NONE = (1 << 64) - 1
    guide = [(K.mem_first[b] + m if 0 <= b < len(blocks) and 0 <= m < len(blocks[b]["members"]) else NONE, rev) for b, m, rev in guide_nodes]
    return core_alignment_packed(K, member_path, n_paths, guide_path, guide, aligned, order, want_seqs, dll)


def core_from_json(g, guide_name):
    """a pangraph JSON (as reconstruct.graph_from_json takes it) and the guide strain's name -> (args, keys, in_record_order): args, a
    dict: blocks as reconstruct takes them, member_path[m] = the path index of global member m, n_paths, guide_path = the guide's path
    index, guide_nodes = its nodes in path.nodes order as (block index, member index inside the block, reverse); keys[p], the record key of path p (its
    name, or its id as a string: pangraph_block.rs:170); in_record_order(rows), the rows as the reference emits its records: sorted by key
    (concatenate_records collects them in a BTreeMap<String, _>; equal keys stay in path order here, merging them is the caller's)."""
    if isinstance(g, str):
        import gzip
        import json
        with (gzip.open(g, "rt") if g.endswith(".gz") else open(g)) as f:
            g = json.load(f)
    blocks, paths, names = graph_from_json(g)
    path_ids = sorted(g["paths"], key=int)
    keys = [n if n is not None else str(int(pid)) for n, pid in zip(names, path_ids)]
    member_path = [None] * sum(len(b["members"]) for b in blocks)
    first = [0]
    for b in blocks:
        first.append(first[-1] + len(b["members"]))
    for p, path in enumerate(paths):
        for blk, mem, _ in path["nodes"]:
            member_path[first[blk] + mem] = p
    if None in member_path:
        raise ValueError("a block member that no path visits")
    if guide_name not in names:
        raise KeyError(f"path {guide_name!r} not found in graph")       # (path_id_by_name, pangraph.rs:258-268)
    guide = names.index(guide_name)
    args = dict(blocks=blocks, member_path=member_path, n_paths=len(paths), guide_path=guide, guide_nodes=list(paths[guide]["nodes"]))

    def in_record_order(rows):
        return [rows[p] for p in sorted(range(len(keys)), key=lambda p: keys[p].encode())]
    return args, keys, in_record_order


def core_records(g, guide_name, aligned=True, dll=None):
    """export core-genome of a pangraph JSON as the reference writes it: a generator of (key, seq) in the reference's record order (sorted by
    key).  Raises ValueError where two paths share a key (the reference joins their rows; that is the caller's job here) and
    batch.PgaError where a row cannot be built -- found out in verdict mode, before anything is yielded (the reference's export returns Err
    and writes nothing)."""
    args, keys, _ = core_from_json(g, guide_name)
    if len(set(keys)) != len(keys):
        raise ValueError("two paths share a record key")
    order = sorted(range(len(keys)), key=lambda p: keys[p].encode())
    verdict, _ = core_alignment(aligned=aligned, order=order, want_seqs=False, dll=dll, **args)
    bad = [keys[p] for p, r in enumerate(verdict) if r["status"] != 0]
    if bad:
        raise batch.PgaError(f"core alignment: {len(bad)} rows cannot be built (first: {bad[0]!r}, status {verdict[keys.index(bad[0])]['status']})")

    def records():
        rows, _ = core_alignment(aligned=aligned, order=order, dll=dll, **args)
        for p in order:
            yield keys[p], rows[p]["seq"]
    return records()
