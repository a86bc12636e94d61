"""`pangraph export gfa` on the device: `pga_export_gfa` (include/pga_align.h, pga_gfa.hip) builds the tables of the file (segments, links,
paths, steps) and formats its text from the flat graph of pangraph_amd/topology.py, streamed to a sink in tiles.  ctypes only; the HIP
library does the work.  `gfa_write_str` is the pure-Python restatement of the reference (io/gfa.rs:79-279 gfa_write, Edge of
circularize/circularize_utils.rs:46-102): the host fallback and the expectation of the tests.

The six graph arguments may be a PlanOut's / RemoveOut's graph_args() or the apply output, by pointer: a build or simplify that keeps its
graph flat ends in a GFA file without rebuilding the host dictionaries."""
import ctypes as C
import gzip
import json

from . import batch
from .topology import pack_lists, topo_edge_t

STEPS = 1                            # PGA_GFA_STEPS
U64_MAX = (1 << 64) - 1
HEADER = b"H\tVN:Z:1.0\n"


class gfa_params_t(C.Structure):
    _fields_ = [("min_len", C.c_uint64), ("max_len", C.c_uint64), ("min_depth", C.c_uint64), ("max_depth", C.c_uint64), ("no_duplicated", C.c_int32),
                ("include_sequences", C.c_int32)]


class gfa_segment_t(C.Structure):
    _fields_ = [("block", C.c_uint32), ("depth", C.c_uint32), ("cons_len", C.c_uint32), ("duplicated", C.c_int32), ("byte_off", C.c_uint64)]


class gfa_path_t(C.Structure):
    _fields_ = [("path", C.c_uint32), ("n_steps", C.c_uint32), ("step_off", C.c_uint64), ("byte_off", C.c_uint64)]


class gfa_step_t(C.Structure):
    _fields_ = [("block", C.c_uint32), ("reverse", C.c_int32)]


class gfa_out_t(C.Structure):
    _fields_ = [("n_segments", C.c_int64), ("n_links", C.c_int64), ("n_paths", C.c_int64), ("n_steps", C.c_int64), ("n_bytes", C.c_uint64),
                ("segments", C.POINTER(gfa_segment_t)), ("links", C.POINTER(topo_edge_t)), ("paths", C.POINTER(gfa_path_t)), ("steps", C.POINTER(gfa_step_t))]


SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)


class GfaParams:
    """GfaWriteParams (gfa.rs:14-39): absent bounds are None"""

    def __init__(self, minimum_length=None, maximum_length=None, minimum_depth=None, maximum_depth=None, include_sequences=False, no_duplicated=False):
        self.minimum_length, self.maximum_length, self.minimum_depth, self.maximum_depth = minimum_length, maximum_length, minimum_depth, maximum_depth
        self.include_sequences, self.no_duplicated = bool(include_sequences), bool(no_duplicated)

    def bounds(self):
        """(min_len, max_len, min_depth, max_depth) with 0 and 2^64 - 1 for the absent ones (gfa.rs:42-56)"""
        d = lambda v, x: x if v is None else v
        return d(self.minimum_length, 0), d(self.maximum_length, U64_MAX), d(self.minimum_depth, 0), d(self.maximum_depth, U64_MAX)

    def to_c(self):
        return gfa_params_t(*self.bounds(), 1 if self.no_duplicated else 0, 1 if self.include_sequences else 0)


def _bind(dll):
    dll.pga_export_gfa.restype = C.c_int
    dll.pga_export_gfa.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                   C.POINTER(gfa_out_t), C.c_void_p, C.c_void_p]
    dll.pga_gfa_free.restype = None
    dll.pga_gfa_free.argtypes = [C.POINTER(gfa_out_t)]
    dll.pga_last_error.restype = C.c_char_p


# ---------------------------------------------------------------- the restatement of the reference
def _conventional(e):
    """Edge::conventional_orientation on ((block, strand), (block, strand)), strand 0 forward (circularize_utils.rs:65-71)"""
    (b1, s1), (b2, s2) = e
    return e if b1 < b2 or (b1 == b2 and s1 == 0) else ((b2, s2 ^ 1), (b1, s1 ^ 1))


def gfa_tables(blocks, paths, nodes, params, cons=None, names=None):
    """the flat lists of topology.pack_lists (blocks in ascending id, so that index order is id order), cons: per block bytes or None, names:
    per path bytes -> {"segments": [(block, depth, cons_len, duplicated, byte_off)], "links": [(b1, b2, s1, s2, count)], "paths": [(path,
    n_steps, step_off, byte_off)], "steps": [(block, reverse)], "text": bytes}: convert_pangraph_to_gfa and gfa_write on block indices"""
    params = params or GfaParams()
    lo_len, hi_len, lo_depth, hi_depth = params.bounds()
    dup = [False] * len(blocks)
    for _, off, n, _ in paths:                                               # PangraphBlock::is_duplicated, on the unfiltered graph
        seen = set()
        for x in nodes[off:off + n]:
            if x[3] in seen:
                dup[x[3]] = True
            seen.add(x[3])
    ok = [bool(b[3]) and lo_len <= b[1] <= hi_len and lo_depth <= b[2] <= hi_depth and not (params.no_duplicated and dup[i]) for i, b in enumerate(blocks)]
    steps, out_paths, count = [], [], {}
    for k, (_, off, n, circular) in enumerate(paths):                        # gfa_filter_path; paths left empty are dropped
        kept = [(x[3], 1 if x[5] else 0) for x in nodes[off:off + n] if ok[x[3]]]
        if not kept:
            continue
        out_paths.append((k, len(kept), len(steps)))
        steps += kept
        for e in list(zip(kept, kept[1:])) + ([(kept[-1], kept[0])] if circular else []):   # gfa_paths_to_links
            e = _conventional(e)
            count[e] = count.get(e, 0) + 1
    links = [(b1, b2, s1, s2, c) for ((b1, s1), (b2, s2)), c in sorted(count.items(), key=lambda kv: (kv[0][0][0], kv[0][1][0], kv[0][0][1], kv[0][1][1]))]
    used = sorted({b for b, _ in steps})
    out, at, segments, path_rows = [HEADER], len(HEADER), [], []
    put = lambda line: (out.append(line), len(line))[1]
    if used:
        at += put(b"# blocks\n")
    for b in used:
        bid, length, depth, _ = blocks[b]
        seq = (cons[b] if length else b"") if params.include_sequences else b"*"
        if params.include_sequences and len(seq) != length:
            raise ValueError(f"the consensus of block {bid} does not have its length")
        segments.append((b, depth, length, 1 if dup[b] else 0, at))
        at += put(b"S\t%d\t%s\tRC:i:%d\tLN:i:%d%s\n" % (bid, seq, depth * length, length, b"\tTP:Z:duplicated" if dup[b] else b""))
    if links:
        at += put(b"# edges\n")
    for b1, b2, s1, s2, c in links:
        at += put(b"L\t%d\t%s\t%d\t%s\t*\tRC:i:%d\n" % (blocks[b1][0], b"-" if s1 else b"+", blocks[b2][0], b"-" if s2 else b"+", c))
    if out_paths:
        at += put(b"# paths\n")
    ids = [b"%d" % b[0] for b in blocks]
    for k, n, so in out_paths:
        if names is None or names[k] is None:
            raise ValueError(f"path {paths[k][0]} has no name")
        path_rows.append((k, n, so, at))
        at += put(b"P\t%s\t%s\t*%s\n" % (names[k], b",".join(ids[b] + (b"-" if r else b"+") for b, r in steps[so:so + n]), b"\tTP:Z:circular" if paths[k][3] else b""))
    return {"segments": segments, "links": links, "paths": path_rows, "steps": steps, "text": b"".join(out)}


def _load(g):
    if isinstance(g, str):
        with (gzip.open(g, "rt") if g.endswith(".gz") else open(g)) as f:
            g = json.load(f)
    return g


def lists_from_json(g):
    """a pangraph JSON (a file name, or the parsed object) -> (blocks, paths, nodes, cons, names): the lists of topology.pack_lists -- blocks
    in ascending id, the member slots of a block its alignments in ascending node id (as reconstruct.graph_from_json orders members), paths in
    ascending id -- the consensus of every block and the name of every path as bytes (None for a path without a name)"""
    g = _load(g)
    bids = sorted(g["blocks"], key=int)
    at = {int(b): i for i, b in enumerate(bids)}
    slot = {int(n): k for b in bids for k, n in enumerate(sorted(g["blocks"][b]["alignments"], key=int))}
    blocks = [(int(b), len(g["blocks"][b]["consensus"]), len(g["blocks"][b]["alignments"]), 1) for b in bids]
    cons = [g["blocks"][b]["consensus"].encode() for b in bids]
    node_of = {int(k): v for k, v in g["nodes"].items()}
    paths, nodes, names = [], [], []
    for pid in sorted(g["paths"], key=int):
        p = g["paths"][pid]
        paths.append((int(pid), len(nodes), len(p["nodes"]), 1 if p["circular"] else 0))
        name = p.get("name")
        names.append(None if name is None else name.encode())
        for nid in p["nodes"]:
            n = node_of[int(nid)]
            nodes.append((int(nid), n["position"][0], n["position"][1], at[int(n["block_id"])], slot[int(nid)], n["strand"] == "-"))
    return blocks, paths, nodes, cons, names


def gfa_write_str(g, params=None):
    """gfa_write_str of the reference (gfa.rs:73-77) on a pangraph JSON -> bytes.  ValueError where the reference unwraps a missing path
    name (gfa.rs:231: every path of the graph, emitted or not)"""
    blocks, paths, nodes, cons, names = lists_from_json(g)
    for p, name in zip(paths, names):
        if name is None:
            raise ValueError(f"path {p[0]} has no name")
    return gfa_tables(blocks, paths, nodes, params, cons, names)["text"]


# ---------------------------------------------------------------- the call
def gfa_from_json(g):
    """-> (graph_args, cons, names): the six graph arguments of pga_export_gfa (pack_lists), the consensus of every block and the name of
    every path as bytes"""
    blocks, paths, nodes, cons, names = lists_from_json(g)
    return pack_lists(blocks, paths, nodes), cons, names


def _ptr(p):
    return C.cast(p, C.c_void_p) if p is not None and not isinstance(p, int) else p


class GfaOut:
    """the tables of one call; owns its arrays until free()"""

    def __init__(self, dll, out, keep_alive):
        self.dll, self.out, self.keep_alive, self.n_bytes, self.n_steps = dll, out, keep_alive, out.n_bytes, out.n_steps

    def segments(self):
        o = self.out
        return [(s.block, s.depth, s.cons_len, s.duplicated, s.byte_off) for s in (o.segments[i] for i in range(o.n_segments))]

    def links(self):
        o = self.out
        return [(e.b1, e.b2, e.s1, e.s2, e.count) for e in (o.links[i] for i in range(o.n_links))]

    def paths(self):
        o = self.out
        return [(p.path, p.n_steps, p.step_off, p.byte_off) for p in (o.paths[i] for i in range(o.n_paths))]

    def steps(self):
        """[(block, reverse)], or None when the call was made without steps=True"""
        o = self.out
        if not o.steps:
            return None
        return [(s.block, s.reverse) for s in (o.steps[i] for i in range(o.n_steps))]

    def free(self):
        if self.out is not None:
            self.dll.pga_gfa_free(C.byref(self.out))
            self.out = None


def _bytes_array(items, n):
    """a list of bytes / None -> (char*[n], uint32[n], what must stay alive)"""
    if items is None:
        return None, None, None
    if len(items) != n:
        raise ValueError(f"{len(items)} entries for {n} blocks or paths")
    bufs = [None if x is None else (x.encode() if isinstance(x, str) else bytes(x)) for x in items]
    P = (C.c_char_p * max(n, 1))(*bufs)
    L = (C.c_uint32 * max(n, 1))(*[len(x) if x is not None else 0 for x in bufs])
    return P, L, bufs


def export_gfa_raw(graph_args, cons, names, params=None, sink=None, steps=False, dll=None):
    """graph_args: (n_blocks, blocks, n_paths, paths, n_nodes, nodes) as C arrays or pointers (topology.pack_lists, gfa_from_json, or the
    graph_args() of a PlanOut / RemoveOut / apply output); cons: per block bytes (None: no letters at hand), names: per path bytes;
    sink: None (verdict mode: the tables and n_bytes) or a callable taking one piece of the file as bytes -- a true return value stops the
    export, an exception too (raised again here) -> GfaOut"""
    dll = dll or batch.lib()
    _bind(dll)
    params = params or GfaParams()
    cons_p, _, keep_c = _bytes_array(cons, graph_args[0])
    names_p, names_l, keep_n = _bytes_array(names, graph_args[2])
    raised = []

    def on_piece(_, at, n):
        try:
            return 1 if sink(C.string_at(at, n)) else 0
        except BaseException as e:                                           # (never through the C frames)
            raised.append(e)
            return 1
    cb = SINK(on_piece) if sink is not None else None
    prm, out = params.to_c(), gfa_out_t()
    rc = dll.pga_export_gfa(*[_ptr(a) for a in graph_args], _ptr(cons_p), _ptr(names_p), _ptr(names_l), C.cast(C.byref(prm), C.c_void_p), STEPS if steps else 0,
                            C.byref(out), C.cast(cb, C.c_void_p) if cb is not None else None, None)
    if raised:
        raise raised[0]
    if rc != 0:
        raise batch.PgaError(dll.pga_last_error().decode())
    return GfaOut(dll, out, (graph_args, keep_c, keep_n, cons_p, names_p, names_l))


def _named(g):
    """gfa_from_json, with the ValueError of gfa_write_str for a path without a name"""
    args, cons, names = gfa_from_json(g)
    if any(n is None for n in names):
        raise ValueError("a path has no name")
    return args, cons, names


def export_gfa(g, params=None, dll=None):
    """a pangraph JSON (a file name, or the parsed object) -> the GFA file as bytes"""
    args, cons, names = _named(g)
    pieces = []
    export_gfa_raw(args, cons if (params and params.include_sequences) else None, names, params, pieces.append, dll=dll).free()
    return b"".join(pieces)


def write_gfa(g, path_or_file, params=None, dll=None):
    """streams the file tile by tile into a file name or a binary file object; the tiles are never joined -> the number of bytes written"""
    args, cons, names = _named(g)
    f = open(path_or_file, "wb") if isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, "__fspath__") else path_or_file
    try:
        out = export_gfa_raw(args, cons if (params and params.include_sequences) else None, names, params, lambda piece: f.write(piece) and None, dll=dll)
        n = out.n_bytes
        out.free()
        return n
    finally:
        if f is not path_or_file:
            f.close()
