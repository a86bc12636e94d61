"""The pangraph JSON on the device: `pga_export_json` (include/pga_align.h, pga_json.hip) formats the file that `pangraph build` and
`pangraph simplify` write (serde_json::to_writer_pretty of Pangraph: build_run.rs:78, simplify_run.rs:20) from the flat graph of
pangraph_amd/topology.py and the block arrays of pangraph_amd/reconstruct.py, streamed to a sink in tiles.  ctypes only; the HIP library does
the work.  `json_write_str` is the pure-Python restatement: dicts in the reference's key order through json.dumps(indent=2,
ensure_ascii=False), which reproduces the reference's own file byte for byte (tests/golden/plasmids.json.gz): the host fallback and the
expectation of the tests.

The graph arguments may be a PlanOut's / RemoveOut's graph_args() or the apply output, the block arguments a RemoveOut's block_args() or
a _Packed's args()[:7], by pointer: a build or simplify that keeps its graph flat ends in its JSON without rebuilding the host dictionaries."""
import ctypes as C
import json
import struct

from . import batch
from .gfa import SINK, _load
from .mapvar import del_t, ins_t, sub_t
from .reconsensus import rc_block_t, rc_member_t
from .topology import pack_lists

U64_MAX = (1 << 64) - 1
EMPTY = b'{\n  "paths": {},\n  "blocks": {},\n  "nodes": {}\n}'


class json_out_t(C.Structure):
    _fields_ = [("n_bytes", C.c_uint64), ("section_off", C.c_uint64 * 3), ("n_paths", C.c_int64), ("n_blocks", C.c_int64), ("n_nodes", C.c_int64),
                ("path_off", C.POINTER(C.c_uint64)), ("block_off", C.POINTER(C.c_uint64)), ("node_order", C.POINTER(C.c_uint32))]


def _bind(dll):
    dll.pga_export_json.restype = C.c_int
    dll.pga_export_json.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p] + [C.c_void_p] * 6 + [C.c_uint64] + [C.c_void_p] * 5 + \
                                   [C.c_uint32, C.POINTER(json_out_t), C.c_void_p, C.c_void_p]
    dll.pga_json_free.restype = None
    dll.pga_json_free.argtypes = [C.POINTER(json_out_t)]
    dll.pga_json_last_ms.restype = None
    dll.pga_json_last_ms.argtypes = [C.POINTER(C.c_double)]
    dll.pga_last_error.restype = C.c_char_p


# ---------------------------------------------------------------- the restatement of the reference
def ordered(g):
    """a pangraph JSON (a file name, or the parsed object) -> the same graph as dicts in the reference's order: the three maps by ascending
    id (BTreeMap), every struct in its field order, every number a Python int"""
    g = _load(g)
    by_id = lambda d: sorted(d, key=int)
    edit = lambda e: {"subs": [{"pos": int(x["pos"]), "alt": x["alt"]} for x in e["subs"]], "dels": [{"pos": int(x["pos"]), "len": int(x["len"])} for x in e["dels"]],
                      "inss": [{"pos": int(x["pos"]), "seq": x["seq"]} for x in e["inss"]]}
    paths = {str(int(k)): {"id": int(k), "nodes": [int(n) for n in g["paths"][k]["nodes"]], "tot_len": int(g["paths"][k]["tot_len"]), "circular": bool(g["paths"][k]["circular"]),
                           "name": g["paths"][k].get("name"), "desc": g["paths"][k].get("desc")} for k in by_id(g["paths"])}
    blocks = {str(int(k)): {"id": int(k), "consensus": g["blocks"][k]["consensus"],
                            "alignments": {str(int(n)): edit(g["blocks"][k]["alignments"][n]) for n in by_id(g["blocks"][k]["alignments"])}} for k in by_id(g["blocks"])}
    nodes = {str(int(k)): {"id": int(k), "block_id": int(g["nodes"][k]["block_id"]), "path_id": int(g["nodes"][k]["path_id"]), "strand": g["nodes"][k]["strand"],
                           "position": [int(g["nodes"][k]["position"][0]), int(g["nodes"][k]["position"][1])]} for k in by_id(g["nodes"])}
    return {"paths": paths, "blocks": blocks, "nodes": nodes}


def json_write_str(g):
    """serde_json::to_writer_pretty(&Pangraph) on a pangraph JSON -> bytes (UTF-8, no trailing newline)"""
    return json.dumps(ordered(g), indent=2, ensure_ascii=False).encode()


def json_tables(g):
    """-> {"text", "section_off": the opening quotes of "paths", "blocks", "nodes", "path_off" / "block_off": the opening quote of every
    path's / block's key in ascending id, "node_order": the positions (the nodes path after path, paths in ascending id) by ascending node id}"""
    o = ordered(g)
    text = json_write_str(o)
    off, at = {}, 0
    for sec in ("paths", "blocks", "nodes"):
        at = text.index(b'\n  "%s": {' % sec.encode(), at) + 3
        off[sec] = [at]
        if sec != "nodes":
            for k in o[sec]:                                                  # (a line indented by four starts with a key of the section and with nothing else)
                at = text.index(b'\n    "%s": {' % k.encode(), at) + 5
                off[sec].append(at)
    ids = [n for p in o["paths"].values() for n in p["nodes"]]
    return {"text": text, "section_off": [off[s][0] for s in ("paths", "blocks", "nodes")], "path_off": off["paths"][1:], "block_off": off["blocks"][1:],
            "node_order": sorted(range(len(ids)), key=ids.__getitem__)}


# ---------------------------------------------------------------- the arrays of the call
class Flat:
    """the C arrays of one graph: graph_args (the six of pga_plan_simplify), block_args (the seven of pga_reconstruct), path_meta
    [(tot_len, name, desc)] with bytes or None; keeps every buffer alive"""

    def __init__(self, blocks, paths, nodes, cons, members, ins_seq, path_meta):
        """blocks, paths, nodes: the lists of topology.pack_lists; cons: per block bytes (None for a dead one); members: per block its slots in
        member order, each {"subs": [(pos, alt)], "dels": [(pos, len)], "inss": [(pos, len, seq_off)]} with alt a byte value (dead blocks: []);
        ins_seq: the insertion letters"""
        self.graph_args = pack_lists(blocks, paths, nodes)
        nb = len(blocks)
        self.cons = [None if c is None else bytes(c) for c in cons]
        self.B = (rc_block_t * max(nb, 1))()
        for i, b in enumerate(blocks):
            self.B[i].consensus = self.cons[i]; self.B[i].cons_len = b[1]; self.B[i].n_members = len(members[i])
        flat = [e for m in members for e in m]
        self.M = (rc_member_t * max(len(flat), 1))(*[rc_member_t(len(e["subs"]), len(e["dels"]), len(e["inss"])) for e in flat])
        pack = lambda fmt, ct, rows: (ct * max(len(rows), 1)).from_buffer_copy(b"".join(struct.pack(fmt, *r) for r in rows) or bytes(C.sizeof(ct)))
        self.S = pack("<II", sub_t, [x for e in flat for x in e["subs"]])
        self.D = pack("<II", del_t, [x for e in flat for x in e["dels"]])
        self.I = pack("<IIQ", ins_t, [x for e in flat for x in e["inss"]])
        self.L = C.create_string_buffer(bytes(ins_seq), max(len(ins_seq), 1))
        self.ins_seq_len = len(ins_seq)
        self.block_args = (nb, self.B, self.M, self.S, self.D, self.I, self.L)
        self.path_meta = list(path_meta)


def json_from_json(g):
    """a pangraph JSON (a file name, or the parsed object) -> Flat: blocks in ascending id, the member slots of a block its alignments in
    ascending node id (the order of gfa.lists_from_json and reconstruct.graph_from_json), paths in ascending id"""
    o = ordered(g)
    bids = list(o["blocks"])
    at = {b: i for i, b in enumerate(bids)}
    slot = {n: k for b in bids for k, n in enumerate(o["blocks"][b]["alignments"])}
    blocks = [(int(b), len(o["blocks"][b]["consensus"].encode()), len(o["blocks"][b]["alignments"]), 1) for b in bids]
    letters, members = bytearray(), []
    for b in bids:
        members.append([])
        for e in o["blocks"][b]["alignments"].values():
            inss = []
            for x in e["inss"]:
                seq = x["seq"].encode()
                inss.append((x["pos"], len(seq), len(letters)))
                letters += seq
            members[-1].append({"subs": [(x["pos"], ord(x["alt"])) for x in e["subs"]], "dels": [(x["pos"], x["len"]) for x in e["dels"]], "inss": inss})
    paths, nodes, meta = [], [], []
    enc = lambda s: None if s is None else s.encode()
    for pid, p in o["paths"].items():
        paths.append((int(pid), len(nodes), len(p["nodes"]), 1 if p["circular"] else 0))
        meta.append((p["tot_len"], enc(p["name"]), enc(p["desc"])))
        for nid in p["nodes"]:
            n = o["nodes"][str(nid)]
            nodes.append((nid, n["position"][0], n["position"][1], at[str(n["block_id"])], slot[str(nid)], n["strand"] == "-"))
    return Flat(blocks, paths, nodes, [o["blocks"][b]["consensus"].encode() for b in bids], members, letters, meta)


def _ptr(p):
    return C.cast(p, C.c_void_p) if p is not None and not isinstance(p, int) else p


class JsonOut:
    """the tables of one call; owns its arrays until free()"""

    def __init__(self, dll, out, keep_alive):
        self.dll, self.out, self.keep_alive, self.n_bytes, self.section_off = dll, out, keep_alive, out.n_bytes, list(out.section_off)

    def path_off(self):
        return self.out.path_off[:self.out.n_paths] if self.out.n_paths else []

    def block_off(self):
        """per block index; U64_MAX for a dead block"""
        return self.out.block_off[:self.out.n_blocks] if self.out.n_blocks else []

    def node_order(self):
        return self.out.node_order[:self.out.n_nodes] if self.out.n_nodes else []

    def free(self):
        if self.out is not None:
            self.dll.pga_json_free(C.byref(self.out))
            self.out = None


def marshal(graph_args, block_args, path_meta, ins_seq_len=None):
    """-> (the first eighteen arguments of pga_export_json, what must stay alive): the consensus pointers read off rc_blocks, the path
    records as five arrays"""
    nb, rc_blocks, members, subs, dels, inss, ins_seq = block_args
    if nb != graph_args[0]:
        raise ValueError("the graph and the block arrays differ in their number of blocks")
    if len(path_meta) != graph_args[2]:
        raise ValueError(f"{len(path_meta)} entries for {graph_args[2]} paths")
    if ins_seq_len is None:
        if ins_seq is not None and not isinstance(ins_seq, C.Array):
            raise ValueError("ins_seq_len is needed with insertion letters given by pointer")
        ins_seq_len = C.sizeof(ins_seq) if ins_seq is not None else 0
    R = C.cast(rc_blocks, C.POINTER(rc_block_t)) if rc_blocks is not None else None
    cons = (C.c_void_p * max(nb, 1))(*[C.c_void_p.from_address(C.addressof(R[b])).value for b in range(nb)]) if R else None   # (the consensus pointers, not the letters)
    n = max(len(path_meta), 1)
    text = lambda s: None if s is None else (s.encode() if isinstance(s, str) else bytes(s))
    keep_n, keep_d = [text(m[1]) for m in path_meta], [text(m[2]) for m in path_meta]
    tot = (C.c_uint64 * n)(*[m[0] for m in path_meta])
    names, descs = (C.c_char_p * n)(*keep_n), (C.c_char_p * n)(*keep_d)
    name_len, desc_len = (C.c_uint32 * n)(*[len(x) if x is not None else 0 for x in keep_n]), (C.c_uint32 * n)(*[len(x) if x is not None else 0 for x in keep_d])
    args = [_ptr(a) for a in graph_args] + [_ptr(cons), _ptr(members), _ptr(subs), _ptr(dels), _ptr(inss), _ptr(ins_seq), ins_seq_len, _ptr(tot), _ptr(names), _ptr(name_len),
                                            _ptr(descs), _ptr(desc_len)]
    return args, (graph_args, block_args, keep_n, keep_d, cons, tot, names, descs, name_len, desc_len)


def export_json_raw(graph_args, block_args, path_meta, sink=None, ins_seq_len=None, flags=0, dll=None):
    """graph_args: (n_blocks, blocks, n_paths, paths, n_nodes, nodes) and block_args: (n_blocks, rc_blocks, members, subs, dels, inss, ins_seq)
    as C arrays or pointers (a Flat's, or the graph_args() / block_args() of a RemoveOut, a PlanOut, the apply output); path_meta: per path
    (tot_len, name, desc), name and desc bytes or None (JSON null); ins_seq_len: the letters at ins_seq (taken from a C array's size when
    absent); sink: None (verdict mode: the tables and n_bytes) or a callable taking one piece of the file as bytes -- a true return value
    stops the export, an exception too (raised again here) -> JsonOut"""
    dll = dll or batch.lib()
    _bind(dll)
    args, keep = marshal(graph_args, block_args, path_meta, ins_seq_len)
    raised = []

    def on_piece(_, at, n_):
        try:
            return 1 if sink(C.string_at(at, n_)) else 0
        except BaseException as e:                                           # (never through the C frames)
            raised.append(e)
            return 1
    cb = SINK(on_piece) if sink is not None else None
    out = json_out_t()
    rc = dll.pga_export_json(*args, flags, C.byref(out), C.cast(cb, C.c_void_p) if cb is not None else None, None)
    if raised:
        raise raised[0]
    if rc != 0:
        raise batch.PgaError(dll.pga_last_error().decode())
    return JsonOut(dll, out, keep)


def last_ms(dll=None):
    """(tables, tile kernels, host copies, sink) of the calling thread's last call, in ms (measurement only)"""
    dll = dll or batch.lib()
    _bind(dll)
    ms = (C.c_double * 4)()
    dll.pga_json_last_ms(ms)
    return tuple(ms)


def export_json(g, dll=None):
    """a pangraph JSON (a file name, or the parsed object) -> the file as the reference writes it, as bytes"""
    F = json_from_json(g)
    pieces = []
    export_json_raw(F.graph_args, F.block_args, F.path_meta, pieces.append, F.ins_seq_len, dll=dll).free()
    return b"".join(pieces)


def write_json(g, path_or_file, dll=None):
    """streams the file tile by tile into a file name or a binary file object; the tiles are never joined -> the number of bytes written"""
    F = json_from_json(g)
    f = open(path_or_file, "wb") if isinstance(path_or_file, (str, bytes)) or hasattr(path_or_file, "__fspath__") else path_or_file
    try:
        out = export_json_raw(F.graph_args, F.block_args, F.path_meta, lambda piece: f.write(piece) and None, F.ins_seq_len, dll=dll)
        n = out.n_bytes
        out.free()
        return n
    finally:
        if f is not path_or_file:
            f.close()
