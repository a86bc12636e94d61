"""Python host mirror of the reconstruct entry: `pga_reconstruct` (include/pga_align.h) replaces reconstruct (packages/pangraph/src/commands/
reconstruct/reconstruct_run.rs:56-127) for all paths of a graph -- blocks with their members' edit lists and the node chains of the paths in,
every path's sequence out (write mode) or only whether it is the expected one (verify mode: the comparison runs on the device).  ctypes
only; the HIP library does the work."""
import ctypes as C
import gzip
import json

from . import batch
from .mapvar import del_t, ins_t, sub_t
from .reconsensus import rc_block_t, rc_member_t

TILE = 4096          # letters one workgroup of k_rows writes (256 threads x 16 letters, pga_rows.h)
LETTERS = 16         # letters one thread writes; every path starts at a multiple of it in the output


class recon_path_t(C.Structure):
    _fields_ = [("tot_len", C.c_uint64), ("first_pos", C.c_uint64), ("n_nodes", C.c_uint32), ("pad", C.c_uint32)]


class recon_node_t(C.Structure):
    _fields_ = [("member", C.c_uint64), ("reverse", C.c_int32), ("pad", C.c_int32)]


class recon_res_t(C.Structure):
    _fields_ = [("status", C.c_int32), ("pad", C.c_int32), ("len", C.c_uint64), ("seq_off", C.c_uint64), ("first_mismatch", C.c_int64), ("n_mismatch", C.c_int64)]


def _bytes(s):
    return s if isinstance(s, (bytes, bytearray)) else s.encode()


class _Packed:
    """the C arrays of a graph; keeps every buffer alive"""

    def __init__(self, blocks, paths):
        nb = len(blocks)
        self.n_blocks, self.n_paths = nb, len(paths)
        self.cons = [_bytes(b["consensus"]) for b in blocks]
        self.mem_first = [0]
        for b in blocks:
            self.mem_first.append(self.mem_first[-1] + len(b["members"]))
        self.n_mem = self.mem_first[-1]
        self.B = (rc_block_t * max(nb, 1))()
        self.M = (rc_member_t * max(self.n_mem, 1))()
        subs, dels, inss, letters = [], [], [], bytearray()
        m = 0
        for i, b in enumerate(blocks):
            self.B[i].consensus = self.cons[i]; self.B[i].cons_len = len(self.cons[i]); self.B[i].n_members = len(b["members"])
            for e in b["members"]:
                self.M[m].n_subs = len(e["subs"]); self.M[m].n_dels = len(e["dels"]); self.M[m].n_inss = len(e["inss"])
                subs += [(pos, ord(a)) for pos, a in e["subs"]]
                dels += list(e["dels"])
                for pos, seq in e["inss"]:
                    inss.append((pos, len(seq), len(letters)))
                    letters += _bytes(seq)
                m += 1
        self.S = (sub_t * max(len(subs), 1))(*[sub_t(*x) for x in subs])
        self.D = (del_t * max(len(dels), 1))(*[del_t(*x) for x in dels])
        self.I = (ins_t * max(len(inss), 1))(*[ins_t(*x) for x in inss])
        self.L = C.create_string_buffer(bytes(letters), max(len(letters), 1))
        self.n_nodes = sum(len(p["nodes"]) for p in paths)
        self.P = (recon_path_t * max(len(paths), 1))()
        self.N = (recon_node_t * max(self.n_nodes, 1))()
        k = 0
        for i, p in enumerate(paths):
            self.P[i].tot_len = p["tot_len"]; self.P[i].first_pos = p["first_pos"]; self.P[i].n_nodes = len(p["nodes"])
            for blk, mem, reverse in p["nodes"]:
                self.N[k].member = self.mem_first[blk] + mem; self.N[k].reverse = 1 if reverse else 0
                k += 1

    def args(self):
        return (self.n_blocks, self.B, self.M, self.S, self.D, self.I, self.L, self.n_paths, self.P, self.N)


def _bind(dll):
    dll.pga_reconstruct.restype = C.c_int
    dll.pga_reconstruct.argtypes = [C.c_int64] + [C.c_void_p] * 6 + [C.c_int64] + [C.c_void_p] * 5 + [C.POINTER(C.POINTER(C.c_char))]
    dll.pga_last_error.restype = C.c_char_p
    dll.pga_free.argtypes = [C.c_void_p]


def reconstruct_packed(K, expected=None, want_seqs=True, dll=None, expected_len=None):
    """the call itself over packed arrays (a _Packed, which a test may have altered); expected_len overrides the lengths of `expected`,
    an entry None of `expected` is passed as a NULL pointer"""
    dll = dll or batch.lib()
    _bind(dll)
    n = max(K.n_paths, 1)
    R = (recon_res_t * n)()
    exp_p = exp_n = keep = None
    if expected is not None:
        assert len(expected) == K.n_paths
        keep = [None if s is None else _bytes(s) for s in expected]
        exp_p = (C.c_char_p * n)(*keep)
        exp_n = (C.c_uint64 * n)(*(expected_len if expected_len is not None else [0 if s is None else len(s) for s in keep]))
    out = C.POINTER(C.c_char)()
    if dll.pga_reconstruct(*K.args(), exp_p, exp_n, R, C.byref(out) if want_seqs else None) != 0:
        raise batch.PgaError(dll.pga_last_error().decode())
    try:
        base = C.addressof(out.contents) if want_seqs and out else 0
        return [dict(status=r.status, len=r.len, seq=C.string_at(base + r.seq_off, r.len).decode() if want_seqs and r.status == 0 else None,
                     first_mismatch=r.first_mismatch, n_mismatch=r.n_mismatch) for r in R[:K.n_paths]]
    finally:
        if want_seqs and out:
            dll.pga_free(C.cast(out, C.c_void_p))


def reconstruct(blocks, paths, expected=None, want_seqs=True, dll=None):
    """blocks: [{"consensus": str, "members": [edit, ...]}] with edit = {"subs": [(pos, letter)], "dels": [(pos, len)], "inss": [(pos, seq)]},
    blocks and members in the reference's BTreeMap order; paths: [{"nodes": [(block index, member index inside the block, reverse), ...] in
    path.nodes order, "tot_len": int, "first_pos": position().0 of the first node}].  expected: one sequence (str or bytes) per path, or None
    (no verify mode); want_seqs: write mode.  -> one dict per path: status, len, seq (str; None unless want_seqs and status == 0),
    first_mismatch, n_mismatch."""
    return reconstruct_packed(_Packed(blocks, paths), expected, want_seqs, dll)


def graph_from_json(g):
    """a pangraph JSON (a file name, .gz or not, or the parsed object with `paths` / `blocks` / `nodes`) -> (blocks, paths, names) as
    reconstruct takes them: blocks in BlockId order, the members of a block in NodeId order (PangraphBlock::alignments(), a BTreeMap), paths
    in PathId order (reconstruct_run.rs:60), nodes in path.nodes order, first_pos = position[0] of the path's first node"""
    if isinstance(g, str):
        with (gzip.open(g, "rt") if g.endswith(".gz") else open(g)) as f:
            g = json.load(f)
    block_ids = sorted(g["blocks"], key=int)
    block_at = {int(b): i for i, b in enumerate(block_ids)}
    blocks, member_at = [], {}
    for i, b in enumerate(block_ids):
        blk = g["blocks"][b]
        members = []
        for j, nid in enumerate(sorted(blk["alignments"], key=int)):
            e = blk["alignments"][nid]
            member_at[int(nid)] = (i, j)
            members.append({"subs": [(x["pos"], x["alt"]) for x in e["subs"]], "dels": [(x["pos"], x["len"]) for x in e["dels"]],
                            "inss": [(x["pos"], x["seq"]) for x in e["inss"]]})
        blocks.append({"consensus": blk["consensus"], "members": members})
    nodes = {int(k): v for k, v in g["nodes"].items()}
    paths, names = [], []
    for pid in sorted(g["paths"], key=int):
        p = g["paths"][pid]
        chain = []
        for nid in p["nodes"]:
            node = nodes[int(nid)]
            blk, mem = member_at[int(nid)]
            assert blk == block_at[int(node["block_id"])]
            chain.append((blk, mem, node["strand"] == "-"))
        paths.append({"nodes": chain, "tot_len": p["tot_len"], "first_pos": nodes[int(p["nodes"][0])]["position"][0] if p["nodes"] else 0})
        names.append(p.get("name"))
    return blocks, paths, names
