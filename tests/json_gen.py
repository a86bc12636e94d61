"""Graphs for pga_export_json (pangraph_amd/jsonout.py, pga_json.hip): every named case is the smallest graph with its property and carries
a pin -- what tests/test_json_cpu.py holds against the host restatement (jsonout.json_tables) before tests/test_gpu_json.py relies on it --
and, where it is small, the text written out by hand.  A case is flat, as the entry takes it: {"blocks": [(block_id, cons_len, depth,
alive)], "cons": per block bytes (None for a dead entry), "paths": [(path_id, node_off, n_nodes, circular)], "nodes": [(node_id, pos0, pos1,
block, member, reverse)], "members": per block its slots in member order, each {"subs": [(pos, alt)], "dels": [(pos, len)], "inss": [(pos,
len, seq_off)]}, "ins_seq": bytes, "meta": [(tot_len, name, desc)] with bytes or None, "pin": exp -> truth, "text": bytes or None}.
to_json() is the pangraph JSON of a case, which the restatement prints.  The tile cases are made for PGA_EXPORT_TILE_KB=4."""
import ctypes as C
import functools
import hashlib
import random
import struct

import numpy as np

from pangraph_amd import jsonout

EDGE = 4096                              # PGA_EXPORT_TILE_KB=4
TILE = 1024                              # PGA_TOPO_TILE: the tile of the 64-bit scan
CHUNK = 64                               # JS_CHUNK: letters of an insertion per item
U64, U32 = (1 << 64) - 1, (1 << 32) - 1
NONE = {"subs": [], "dels": [], "inss": []}
NP_BLOCK = np.dtype([("block_id", "<u8"), ("cons_len", "<u4"), ("depth", "<u4"), ("alive", "<i4"), ("pad", "<i4")])
NP_PATH = np.dtype([("path_id", "<u8"), ("node_off", "<u8"), ("n_nodes", "<u4"), ("circular", "<i4")])
NP_NODE = np.dtype([("node_id", "<u8"), ("pos0", "<u8"), ("pos1", "<u8"), ("block", "<u4"), ("member", "<u4"), ("reverse", "<i4"), ("pad", "<i4")])
NP_RC_BLOCK = np.dtype([("consensus", "<u8"), ("cons_len", "<u4"), ("n_members", "<u4")])
NP_MEMBER = np.dtype([("n_subs", "<u4"), ("n_dels", "<u4"), ("n_inss", "<u4")])
NP_SUB = np.dtype([("pos", "<u4"), ("alt", "<u4")])


def letters(seed, n):
    """n letters in a pattern that depends on the seed, so that a copy from the wrong place shows"""
    return bytes(b"ACGT"[(seed * 7 + k * k + k // 3) % 4] for k in range(n)) if n < 4096 else (letters(seed, 1024) * (n // 1024 + 1))[:n]


def build(blocks, paths, slots="asc", pool=b"", pin=None, text=None):
    """blocks: [(block_id, consensus) or None for a dead entry]; paths: [(path_id, circular, tot_len, name, desc, [node])] with node = (node_id,
    block index, reverse, pos0, pos1, edit); edit: None or {"subs": [(pos, letter)], "dels": [(pos, len)], "inss": [(pos, seq) or (pos, len,
    seq_off) into `pool`]}.  slots: the member order of every block by node id: "asc", "desc" or a seed to shuffle with"""
    by_block = {}
    for p in paths:
        for n in p[5]:
            by_block.setdefault(n[1], []).append(n[0])
    slot, ins_seq = {}, bytearray(pool)
    for b, ids in by_block.items():
        ids.sort(reverse=slots == "desc")
        if isinstance(slots, int):
            random.Random(slots * 1000 + b).shuffle(ids)
        slot.update({n: k for k, n in enumerate(ids)})
    members = [[None] * len(by_block.get(b, [])) for b in range(len(blocks))]
    p_list, n_list, meta = [], [], []
    enc = lambda s: s.encode() if isinstance(s, str) else s
    for pid, circular, tot_len, name, desc, nodes in paths:
        p_list.append((pid, len(n_list), len(nodes), 1 if circular else 0))
        meta.append((tot_len, enc(name), enc(desc)))
        for nid, b, rev, pos0, pos1, edit in nodes:
            n_list.append((nid, pos0, pos1, b, slot[nid], 1 if rev else 0))
            e = {"subs": [], "dels": [], "inss": []}
            for pos, a in (edit or NONE)["subs"]:
                e["subs"].append((pos, a if isinstance(a, int) else ord(a)))
            e["dels"] = list((edit or NONE)["dels"])
            for x in (edit or NONE)["inss"]:
                if len(x) == 2:
                    e["inss"].append((x[0], len(x[1]), len(ins_seq)))
                    ins_seq += enc(x[1])
                else:
                    e["inss"].append(tuple(x))
            members[b][slot[nid]] = e
    b_list = [(0, 0, 0, 0) if blk is None else (blk[0], len(blk[1]), len(members[i]), 1) for i, blk in enumerate(blocks)]
    return {"blocks": b_list, "cons": [None if blk is None else enc(blk[1]) for blk in blocks], "paths": p_list, "nodes": n_list, "members": members, "ins_seq": bytes(ins_seq),
            "meta": meta, "pin": pin or (lambda e: True), "text": text}


def to_json(c):
    """the pangraph JSON of a case (alive blocks only): what jsonout.json_write_str, json_tables and json_from_json take"""
    dec = lambda s: None if s is None else s.decode()
    g = {"paths": {}, "nodes": {}, "blocks": {str(b[0]): {"id": b[0], "consensus": c["cons"][i].decode(), "alignments": {}} for i, b in enumerate(c["blocks"]) if b[3]}}
    for k, (pid, off, n, circular) in enumerate(c["paths"]):
        tot_len, name, desc = c["meta"][k]
        g["paths"][str(pid)] = {"id": pid, "nodes": [x[0] for x in c["nodes"][off:off + n]], "tot_len": tot_len, "circular": bool(circular), "name": dec(name), "desc": dec(desc)}
        for nid, pos0, pos1, b, m, rev in c["nodes"][off:off + n]:
            bid, e = c["blocks"][b][0], c["members"][b][m]
            g["nodes"][str(nid)] = {"id": nid, "block_id": bid, "path_id": pid, "strand": "-" if rev else "+", "position": [pos0, pos1]}
            g["blocks"][str(bid)]["alignments"][str(nid)] = {"subs": [{"pos": p, "alt": chr(a)} for p, a in e["subs"]], "dels": [{"pos": p, "len": n_} for p, n_ in e["dels"]],
                                                             "inss": [{"pos": p, "seq": c["ins_seq"][o:o + n_].decode()} for p, n_, o in e["inss"]]}
    return g


def expected_of(c):
    """jsonout.json_tables of the case, block_off per block INDEX (U64 for a dead entry)"""
    exp = jsonout.json_tables(to_json(c))
    alive = iter(exp["block_off"])
    exp["block_off"] = [next(alive) if b[3] else U64 for b in c["blocks"]]
    return exp


def flat(c):
    return jsonout.Flat(c["blocks"], c["paths"], c["nodes"], c["cons"], c["members"], c["ins_seq"], c["meta"])


def dump(c, exp, file):
    """the flat binary tests/emu/json_emu.cpp reads: the arrays of the call, then the text and the tables of the restatement"""
    opt = lambda s: struct.pack("<I", U32) if s is None else struct.pack("<I", len(s)) + s
    flat_m = [e for m in c["members"] for e in m]
    subs, dels, inss = ([x for e in flat_m for x in e[k]] for k in ("subs", "dels", "inss"))
    out = [b"PGAJSON1", struct.pack("<9Q", len(c["blocks"]), len(c["paths"]), len(c["nodes"]), len(flat_m), len(subs), len(dels), len(inss), len(c["ins_seq"]), len(exp["text"]))]
    out += [struct.pack("<QIIii", b[0], b[1], b[2], 1 if b[3] else 0, 0) for b in c["blocks"]]
    out += [struct.pack("<QQIi", *p) for p in c["paths"]]
    out += [struct.pack("<QQQIIii", *n, 0) for n in c["nodes"]]
    out += [opt(x) for x in c["cons"]]
    out += [struct.pack("<III", len(e["subs"]), len(e["dels"]), len(e["inss"])) for e in flat_m]
    out += [struct.pack("<II", *x) for x in subs] + [struct.pack("<II", *x) for x in dels] + [struct.pack("<IIQ", *x) for x in inss] + [c["ins_seq"]]
    out += [struct.pack("<Q", m[0]) + opt(m[1]) + opt(m[2]) for m in c["meta"]]
    out += [exp["text"], struct.pack("<3Q", *exp["section_off"]), struct.pack(f"<{len(exp['path_off'])}Q", *exp["path_off"]), struct.pack(f"<{len(exp['block_off'])}Q", *exp["block_off"]),
            struct.pack(f"<{len(exp['node_order'])}I", *exp["node_order"])]
    with open(file, "wb") as f:
        f.write(b"".join(out))


def node(nid, b, edit=None, rev=False, pos=(0, 0)):
    return (nid, b, rev, pos[0], pos[1], edit)


def simple(n_nodes=2, **kw):
    """one path "p" over one block of n_nodes members without an edit, node ids 101 ..."""
    return build([(1, "ACGT")], [(1, False, 4, "p", None, [node(101 + k, 0) for k in range(n_nodes)])], **kw)


# ---------------------------------------------------------------- numbers at every decimal width
WIDTHS_64 = sorted({10 ** k - 1 for k in range(1, 20)} | {10 ** k for k in range(1, 20)} | {U64})
WIDTHS_32 = sorted({10 ** k - 1 for k in range(1, 10)} | {10 ** k for k in range(1, 10)} | {0, U32})


def _widths_64():
    """block ids, path ids, node ids, positions and tot_len at 9, 10, 99, 100 ... 2^64 - 1: path k holds node k of block k"""
    w = WIDTHS_64
    blocks = [(x, "AC") for x in w]
    paths = [(x, k % 2 == 0, w[-1 - k], f"p{k}", None, [node(w[(k * 7) % len(w)], k, rev=k % 3 == 0, pos=(w[(k * 3) % len(w)], w[(k * 5 + 1) % len(w)]))]) for k, x in enumerate(w)]
    return build(blocks, paths, pin=lambda e: all(b'"id": %d,' % x in e["text"] and b"\n        %d" % x in e["text"] and b'"tot_len": %d,' % x in e["text"] for x in w)
                 and b'"18446744073709551615": {\n      "id": 18446744073709551615,\n      "block_id": ' in e["text"])


def _widths_32():
    """pos and len of the edits at every width up to 2^32 - 1"""
    w = WIDTHS_32
    edit = {"subs": [(x, "ACGT"[k % 4]) for k, x in enumerate(w)], "dels": [(x, w[-1 - k]) for k, x in enumerate(w)], "inss": [(x, "GA"[:k % 3]) for k, x in enumerate(w)]}
    return build([(1, "ACGT")], [(1, True, 4, "p", "d", [node(7, 0, edit)])],
                 pin=lambda e: all(b'"pos": %d,\n              "alt"' % x in e["text"] and b'"len": %d\n' % x in e["text"] and b'"pos": %d,\n              "seq"' % x in e["text"] for x in w))


# ---------------------------------------------------------------- names and descriptions
def _null_name_desc():
    paths = [(1, False, 1, None, "only desc", [node(11, 0)]), (2, True, 2, "only name", None, [node(12, 0)]), (3, False, 3, "both", "set", []), (4, True, 0, "", "", []), (5, False, 0, None, None, [])]
    return build([(1, "A")], paths, pin=lambda e: e["text"].count(b": null") == 4 and b'"name": "",\n      "desc": ""\n' in e["text"],
                 text=b'{\n  "paths": {\n    "1": {\n      "id": 1,\n      "nodes": [\n        11\n      ],\n      "tot_len": 1,\n      "circular": false,\n      "name": null,\n      "desc": "only desc"\n    },\n'
                      b'    "2": {\n      "id": 2,\n      "nodes": [\n        12\n      ],\n      "tot_len": 2,\n      "circular": true,\n      "name": "only name",\n      "desc": null\n    },\n'
                      b'    "3": {\n      "id": 3,\n      "nodes": [],\n      "tot_len": 3,\n      "circular": false,\n      "name": "both",\n      "desc": "set"\n    },\n'
                      b'    "4": {\n      "id": 4,\n      "nodes": [],\n      "tot_len": 0,\n      "circular": true,\n      "name": "",\n      "desc": ""\n    },\n'
                      b'    "5": {\n      "id": 5,\n      "nodes": [],\n      "tot_len": 0,\n      "circular": false,\n      "name": null,\n      "desc": null\n    }\n  },\n'
                      b'  "blocks": {\n    "1": {\n      "id": 1,\n      "consensus": "A",\n      "alignments": {\n        "11": {\n          "subs": [],\n          "dels": [],\n          "inss": []\n        },\n'
                      b'        "12": {\n          "subs": [],\n          "dels": [],\n          "inss": []\n        }\n      }\n    }\n  },\n'
                      b'  "nodes": {\n    "11": {\n      "id": 11,\n      "block_id": 1,\n      "path_id": 1,\n      "strand": "+",\n      "position": [\n        0,\n        0\n      ]\n    },\n'
                      b'    "12": {\n      "id": 12,\n      "block_id": 1,\n      "path_id": 2,\n      "strand": "+",\n      "position": [\n        0,\n        0\n      ]\n    }\n  }\n}')


ESCAPES = ['q"q', "b\\s", "\x01", "\x1f", "l\nf", "t\tb", "\x7f", "plásmido 中文 \U0001f9ec", "\b\f\r", '"\\\n\x00/']
ESCAPED = [b'q\\"q', b"b\\\\s", b"\\u0001", b"\\u001f", b"l\\nf", b"t\\tb", b"\x7f", "plásmido 中文 \U0001f9ec".encode(), b"\\b\\f\\r", b'\\"\\\\\\n\\u0000/']


def _escapes():
    paths = [(k + 1, False, 0, s, ESCAPES[-1 - k], [node(50 + k, 0)] if k == 0 else []) for k, s in enumerate(ESCAPES)]
    return build([(1, "A")], paths, pin=lambda e: all(b'"name": "%s",\n      "desc": "%s"\n' % (x, ESCAPED[-1 - k]) in e["text"] for k, x in enumerate(ESCAPED)))


ESCAPE_ALL = [chr(c) for c in range(128)] + ["é", "中", "\U0001f9ec", "a b", "\x7f\x80", 'x"\\\n\x00y']   # every single byte that is valid UTF-8, a few longer


def _escape_every_byte():
    return build([(1, "A")], [(k, False, 0, s, s + s, []) for k, s in enumerate(ESCAPE_ALL)], pin=lambda e: e["text"].count(b"\\u00") == 3 * 27 + 3 and b'"name": "\x7f",' in e["text"])


def _long_name_desc():
    return build([(1, "ACGT")], [(1, False, 4, "x" * 9000, "y\n" * 2500, [node(5, 0)]), (2, True, 4, "second", "z" * 5000, [node(6, 0)])],
                 pin=lambda e: e["path_off"][1] > 3 * EDGE and e["section_off"][1] > 5 * EDGE and e["text"].count(b"y\\n") == 2500)


# ---------------------------------------------------------------- edits
def _edit_combos():
    """eight members: subs, dels and inss empty or not in every combination"""
    mk = lambda k: {"subs": [(1, "T"), (2, "G")] if k & 1 else [], "dels": [(3, 1)] if k & 2 else [], "inss": [(0, "AC"), (4, "G")] if k & 4 else []}
    want = b'"subs": [],\n          "dels": [\n            {\n              "pos": 3,\n              "len": 1\n            }\n          ],\n          "inss": []\n'
    return build([(1, "ACGT")], [(1, False, 32, "p", None, [node(20 + k, 0, mk(k)) for k in range(8)])],
                 pin=lambda e: e["text"].count(b'"subs": []') == 4 and e["text"].count(b'"dels": []') == 4 and e["text"].count(b'"inss": []') == 4 and want in e["text"])


def _block_no_edits():
    return build([(1, "ACGT"), (2, "GG")], [(1, False, 8, "p", None, [node(31, 0), node(32, 1, {"subs": [(0, "A")], "dels": [], "inss": []}), node(33, 0)]), (2, False, 4, "q", None, [node(34, 0)])],
                 pin=lambda e: e["text"].count(b'"subs": [],\n          "dels": [],\n          "inss": []') == 3)


def _empty_path():
    return build([(1, "ACGT")], [(1, False, 0, "first", None, []), (2, True, 4, "mid", None, [node(41, 0)]), (5, False, 0, "last", None, [])],
                 pin=lambda e: e["text"].count(b'"nodes": [],') == 2)


def _no_nodes():
    """paths without a node, an alive block without a member, a dead entry: empty maps inside a graph that is not empty"""
    return build([None, (4, "ACG")], [(1, False, 0, "a", None, []), (2, False, 0, None, "b", [])], pin=lambda e: e["text"].endswith(b'"alignments": {}\n    }\n  },\n  "nodes": {}\n}'))


def _only_dead():
    return build([None, None], [], pin=lambda e: e["text"] == jsonout.EMPTY, text=jsonout.EMPTY)


def _dead_between():
    blocks = [None, (3, "AAC"), None, None, (8, "G"), (9, "TT"), None]
    return build(blocks, [(1, True, 6, "p", None, [node(61, 4), node(62, 1, rev=True), node(63, 5)]), (2, False, 1, "q", None, [node(64, 4)])],
                 pin=lambda e: [o == U64 for o in e["block_off"]] == [True, False, True, True, False, False, True])


def _slots(order):
    """three blocks of four members each over two paths; the member slots in descending / shuffled node id: the alignments still ascend"""
    mk = lambda nid: {"subs": [(nid % 10, "ACGT"[nid % 4])], "dels": [(nid % 7, 1)] * (nid % 2), "inss": [(0, "TG"[:nid % 3])]}
    ids = [904, 17, 560, 33, 12, 871, 405, 99, 250, 18, 777, 6]
    paths = [(1, False, 10, "p", None, [node(n, k % 3, mk(n)) for k, n in enumerate(ids[:7])]), (2, True, 10, "q", None, [node(n, (k + 7) % 3, mk(n)) for k, n in enumerate(ids[7:])])]
    def pin(e):
        keys = [int(l.split(b'"')[1]) for l in e["text"].split(b"\n") if l.startswith(b'        "')]
        return keys == sorted(ids[0::3]) + sorted(ids[1::3]) + sorted(ids[2::3])
    return build([(1, "ACGTACGTAC"), (2, "ACGTACGTAC"), (3, "ACGTACGTAC")], paths, slots=order, pin=pin)


def _adjacent_ids():
    """node ids 1000 .. 1011 dealt round the three paths, and round two blocks the other way"""
    paths = [(p + 1, False, 12, f"p{p}", None, [node(1000 + k, k % 2, {"subs": [(k, "A")], "dels": [], "inss": []}) for k in range(11, -1, -1) if k % 3 == p]) for p in range(3)]
    return build([(1, "A" * 12), (2, "C" * 12)], paths, slots=5, pin=lambda e: e["node_order"] == [3, 7, 11, 2, 6, 10, 1, 5, 9, 0, 4, 8])


def _high_block_index():
    blocks = [None] * ((1 << 16) + 5) + [(1, "ACGT"), None, (2, "GG")]
    at = (1 << 16) + 5
    return build(blocks, [(1, True, 6, "p", None, [node(71, at, {"subs": [(1, "G")], "dels": [], "inss": [(2, "AA")]}), node(72, at + 2), node(73, at, rev=True)])],
                 pin=lambda e: e["block_off"][at] < e["block_off"][at + 2] < U64 and e["block_off"][at + 1] == U64)


def _subs_in_one_member(n):
    edit = {"subs": [(k, "ACGT"[(k * k) % 4]) for k in range(n)], "dels": [], "inss": []}
    return build([(1, "ACGT"), (2, "AC")], [(1, False, 4, "p", None, [node(81, 0, edit), node(82, 1), node(83, 0)])], pin=lambda e: e["text"].count(b'"alt"') == n)


def _members_in_one_block(n):
    nodes = [node(5000 + (k * 7919) % 100003, 0, {"subs": [(k % 4, "T")] * (k % 5 == 0), "dels": [], "inss": []}, rev=k % 2 == 1) for k in range(n)]
    return build([(1, "ACGT"), (2, "AC")], [(1, True, 4 * n, "p", None, nodes), (2, False, 2, "q", None, [node(1, 1)])], slots=3,
                 pin=lambda e: e["text"].count(b'"subs"') == n + 1 and len(set(x[0] for x in nodes)) == n)


def _nodes_in_one_path(n):
    nodes = [node(10 ** 6 + (k * 104729) % (10 ** 6 + 3), k % 3, pos=(k, k + 1)) for k in range(n)]
    return build([(1, "A"), (2, "C"), (3, "G")], [(1, False, n, "p", None, nodes), (2, False, 1, "q", None, [node(7, 2)])], pin=lambda e: len(e["node_order"]) == n + 1)


def _heavy_member():
    """one member with 5 000 subs and 3 000 insertions beside 2 000 members without an edit"""
    edit = {"subs": [(k, "ACGT"[k % 4]) for k in range(5000)], "dels": [(k, 1 + k % 3) for k in range(7)], "inss": [(k, letters(k, k % 9)) for k in range(3000)]}
    nodes = [node(10 + 3 * k, 0, edit if k == 1000 else None) for k in range(2001)]
    return build([(1, letters(1, 5000))], [(1, False, 10 ** 7, "p", None, nodes)], pin=lambda e: e["text"].count(b'"alt"') == 5000 and e["text"].count(b'"seq"') == 3000)


INS_LENGTHS = (1, 63, 64, 65, 5000, 0, 128, 127)


def _ins_lengths():
    edit = {"subs": [], "dels": [], "inss": [(k, letters(k + 2, n)) for k, n in enumerate(INS_LENGTHS)]}
    return build([(1, "ACGT")], [(1, False, 4, "p", None, [node(91, 0, edit), node(92, 0, {"subs": [], "dels": [], "inss": [(0, letters(9, 64))]})])],
                 pin=lambda e: all(b'"seq": "%s"\n' % letters(k + 2, n) in e["text"] for k, n in enumerate(INS_LENGTHS)))


def _ins_shared():
    """two insertions share letters, others overlap, seq_off in shuffled order, letters no insertion names"""
    pool = b"?!" + letters(3, 100) + b"##"
    edit_a = {"subs": [], "dels": [], "inss": [(5, 70, 30), (1, 10, 2), (3, 70, 30)]}
    edit_b = {"subs": [], "dels": [], "inss": [(0, 100, 2), (2, 0, 104), (9, 1, 101)]}
    return build([(1, "ACGT")], [(1, False, 4, "p", None, [node(95, 0, edit_a), node(96, 0, edit_b)])], pool=pool,
                 pin=lambda e: e["text"].count(b'"seq": "%s"' % pool[30:100]) == 2 and b'"seq": "%s"' % pool[2:102] in e["text"] and b"?" not in e["text"] and b"#" not in e["text"])


# ---------------------------------------------------------------- tiles (PGA_EXPORT_TILE_KB=4)
def _cut(make, marker, into, pin_len=None):
    """make(pad) -> a case whose first path carries a name of `pad` letters; the pad that puts byte `into` of the first `marker` on a tile edge"""
    at = expected_of(make(0))["text"].index(marker) + into
    edge = (at + EDGE - 1) // EDGE * EDGE
    c = make(edge - at)
    c["pin"] = lambda e: e["text"].index(marker) + into == edge and (pin_len is None or len(marker) > into > 0)
    return c


def _cut_base(pad, cons="ACGT", edit=None):
    e = edit or {"subs": [(77777, "G"), (5, "T")], "dels": [], "inss": []}
    return build([(4242, cons)], [(1, False, 0, "n" * pad, None, []), (2, True, 9, "p", None, [node(555, 0), node(123456789012, 0, e, pos=(3, 7)), node(777, 0)])])


CUTS = {
    "cut_sub": lambda: _cut(_cut_base, b'"pos": 77777', 9, True),
    "cut_ins_letters": lambda: _cut(lambda pad: _cut_base(pad, edit={"subs": [], "dels": [], "inss": [(1, letters(4, 200))]}), letters(4, 200), 100, True),
    "cut_consensus": lambda: _cut(lambda pad: _cut_base(pad, cons=letters(6, 300)), letters(6, 300), 150, True),
    "cut_node_item": lambda: _cut(_cut_base, b'"block_id": 4242', 14, True),
    "cut_path_node_line": lambda: _cut(_cut_base, b"123456789012", 5, True),
    "item_end": lambda: _cut(_cut_base, b'"alt": "G"\n            }', 24),          # the tile ends exactly where the first sub item ends
}


# ---------------------------------------------------------------- past the second level of the tile scan
def big_text(n):
    """the text of big(n), put together from its parts (the restatement is too slow for 2^20 subs; tests/test_json_cpu.py holds this
    function against it at a small n)"""
    subs = ",\n".join('            {\n              "pos": %d,\n              "alt": "%s"\n            }' % (k, "ACGT"[(k * k + k // 5) % 4]) for k in range(n))
    return ('{\n  "paths": {\n    "1": {\n      "id": 1,\n      "nodes": [\n        7\n      ],\n      "tot_len": 4,\n      "circular": false,\n      "name": "big",\n      "desc": null\n    }\n  },\n'
            '  "blocks": {\n    "3": {\n      "id": 3,\n      "consensus": "ACGT",\n      "alignments": {\n        "7": {\n          "subs": [\n' + subs + '\n          ],\n          "dels": [],\n'
            '          "inss": []\n        }\n      }\n    }\n  },\n  "nodes": {\n    "7": {\n      "id": 7,\n      "block_id": 3,\n      "path_id": 1,\n      "strand": "+",\n      "position": [\n        0,\n'
            '        4\n      ]\n    }\n  }\n}').encode()


def big_case(n):
    k = np.arange(n)
    return build([(3, "ACGT")], [(1, False, 4, "big", None, [node(7, 0, {"subs": [(int(x), "ACGT"[(int(x) * int(x) + int(x) // 5) % 4]) for x in k], "dels": [], "inss": []}, pos=(0, 4))])])


@functools.lru_cache(maxsize=None)
def big():
    """1024 * 1024 + 1 subs in one member -> (the arrays of the call through numpy, what must stay alive, sha256 and length of the text, section_off)"""
    n = TILE * TILE + 1
    k = np.arange(n, dtype=np.uint64)
    S = np.zeros(n, NP_SUB)
    S["pos"] = k
    S["alt"] = np.frombuffer(b"ACGT", np.uint8)[(k * k + k // 5) % 4]
    cons = C.create_string_buffer(b"ACGT", 4)
    B = np.array([(3, 4, 1, 1, 0)], NP_BLOCK); P = np.array([(1, 0, 1, 0)], NP_PATH); N = np.array([(7, 0, 4, 0, 0, 0, 0)], NP_NODE)
    R = np.array([(C.addressof(cons), 4, 1)], NP_RC_BLOCK); M = np.array([(n, 0, 0)], NP_MEMBER)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    text = big_text(n)
    return ((1, ptr(B), 1, ptr(P), 1, ptr(N)), (1, ptr(R), ptr(M), ptr(S), None, None, None), [(4, b"big", None)], (B, P, N, R, M, S, cons),
            hashlib.sha256(text).hexdigest(), len(text), [4, text.index(b'"blocks": {'), text.index(b'"nodes": {')])


CASES = {
    "widths_64": _widths_64, "widths_32": _widths_32, "null_name_desc": _null_name_desc, "escapes": _escapes, "escape_every_byte": _escape_every_byte, "long_name_desc": _long_name_desc,
    "edit_combos": _edit_combos, "block_no_edits": _block_no_edits, "empty_path": _empty_path, "no_nodes": _no_nodes, "only_dead": _only_dead, "dead_between": _dead_between,
    "slots_descending": functools.partial(_slots, "desc"), "slots_shuffled": functools.partial(_slots, 11), "adjacent_ids": _adjacent_ids, "high_block_index": _high_block_index,
    **{f"subs_{n}": functools.partial(_subs_in_one_member, n) for n in (TILE - 1, TILE, TILE + 1)},
    **{f"members_{n}": functools.partial(_members_in_one_block, n) for n in (TILE - 1, TILE, TILE + 1)},
    **{f"nodes_{n}": functools.partial(_nodes_in_one_path, n) for n in (TILE - 1, TILE, TILE + 1)},
    "heavy_member": _heavy_member, "ins_lengths": _ins_lengths, "ins_shared": _ins_shared, **CUTS,
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    return expected_of(case(name))


# ---------------------------------------------------------------- seeded random graphs
@functools.lru_cache(maxsize=None)
def random_case(seed):
    """1-8 paths over 2-25 block entries (some dead), mixed strands, ids of mixed widths, random edits, names with escapes and nulls, the
    member slots shuffled"""
    rng = random.Random(7000 + seed)
    n_blocks, n_paths = rng.randint(2, 25), rng.randint(1, 8)
    ids = sorted(rng.sample(range(1, 5000), n_blocks - 1) + [rng.getrandbits(64)])
    blocks = [None if rng.random() < 0.2 else (ids[b], letters(b, rng.choice((0, 1, 5, 40, 200)))) for b in range(n_blocks)]
    alive = [b for b, x in enumerate(blocks) if x is not None]
    nids = iter(rng.sample(range(1, 10 ** 6), 400) + [rng.getrandbits(64) for _ in range(40)])
    def edit():
        if rng.random() < 0.3:
            return None
        return {"subs": [(rng.getrandbits(rng.choice((4, 12, 32))), rng.choice("ACGTN-acgt")) for _ in range(rng.choice((0, 0, 1, 3, 20)))],
                "dels": [(rng.getrandbits(rng.choice((4, 32))), rng.getrandbits(rng.choice((2, 32)))) for _ in range(rng.choice((0, 0, 1, 4)))],
                "inss": [(rng.getrandbits(rng.choice((4, 32))), letters(rng.randint(0, 9), rng.choice((0, 1, 2, 9, 64, 130)))) for _ in range(rng.choice((0, 0, 1, 3)))]}
    name = lambda: rng.choice((None, "", "plain", 'q"\\\n\t\x02', "é中", "n" * rng.randint(1, 300)))
    paths = []
    for p in range(n_paths):
        nodes = [node(next(nids), rng.choice(alive), edit(), rng.random() < 0.5, (rng.getrandbits(rng.choice((8, 40, 64))), rng.getrandbits(20))) for _ in range(rng.choice((0, 1, 2, 5, 9, 30)) if alive else 0)]
        paths.append((p * p + rng.randint(0, 1) + (1 << 40) * (p == n_paths - 1), rng.random() < 0.5, rng.getrandbits(rng.choice((8, 64))), name(), name(), nodes))
    paths = [p for k, p in enumerate(paths) if k == 0 or p[0] > paths[k - 1][0]]
    return build(blocks, paths, slots=rng.choice(("asc", "desc", seed)))
