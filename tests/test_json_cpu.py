"""pga_export_json without a GPU: the reference's own file through json_write_str, what the cases of tests/json_gen.py hold (pinned on the
host restatement, which is the expectation of the GPU tests) and their hand-written texts, the escape rules, the ctypes mirrors against
the header, export_json / write_json over a stand-in for the device call (the packing, the letters and names as the library will read
them, the sink plumbing), and the kernels of pga_json_idx.h in a stand-alone program under the host sanitizers (tests/emu/json_emu.cpp)."""
import ctypes as C
import gzip
import hashlib
import io
import json
import os
import shutil
import subprocess
import types

import pytest

import json_gen as jg
from conftest import GOLDEN, ROOT
from pangraph_amd import batch, jsonout
from pangraph_amd.mapvar import del_t, ins_t, sub_t
from pangraph_amd.reconsensus import rc_block_t, rc_member_t
from pangraph_amd.remove import edits_to_dicts
from pangraph_amd.topology import unpack_lists

PLASMIDS = os.path.join(GOLDEN, "plasmids.json.gz")


# ---------------------------------------------------------------- the reference's own file
def test_plasmids_restated_byte_for_byte():
    text = gzip.open(PLASMIDS, "rb").read()
    g = json.loads(text)
    assert len(text) == 1915265 and (len(g["paths"]), len(g["blocks"]), len(g["nodes"])) == (15, 137, 1042) and not text.endswith(b"\n")
    assert jsonout.json_write_str(g) == text
    assert jsonout.json_write_str(PLASMIDS) == text
    # through the flat arrays and back: what the device is given holds the whole graph
    F = jsonout.json_from_json(g)
    assert jsonout.json_write_str(unflatten(F)) == text
    t = jsonout.json_tables(g)
    assert [text[o:o + 8] for o in t["section_off"]] == [b'"paths":', b'"blocks"', b'"nodes":'] and len(t["path_off"]) == 15 and len(t["block_off"]) == 137
    assert all(text[o - 5:o + 1] == b'\n    "' for o in t["path_off"] + t["block_off"]) and sorted(t["node_order"]) == list(range(1042))


def unflatten(F):
    """a jsonout.Flat -> the pangraph JSON it holds, read from the C arrays as the library reads them"""
    blocks, paths, nodes = unpack_lists(F.graph_args)
    dicts = edits_to_dicts(*F.block_args)
    g = {"paths": {}, "nodes": {}, "blocks": {str(b[0]): {"consensus": dicts[i]["consensus"], "alignments": {}} for i, b in enumerate(blocks) if b[3]}}
    dec = lambda s: None if s is None else s.decode()
    for k, (pid, off, n, circular) in enumerate(paths):
        g["paths"][str(pid)] = {"nodes": [x[0] for x in nodes[off:off + n]], "tot_len": F.path_meta[k][0], "circular": bool(circular), "name": dec(F.path_meta[k][1]), "desc": dec(F.path_meta[k][2])}
        for nid, pos0, pos1, b, m, rev in nodes[off:off + n]:
            e = dicts[b]["members"][m]
            g["nodes"][str(nid)] = {"block_id": blocks[b][0], "path_id": pid, "strand": "-" if rev else "+", "position": [pos0, pos1]}
            g["blocks"][str(blocks[b][0])]["alignments"][str(nid)] = {"subs": [{"pos": p, "alt": a} for p, a in e["subs"]], "dels": [{"pos": p, "len": n_} for p, n_ in e["dels"]],
                                                                      "inss": [{"pos": p, "seq": s} for p, s in e["inss"]]}
    return g


# ---------------------------------------------------------------- every named case holds what it is named for
@pytest.mark.parametrize("name", sorted(jg.CASES))
def test_named_case(name):
    c, exp = jg.case(name), jg.expected(name)
    text = exp["text"]
    assert c["pin"](exp), name
    if c["text"] is not None:
        assert text == c["text"]
    assert json.loads(text) == jsonout.ordered(jg.to_json(c)) and text == jsonout.json_write_str(unflatten(jg.flat(c)))
    # the tables describe the text
    assert [text[o:o + 8] for o in exp["section_off"]] == [b'"paths":', b'"blocks"', b'"nodes":']
    assert all(text[o:].startswith(b'"%d": {' % p[0]) for o, p in zip(exp["path_off"], c["paths"])) and len(exp["path_off"]) == len(c["paths"])
    assert all(o == jg.U64 if not b[3] else text[o:].startswith(b'"%d": {\n      "id": %d,\n      "consensus"' % (b[0], b[0])) for o, b in zip(exp["block_off"], c["blocks"]))
    ids = [n[0] for n in c["nodes"]]
    assert [ids[k] for k in exp["node_order"]] == sorted(ids) and len(set(ids)) == len(ids)


def test_cases_cover_what_the_issue_names():
    assert jg.CHUNK == 64 and {n - jg.CHUNK for n in jg.INS_LENGTHS} >= {-63, -1, 0, 1, 4936}
    assert len(jg.expected("long_name_desc")["text"]) > 4 * jg.EDGE and len(jg.case("heavy_member")["members"][0]) == 2001
    for name in jg.CUTS:                                                     # each is cut by the first tile edge it can reach
        assert jg.case(name)["pin"](jg.expected(name)), name
    t = jg.expected("item_end")["text"]
    at = t.index(b'"alt": "G"\n            }') + 24
    assert at % jg.EDGE == 0 and t[at:at + 2] == b",\n"
    assert [len(jg.case(f"subs_{n}")["members"][0][0]["subs"]) for n in (1023, 1024, 1025)] == [1023, 1024, 1025]
    m = jg.case("slots_descending")["members"]
    assert [n[4] for n in jg.case("slots_descending")["nodes"] if n[3] == 0] != sorted(n[4] for n in jg.case("slots_descending")["nodes"] if n[3] == 0) and len(m) == 3
    assert jg.case("slots_shuffled")["nodes"] != jg.case("slots_descending")["nodes"]


def test_big_text_is_the_restatement_of_its_make():
    for n in (1, 2, 7):
        assert jg.big_text(n) == jsonout.json_write_str(jg.to_json(jg.big_case(n)))
    args, block_args, meta, _, sha, n_bytes, sec = jg.big()
    n = jg.TILE * jg.TILE + 1
    assert n_bytes > 70 * n and len(sha) == 64 and sec[0] == 4 < sec[1] < sec[2] == n_bytes - 159 and C.cast(block_args[2], C.POINTER(rc_member_t))[0].n_subs == n > jg.TILE * 256 * 4
    S = C.cast(block_args[3], C.POINTER(sub_t))
    assert [(S[k].pos, chr(S[k].alt)) for k in (0, 1, 6, n - 1)] == [(k, "ACGT"[(k * k + k // 5) % 4]) for k in (0, 1, 6, n - 1)]


def test_random_graphs_hold_what_the_gpu_tests_rely_on():
    n_null = n_dead = n_empty_paths = n_edits = n_wide = n_unsorted = 0
    for seed in range(40):
        c = jg.random_case(seed)
        exp = jg.expected_of(c)
        assert json.loads(exp["text"]) == jsonout.ordered(jg.to_json(c)) and exp["text"] == jsonout.json_write_str(unflatten(jg.flat(c)))
        n_null += sum((m[1] is None) + (m[2] is None) for m in c["meta"])
        n_dead += sum(1 for b in c["blocks"] if not b[3])
        n_empty_paths += sum(1 for p in c["paths"] if p[2] == 0)
        n_edits += sum(len(e["subs"]) + len(e["dels"]) + len(e["inss"]) for m in c["members"] for e in m)
        n_wide += sum(1 for n in c["nodes"] if n[0] >= 1 << 32 or n[1] >= 1 << 32)
        slot_ids = {}
        for n in c["nodes"]:
            slot_ids.setdefault(n[3], {})[n[4]] = n[0]
        n_unsorted += sum(1 for d in slot_ids.values() if [d[k] for k in sorted(d)] != sorted(d.values()))
    assert n_null >= 40 and n_dead >= 40 and n_empty_paths >= 10 and n_edits >= 2000 and n_wide >= 100 and n_unsorted >= 40, (n_null, n_dead, n_empty_paths, n_edits, n_wide, n_unsorted)


# ---------------------------------------------------------------- escaping
def test_escape_rules_are_those_of_json_dumps():
    names = [chr(c) for c in range(128)] + ["é", "中", "\U0001f9ec", "a b", "\x7f\x80", 'x"\\\n\x00y']      # every single byte that is valid UTF-8, a few longer
    g = jg.to_json(jg.build([(1, "A")], [(k, False, 0, s, s + s, []) for k, s in enumerate(names)]))
    text = jsonout.json_write_str(g)
    for k, s in enumerate(names):
        esc = json.dumps(s, ensure_ascii=False).encode()
        assert b'"name": %s,\n      "desc": %s%s\n' % (esc, esc[:-1], esc[1:]) in text, k
    lower = {c: json.dumps(chr(c)).lower() == json.dumps(chr(c)) for c in range(32)}
    assert all(lower.values()) and json.dumps("\x1f") == '"\\u001f"' and json.dumps("\x7f", ensure_ascii=False) == '"\x7f"'
    assert [json.dumps(chr(c)) for c in (8, 9, 10, 12, 13, 34, 92)] == ['"\\b"', '"\\t"', '"\\n"', '"\\f"', '"\\r"', '"\\""', '"\\\\"']


# ---------------------------------------------------------------- the C interface
def test_json_structs_match_the_header(tmp_path):
    pairs = [("pga_json_out_t", jsonout.json_out_t), ("pga_rc_block_t", rc_block_t), ("pga_rc_member_t", rc_member_t), ("pga_sub_t", sub_t), ("pga_del_t", del_t), ("pga_ins_t", ins_t)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pga_align.h"', 'int main(void) {']
    exp = []
    for name, ct in pairs:
        lines.append(f'  printf("%zu", sizeof({name}));')
        lines += [f'  printf(" %zu", offsetof({name}, {f[0]}));' for f in ct._fields_]
        lines.append('  printf("\\n");')
        exp.append([str(C.sizeof(ct))] + [str(getattr(ct, f[0]).offset) for f in ct._fields_])
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines + ['  return 0;', '}']))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert got == exp
    # the prototypes as jsonout._bind takes them, held by the compiler (compiled, not linked)
    protos = ['#include "pga_align.h"',
              'int (*entry)(int64_t, const pga_topo_block_t*, int64_t, const pga_topo_path_t*, int64_t, const pga_topo_node_t*, const char *const*, const pga_rc_member_t*,',
              '  const pga_sub_t*, const pga_del_t*, const pga_ins_t*, const char*, uint64_t, const uint64_t*, const char *const*, const uint32_t*, const char *const*, const uint32_t*,',
              '  uint32_t, pga_json_out_t*, pga_gfa_sink_t, void*) = pga_export_json;', 'void (*fr)(pga_json_out_t*) = pga_json_free;', 'void (*ms)(double*) = pga_json_last_ms;']
    (tmp_path / "protos.c").write_text("\n".join(protos) + "\n")
    subprocess.run(["gcc", "-std=gnu99", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(tmp_path / "protos.c"), "-o", str(tmp_path / "protos.o")], check=True)
    dll = types.SimpleNamespace(pga_export_json=types.SimpleNamespace(), pga_json_free=types.SimpleNamespace(), pga_json_last_ms=types.SimpleNamespace(), pga_last_error=types.SimpleNamespace())
    jsonout._bind(dll)
    assert len(dll.pga_export_json.argtypes) == 22 and dll.pga_export_json.argtypes[12] is C.c_uint64 and dll.pga_export_json.argtypes[18] is C.c_uint32
    assert len(jsonout.EMPTY) == 48 and json.loads(jsonout.EMPTY) == {"paths": {}, "blocks": {}, "nodes": {}} and jsonout.EMPTY == jsonout.json_write_str({"paths": {}, "blocks": {}, "nodes": {}})


def test_numpy_mirrors_have_the_sizes_of_the_structs():
    for dt, ct in ((jg.NP_RC_BLOCK, rc_block_t), (jg.NP_MEMBER, rc_member_t), (jg.NP_SUB, sub_t)):
        assert dt.itemsize == C.sizeof(ct) and [dt.fields[f[0]][1] for f in ct._fields_] == [getattr(ct, f[0]).offset for f in ct._fields_]


def test_library_exports_the_json_entries(product_so):
    out = subprocess.run(["nm", "-D", "--defined-only", product_so], check=True, capture_output=True, text=True).stdout
    assert {"pga_export_json", "pga_json_free", "pga_json_last_ms"} <= set(line.split()[-1] for line in out.splitlines() if " T " in line)


# ---------------------------------------------------------------- export_json over a stand-in for the device call
def stand_in(tile, calls):
    """an object with the entries jsonout.py binds: pga_export_json reads its arguments as the library does (the arrays by pointer, the
    consensus letters through cons[], names and descriptions at their lengths), makes the file with the host restatement and hands it to the
    sink in pieces of `tile` bytes"""
    state = {"error": b""}

    def export(nb, B, np_, P, nn, N, cons, members, subs, dels, inss, ins_seq, ins_seq_len, tot, names, name_len, descs, desc_len, flags, out, sink, ctx):
        out = out._obj
        blocks, paths, nodes = unpack_lists((nb, B, np_, P, nn, N))
        cons_p = C.cast(cons, C.POINTER(C.c_void_p))
        R = (rc_block_t * max(nb, 1))()
        for b in range(nb):
            C.c_void_p.from_address(C.addressof(R[b])).value = cons_p[b]
            R[b].cons_len, R[b].n_members = blocks[b][1], blocks[b][2] if blocks[b][3] else 0
        F = types.SimpleNamespace(graph_args=(nb, B, np_, P, nn, N), block_args=(nb, R, members, subs, dels, inss, ins_seq))
        tot_p, lens_n, lens_d = C.cast(tot, C.POINTER(C.c_uint64)), C.cast(name_len, C.POINTER(C.c_uint32)), C.cast(desc_len, C.POINTER(C.c_uint32))
        names_p, descs_p = C.cast(names, C.POINTER(C.c_void_p)), C.cast(descs, C.POINTER(C.c_void_p))
        F.path_meta = [(tot_p[k], C.string_at(names_p[k], lens_n[k]) if names_p[k] else None, C.string_at(descs_p[k], lens_d[k]) if descs_p[k] else None) for k in range(np_)]
        I = C.cast(inss, C.POINTER(ins_t))
        n_inss = sum(C.cast(members, C.POINTER(rc_member_t))[m].n_inss for m in range(sum(b[2] for b in blocks if b[3])))
        if any(I[k].seq_off + I[k].len > ins_seq_len for k in range(n_inss)):
            state["error"] = b"pga_export_json: seq_off + len of an insertion runs past the insertion letters"
            return -1
        t = jsonout.json_tables(unflatten(F))
        out.n_bytes, out.n_paths, out.n_blocks, out.n_nodes = len(t["text"]), np_, nb, nn
        out.section_off[:] = t["section_off"]
        calls.append({"flags": flags, "pieces": 0, "tables": t})
        if sink:
            fn = C.cast(sink, jsonout.SINK)
            for at in range(0, len(t["text"]), tile):
                piece = t["text"][at:at + tile]
                calls[-1]["pieces"] += 1
                if fn(ctx, C.cast(C.c_char_p(piece), C.c_void_p), len(piece)) != 0:
                    state["error"] = b"pga_export_json: sink stopped the export"
                    return -1
        return 0
    return types.SimpleNamespace(pga_export_json=export, pga_json_free=lambda out: None, pga_json_last_ms=lambda ms: None, pga_last_error=lambda: state["error"])


def test_stand_in_on_named_and_random_graphs(tmp_path):
    for c in [jg.case(n) for n in ("null_name_desc", "escapes", "edit_combos", "widths_64", "ins_lengths", "empty_path", "long_name_desc")] + [jg.random_case(s) for s in range(12)]:
        g, calls = jg.to_json(c), []
        want = jsonout.json_write_str(g)
        assert jsonout.export_json(g, dll=stand_in(100, calls)) == want and calls[0]["pieces"] == (len(want) + 99) // 100
        with open(tmp_path / "out.json", "wb") as f:
            assert jsonout.write_json(g, f, dll=stand_in(64, calls)) == len(want)
        assert (tmp_path / "out.json").read_bytes() == want
    buf = io.BytesIO()
    jsonout.write_json(jg.to_json(jg.case("escapes")), buf, dll=stand_in(1 << 20, []))
    assert buf.getvalue() == jg.expected("escapes")["text"]
    assert jsonout.write_json({"paths": {}, "blocks": {}, "nodes": {}}, str(tmp_path / "empty.json"), dll=stand_in(5, [])) == 48 and (tmp_path / "empty.json").read_bytes() == jsonout.EMPTY
    # the shuffled slots of a case reach the call as they are: the flat arrays, not a graph rebuilt from the JSON
    c, calls = jg.case("slots_shuffled"), []
    F = jg.flat(c)
    jsonout.export_json_raw(F.graph_args, F.block_args, F.path_meta, None, F.ins_seq_len, dll=stand_in(64, calls)).free()
    assert calls[0]["tables"]["text"] == jg.expected("slots_shuffled")["text"]


def test_stand_in_sink_stops_and_raises():
    c = jg.case("edit_combos")
    F, want = jg.flat(c), jg.expected("edit_combos")["text"]
    got, calls = [], []
    with pytest.raises(batch.PgaError, match="sink stopped the export"):
        jsonout.export_json_raw(F.graph_args, F.block_args, F.path_meta, lambda piece: got.append(piece) or len(got) == 3, F.ins_seq_len, dll=stand_in(16, calls))
    assert len(got) == 3 == calls[0]["pieces"] and b"".join(got) == want[:48]

    def boom(piece):
        raise KeyError("from the sink")
    with pytest.raises(KeyError, match="from the sink"):
        jsonout.export_json_raw(F.graph_args, F.block_args, F.path_meta, boom, F.ins_seq_len, dll=stand_in(16, calls))
    out = jsonout.export_json_raw(F.graph_args, F.block_args, F.path_meta, None, F.ins_seq_len, dll=stand_in(16, calls))      # verdict mode: no piece
    assert calls[-1]["pieces"] == 0 and out.n_bytes == len(want) and out.section_off == jg.expected("edit_combos")["section_off"]
    with pytest.raises(ValueError, match="entries for"):
        jsonout.export_json_raw(F.graph_args, F.block_args, F.path_meta[:0], None, F.ins_seq_len, dll=stand_in(16, calls))
    with pytest.raises(ValueError, match="ins_seq_len is needed"):
        jsonout.export_json_raw(F.graph_args, F.block_args[:6] + (C.cast(F.L, C.c_void_p),), F.path_meta, None, dll=stand_in(16, calls))
    with pytest.raises(batch.PgaError, match="runs past the insertion letters"):
        jsonout.export_json_raw(F.graph_args, F.block_args, F.path_meta, None, F.ins_seq_len - 1, dll=stand_in(16, calls))
    with pytest.raises(ValueError, match="number of blocks"):
        jsonout.export_json_raw(F.graph_args, (2,) + F.block_args[1:], F.path_meta, None, F.ins_seq_len, dll=stand_in(16, calls))


# ---------------------------------------------------------------- the kernels on the host
def test_json_kernels_under_emulation_and_sanitizers(tmp_path):
    """pga_json_idx.h: validation, escaping, the graph checks of pga_topo_idx.h, every kernel (the two orders, the edit scans, the checks of
    letters and ranges, the hierarchy, the layout, the tile writer with items cut by tile edges, the host's copies of letters, names and
    descriptions) on every named case against a direct scalar construction and against the restatement, and every refusal"""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "json_emu")
    subprocess.run([cxx, "-std=c++17", "-g1", "-O1", "-DPGA_EMU", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "emu", "json_emu.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    files = []
    for name in sorted(jg.CASES):
        files.append(str(tmp_path / f"{name}.bin"))
        jg.dump(jg.case(name), jg.expected(name), files[-1])
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    noise = [ln for ln in r.stderr.splitlines() if ln and "doesn't fully support makecontext/swapcontext" not in ln]
    assert r.returncode == 0 and r.stdout.startswith(f"json_emu OK ({len(files)} cases from files") and not noise, (r.returncode, r.stdout, r.stderr[-3000:])
