"""pga_export_gfa without a GPU: the reference's own two vectors through gfa_write_str, what the cases of tests/gfa_gen.py hold (pinned on
the host restatement, which is the expectation of the GPU tests) and their hand-written texts, the ctypes mirrors against the header,
export_gfa / write_gfa over a stand-in for the device call (the packing, the letters and names as the library will read them, the sink
plumbing), and the kernels of pga_gfa_idx.h in a stand-alone program under the host sanitizers (tests/emu/gfa_emu.cpp)."""
import ctypes as C
import gzip
import io
import json
import os
import shutil
import subprocess
import types

import pytest

import gfa_gen as gg
from conftest import GOLDEN, ROOT
from pangraph_amd import batch, gfa
from pangraph_amd.gfa import GfaParams
from pangraph_amd.topology import topo_block_t, topo_edge_t, topo_node_t, topo_path_t, unpack_lists

VEC = json.load(open(os.path.join(GOLDEN, "gfa_vectors.json")))


# ---------------------------------------------------------------- the reference's own vectors
@pytest.mark.parametrize("name", ["test_gfa_empty", "test_gfa_general_case"])
def test_reference_vectors(name):
    v = VEC[name]
    assert gfa.gfa_write_str(v["graph"], GfaParams(**v["params"])) == v["expected"].encode()
    assert name != "test_gfa_general_case" or b"L\t1\t+\t2\t-\t*\tRC:i:2\n" in v["expected"].encode()


def test_missing_path_name_raises():
    g = json.loads(json.dumps(VEC["test_gfa_general_case"]["graph"]))
    del g["paths"]["1"]["name"]
    with pytest.raises(ValueError, match="no name"):
        gfa.gfa_write_str(g)
    g["paths"]["1"]["name"] = None
    with pytest.raises(ValueError, match="no name"):
        gfa.gfa_write_str(g, GfaParams(minimum_length=1000))                # (the reference unwraps the name of every path, emitted or not)


# ---------------------------------------------------------------- every named case holds what it is named for
@pytest.mark.parametrize("name", sorted(gg.CASES))
def test_named_case(name):
    c, exp = gg.case(name), gg.expected(name)
    assert c["pin"](exp), name
    if c["text"] is not None:
        assert exp["text"] == c["text"]
    if c["json"]:
        assert gfa.gfa_write_str(gg.to_json(c), c["params"]) == exp["text"]
    # the tables describe the text: every S and P line starts where its byte_off says, the steps are the P lines' items
    blocks = c["lists"][0]
    for b, _, _, _, off in exp["segments"]:
        assert exp["text"][off:].startswith(b"S\t%d\t" % blocks[b][0]) and (off == 0 or exp["text"][off - 1:off] == b"\n")
    for k, n, so, off in exp["paths"]:
        line = exp["text"][off:exp["text"].index(b"\n", off)]
        assert line.startswith(b"P\t" + c["names"][k] + b"\t")
        items = line[2 + len(c["names"][k]) + 1:].split(b"\t")[0].split(b",")
        assert items == [b"%d%s" % (blocks[b][0], b"-" if r else b"+") for b, r in exp["steps"][so:so + n]]
    assert sum(p[1] for p in exp["paths"]) == len(exp["steps"])


def test_tile_cases_are_cut_where_they_say():
    for name, inside in (("cut_segment", b"S\t2\t"), ("cut_link", b"L\t123456\t"), ("cut_step", b"234567-")):
        t = gg.expected(name)["text"]
        at = t.index(inside)
        assert at < gg.EDGE < at + len(inside), name
    t = gg.expected("record_end")["text"]
    assert t[gg.EDGE - 1:gg.EDGE] == b"\n" and t[gg.EDGE:].startswith(b"# edges\n")
    assert all(len(gg.expected(n)["text"]) < gg.EDGE for n in gg.CASES if n.startswith(("links_", "bounds_", "sequences_")))   # files shorter than a tile


def test_second_level_of_the_tile_scan():
    arrays, exp = gg.second_level()
    n = gg.TILE * gg.TILE + 1
    assert len(arrays["nodes"]) == n > gg.TILE * gg.SCAN_THREADS * 4 and len(arrays["blocks"]) == 4
    assert 0 < len(exp["steps"]) < n and [s[0] for s in exp["segments"]] == [1, 2, 3] and [p[1] > 0 for p in exp["paths"]] == [True] * 3
    assert exp["paths"][2][2] > gg.TILE * gg.SCAN_THREADS // 2 and len(exp["text"]) > 4 * len(exp["steps"])
    # the expectation of the large graph is that of a small graph of the same make
    small = gfa.gfa_tables([(7, 10, 2, 1), (17, 11, 1, 1)], [(1, 0, 3, 1)], [(1, 0, 0, 0, 0, 0), (2, 0, 0, 1, 0, 1), (3, 0, 0, 0, 1, 0)], GfaParams(minimum_length=11), None, [b"x"])
    assert small["text"] == b"H\tVN:Z:1.0\n# blocks\nS\t17\t*\tRC:i:11\tLN:i:11\n# edges\nL\t17\t+\t17\t+\t*\tRC:i:1\n# paths\nP\tx\t17-\t*\tTP:Z:circular\n"


def test_random_graphs_hold_what_the_gpu_tests_rely_on():
    n_dup = n_dropped_paths = n_filtered = n_self = n_wide = n_empty_names = 0
    for seed in range(40):
        c = gg.random_case(seed)
        for kw in gg.PARAM_SETS:
            exp = gfa.gfa_tables(*c["lists"], GfaParams(**kw), c["cons"], c["names"])
            assert gfa.gfa_write_str(gg.to_json(c), GfaParams(**kw)) == exp["text"]
            n_dup += sum(s[3] for s in exp["segments"])
            n_dropped_paths += len(c["lists"][1]) - len(exp["paths"])
            n_filtered += len(c["lists"][2]) - len(exp["steps"])
            n_self += sum(1 for l in exp["links"] if l[0] == l[1])
        n_wide += sum(1 for b in c["lists"][0] if b[0] >= 1 << 32)
        n_empty_names += sum(1 for n in c["names"] if not n)
    assert n_dup >= 50 and n_dropped_paths >= 50 and n_filtered >= 500 and n_self >= 10 and n_wide >= 40 and n_empty_names >= 40, \
        (n_dup, n_dropped_paths, n_filtered, n_self, n_wide, n_empty_names)


@pytest.fixture(scope="module")
def plasmids():
    return json.load(gzip.open(os.path.join(GOLDEN, "plasmids.json.gz")))


def test_plasmids_on_the_host(plasmids):
    n_paths = len(plasmids["paths"])
    plain = gfa.gfa_write_str(plasmids)
    seq = gfa.gfa_write_str(plasmids, GfaParams(include_sequences=True))
    core = gfa.gfa_write_str(plasmids, GfaParams(minimum_depth=n_paths))
    assert plain.count(b"\nS\t") == len(plasmids["blocks"]) and plain.count(b"\nP\t") == n_paths and len(seq) > len(plain) > len(core) > len(gfa.HEADER)
    assert all(int(l.split(b"\t")[3][5:]) >= n_paths * int(l.split(b"\t")[4][5:]) for l in core.split(b"\n") if l.startswith(b"S\t"))


# ---------------------------------------------------------------- the C interface
def test_gfa_structs_match_the_header(tmp_path):
    pairs = [("pga_gfa_params_t", gfa.gfa_params_t), ("pga_gfa_segment_t", gfa.gfa_segment_t), ("pga_gfa_path_t", gfa.gfa_path_t), ("pga_gfa_step_t", gfa.gfa_step_t),
             ("pga_gfa_out_t", gfa.gfa_out_t), ("pga_topo_edge_t", topo_edge_t)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pga_align.h"', 'int main(void) {']
    exp = []
    for name, ct in pairs:
        lines.append(f'  printf("%zu", sizeof({name}));')
        lines += [f'  printf(" %zu", offsetof({name}, {f[0]}));' for f in ct._fields_]
        lines.append('  printf("\\n");')
        exp.append([str(C.sizeof(ct))] + [str(getattr(ct, f[0]).offset) for f in ct._fields_])
    lines += ['  printf("%u\\n", PGA_GFA_STEPS);', '  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert got == exp + [[str(gfa.STEPS)]]


def test_numpy_mirrors_have_the_sizes_of_the_structs():
    for dt, ct in ((gg.NP_BLOCK, topo_block_t), (gg.NP_PATH, topo_path_t), (gg.NP_NODE, topo_node_t), (gg.NP_SEGMENT, gfa.gfa_segment_t), (gg.NP_EDGE, topo_edge_t),
                   (gg.NP_GPATH, gfa.gfa_path_t), (gg.NP_STEP, gfa.gfa_step_t)):
        assert dt.itemsize == C.sizeof(ct) and [dt.fields[f[0]][1] for f in ct._fields_] == [getattr(ct, f[0]).offset for f in ct._fields_]


def test_library_exports_the_gfa_entries(product_so):
    out = subprocess.run(["nm", "-D", "--defined-only", product_so], check=True, capture_output=True, text=True).stdout
    assert {"pga_export_gfa", "pga_gfa_free"} <= set(line.split()[-1] for line in out.splitlines() if " T " in line)


def test_params_bounds():
    assert GfaParams().bounds() == (0, gfa.U64_MAX, 0, gfa.U64_MAX) and GfaParams(3, 4, 5, 6).bounds() == (3, 4, 5, 6)
    p = GfaParams(minimum_depth=2, include_sequences=True).to_c()
    assert (p.min_len, p.max_len, p.min_depth, p.max_depth, p.no_duplicated, p.include_sequences) == (0, gfa.U64_MAX, 2, gfa.U64_MAX, 0, 1)


# ---------------------------------------------------------------- export_gfa over a stand-in for the device call
def stand_in(tile, calls):
    """an object with the three entries gfa.py binds: pga_export_gfa reads its arguments as the library does (the arrays by pointer, the
    letters and names from the caller's buffers at their lengths), makes the file with the host restatement and hands it to the sink in
    pieces of `tile` bytes"""
    state = {"error": b""}

    def export(nb, B, np_, P, nn, N, cons, names, name_len, prm, flags, out, sink, ctx):
        out = out._obj
        prm = C.cast(prm, C.POINTER(gfa.gfa_params_t))[0]
        blocks, paths, nodes = unpack_lists((nb, B, np_, P, nn, N))
        params = GfaParams(prm.min_len, prm.max_len, prm.min_depth, prm.max_depth, bool(prm.include_sequences), bool(prm.no_duplicated))
        cons_p = C.cast(cons, C.POINTER(C.c_void_p)) if cons else None
        names_p, lens = C.cast(names, C.POINTER(C.c_void_p)), C.cast(name_len, C.POINTER(C.c_uint32))
        read = lambda p, n: C.string_at(p, n) if n else b""
        try:
            exp = gfa.gfa_tables(blocks, paths, nodes, params, [read(cons_p[i], b[1]) if cons_p and cons_p[i] else None for i, b in enumerate(blocks)] if cons_p else None,
                                 [read(names_p[k], lens[k]) if names_p[k] or not lens[k] else None for k in range(np_)])
        except (ValueError, TypeError) as e:
            state["error"] = b"pga_export_gfa: " + str(e).encode()
            return -1
        out.n_segments, out.n_links, out.n_paths, out.n_steps, out.n_bytes = len(exp["segments"]), len(exp["links"]), len(exp["paths"]), len(exp["steps"]), len(exp["text"])
        calls.append({"flags": flags, "pieces": 0})
        if sink:
            fn = C.cast(sink, gfa.SINK)
            for at in range(0, len(exp["text"]), tile):
                piece = exp["text"][at:at + tile]
                calls[-1]["pieces"] += 1
                if fn(ctx, C.cast(C.c_char_p(piece), C.c_void_p), len(piece)) != 0:
                    state["error"] = b"pga_export_gfa: sink stopped the export"
                    return -1
        return 0
    return types.SimpleNamespace(pga_export_gfa=export, pga_gfa_free=lambda out: None, pga_last_error=lambda: state["error"])


@pytest.mark.parametrize("name", ["test_gfa_general_case", "test_gfa_empty"])
def test_stand_in_on_the_reference_vectors(name):
    v, calls = VEC[name], []
    assert gfa.export_gfa(v["graph"], GfaParams(**v["params"]), dll=stand_in(7, calls)) == v["expected"].encode()
    assert calls[0]["pieces"] == (len(v["expected"]) + 6) // 7


def test_stand_in_on_named_and_random_graphs(tmp_path):
    for c in [gg.case(n) for n in ("names", "sequences_on", "width_ids", "empty_paths", "long_name")] + [dict(gg.random_case(s), params=GfaParams(**gg.PARAM_SETS[s % 4])) for s in range(12)]:
        exp, calls = gfa.gfa_tables(*c["lists"], c["params"], c["cons"], c["names"]), []
        assert gfa.export_gfa(gg.to_json(c), c["params"], dll=stand_in(100, calls)) == exp["text"]
        with open(tmp_path / "out.gfa", "wb") as f:
            assert gfa.write_gfa(gg.to_json(c), f, c["params"], dll=stand_in(64, calls)) == len(exp["text"])
        assert (tmp_path / "out.gfa").read_bytes() == exp["text"]
    buf = io.BytesIO()
    gfa.write_gfa(VEC["test_gfa_general_case"]["graph"], buf, dll=stand_in(1 << 20, []))
    assert buf.getvalue() == gfa.gfa_write_str(VEC["test_gfa_general_case"]["graph"])
    assert gfa.write_gfa(VEC["test_gfa_empty"]["graph"], str(tmp_path / "empty.gfa"), dll=stand_in(4, [])) == len(gfa.HEADER) and (tmp_path / "empty.gfa").read_bytes() == gfa.HEADER


def test_stand_in_sink_stops_and_raises():
    v = VEC["test_gfa_general_case"]
    args, cons, names = gfa.gfa_from_json(v["graph"])
    got, calls = [], []
    with pytest.raises(batch.PgaError, match="sink stopped the export"):
        gfa.export_gfa_raw(args, cons, names, GfaParams(include_sequences=True), lambda piece: got.append(piece) or len(got) == 3, dll=stand_in(16, calls))
    assert len(got) == 3 == calls[0]["pieces"] and b"".join(got) == v["expected"].encode()[:48]

    def boom(piece):
        raise KeyError("from the sink")
    with pytest.raises(KeyError, match="from the sink"):
        gfa.export_gfa_raw(args, cons, names, None, boom, dll=stand_in(16, calls))
    out = gfa.export_gfa_raw(args, None, names, None, None, steps=True, dll=stand_in(16, calls))               # verdict mode: no piece
    assert calls[-1] == {"flags": gfa.STEPS, "pieces": 0} and out.n_bytes == len(gfa.gfa_write_str(v["graph"])) and out.n_steps == 7
    g = json.loads(json.dumps(v["graph"]))
    g["paths"]["0"]["name"] = None
    with pytest.raises(ValueError, match="no name"):
        gfa.export_gfa(g, dll=stand_in(16, calls))
    with pytest.raises(ValueError, match="entries for"):
        gfa.export_gfa_raw(args, None, names[:1], None, None, dll=stand_in(16, calls))


# ---------------------------------------------------------------- the kernels on the host
def test_gfa_kernels_under_emulation_and_sanitizers(tmp_path):
    """pga_gfa_idx.h: validation, the graph checks of pga_topo_idx.h, every kernel (duplication, the filter, the scans over more than one
    tile, the link keys and runs, the layout, the tile writer with items cut by tile edges, the host's copies of letters and names)
    against a direct scalar construction, and every refusal"""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "gfa_emu")
    subprocess.run([cxx, "-std=c++17", "-g1", "-O1", "-DPGA_EMU", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "emu", "gfa_emu.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    noise = [ln for ln in r.stderr.splitlines() if ln and "doesn't fully support makecontext/swapcontext" not in ln]
    assert r.returncode == 0 and r.stdout.startswith("gfa_emu OK") and not noise, (r.returncode, r.stdout, r.stderr)
