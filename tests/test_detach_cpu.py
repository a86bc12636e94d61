"""detach_unaligned_nodes without a GPU: the restatement tests/detach_ref.py against the reference's own unit-test values
(tests/golden/detach_vectors.json), XXH64 and the block id stream, the graph level and merged_blocks of pangraph_amd/detach.py against the
restatement, the ctypes mirrors against the header, the index arithmetic of the kernels in a stand-alone program under the host sanitizers
(tests/emu/detach_emu.cpp), and what the GPU tests rely on their generated batches for."""
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import detach_gen as dg
import detach_ref as dr
import simplify_ref as sr
from conftest import GOLDEN, ROOT
from pangraph_amd import detach as dt

VEC = json.load(open(os.path.join(GOLDEN, "detach_vectors.json")))


def _block(b):
    return sr.from_json({"paths": {}, "nodes": {}, "blocks": {"0": b}})["blocks"][0]


def _node(n, new_id):
    return {"block_id": new_id if n["block_id"] == "@new" else n["block_id"], "path_id": n["path_id"], "strand": n["strand"], "position": tuple(n["position"])}


# ---------------------------------------------------------------- the restatement against the reference's values
@pytest.mark.parametrize("case", ["forward", "reverse"])
def test_create_new_node_and_block_vectors(case):
    v = VEC["create_new_node_and_block"][case]
    old = _node(v["old_node"], None)
    node, bid, block = dr.create_new_node_and_block(v["node_id"], v["seq"], old)
    assert block == {"consensus": v["expected_consensus"], "alignments": {v["node_id"]: {"subs": [], "dels": [], "inss": []}}}
    assert bid == dr.block_id(v["node_id"], v["expected_consensus"]) and node == _node(v["expected_node"], bid)


def test_extract_unaligned_nodes_vector():
    v = VEC["extract_unaligned_nodes_simple"]
    block = _block(v["block"])
    assert dr.extract_unaligned_nodes(block) == [(u["node_id"], u["sequence"]) for u in v["expected_unaligned"]]
    assert block == _block(v["expected_block"])


def test_detach_unaligned_nodes_vector():
    v = VEC["detach_unaligned_nodes"]
    g = sr.from_json(v["graph"])
    blocks = [(b, g["blocks"][b]) for b in sorted(g["blocks"])]
    dr.detach_unaligned_nodes(blocks, g["nodes"])
    new = v["expected_new_block"]
    new_id = dr.block_id(new["node_id"], new["consensus"])
    assert len(blocks) == v["expected_n_blocks"] and blocks[0] == (0, _block(v["expected_block_0"]))
    assert blocks[1] == (new_id, {"consensus": new["consensus"], "alignments": {new["node_id"]: {"subs": [], "dels": [], "inss": []}}})
    assert g["nodes"] == {int(k): _node(n, new_id) for k, n in v["expected_nodes"].items()}
    # the product's graph level, the restatement standing in for the device
    h = dt.detach_graph(dt.normalize(v["graph"]), [0], detach=dr.expected_call)
    assert h["nodes"] == g["nodes"] and h["blocks"] == dict(blocks)


# ---------------------------------------------------------------- the block id
def test_xxh64_specification_values_and_the_block_id_stream():
    for f in (dr.xxh64, dt.xxh64):
        assert f(b"") == 0xEF46DB3751D8E999 and f(b"a") == 0xD24EC4F1A98C6E5B
    stream = bytes([2, 0, 0, 0, 0, 0, 0, 0,                    # NodeId(2): usize, little-endian
                    8, 0, 0, 0, 0, 0, 0, 0,                    # the length prefix of the Vec<AsciiChar>
                    0x47, 0x47, 0x47, 0x47, 0x47, 0x47, 0x47, 0x47])   # eight AsciiChar(b'G')
    assert dr.id_stream(2, "GGGGGGGG") == stream == dt.block_id_stream(2, "GGGGGGGG")
    assert dr.block_id(2, "GGGGGGGG") == dr.xxh64(stream) == dt.block_id(2, "GGGGGGGG")
    rng = random.Random(3)
    for n in (0, 1, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 4113):           # every tail and stripe count: the two implementations agree
        data = bytes(rng.randrange(256) for _ in range(n))
        assert dr.xxh64(data) == dt.xxh64(data)
    # the tuple-of-words stream of simplify.node_id is the same hash over 40 bytes
    import struct
    from pangraph_amd import simplify as sp
    assert sp.node_id(7, 3, True, (11, 500)) == dr.xxh64(struct.pack("<5Q", 7, 3, 1, 11, 500))


# ---------------------------------------------------------------- the C interface
def test_detach_structs_match_the_header(tmp_path):
    import ctypes as C
    pairs = [("pga_detach_member_t", dt.detach_member_t), ("pga_detach_orphan_t", dt.detach_orphan_t), ("pga_detach_out_t", dt.detach_out_t)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pga_align.h"', 'int main(void) {']
    exp = []
    for name, ct in pairs:
        lines.append(f'  printf("%zu", sizeof({name}));')
        lines += [f'  printf(" %zu", offsetof({name}, {f[0]}));' for f in ct._fields_]
        lines.append('  printf("\\n");')
        exp.append([str(C.sizeof(ct))] + [str(getattr(ct, f[0]).offset) for f in ct._fields_])
    lines += ['  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert got == exp


def test_library_exports_the_detach_entries(product_so):
    out = subprocess.run(["nm", "-D", "--defined-only", product_so], check=True, capture_output=True, text=True).stdout
    assert {"pga_detach_unaligned", "pga_detach_free"} <= set(line.split()[-1] for line in out.splitlines() if " T " in line)


def test_detach_index_arithmetic_under_emulation_and_sanitizers(tmp_path):
    """pga_detach_idx.h: the host tables, k_detach_count, the offsets and k_detach_pack, then k_rows over the orphans' rows, against a direct
    scalar construction on the edge batch and 40 random batches; the device's decision against the host's member by member.
    k_detach_scan (wave intrinsics) is not part of the emulated program."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "detach_emu")
    subprocess.run([cxx, "-std=c++17", "-g1", "-O1", "-DPGA_EMU", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "emu", "detach_emu.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    noise = [ln for ln in r.stderr.splitlines() if ln and "doesn't fully support makecontext/swapcontext" not in ln]
    assert r.returncode == 0 and r.stdout.startswith("detach_emu OK") and not noise, (r.returncode, r.stdout, r.stderr)


# ---------------------------------------------------------------- solve_promise's tail
def _pack(members):
    """[edit] -> (counts, subs, dels, inss, letters) in the packed layout"""
    counts = np.array([(len(e["subs"]), len(e["dels"]), len(e["inss"])) for e in members], np.uint32).reshape(-1, 3)
    letters = bytearray()
    inss = []
    for e in members:
        for pos, seq in e["inss"]:
            inss.append((pos, len(seq), len(letters)))
            letters += seq.encode()
    return (counts, np.array([(p, ord(a)) for e in members for p, a in e["subs"]], dt.SUB), np.array([d for e in members for d in e["dels"]], dt.DEL),
            np.array(inss, dt.INS), bytes(letters))


def _unpack(a):
    """a merged_blocks() dict -> per block (node ids, [edit])"""
    out, m, at = [], 0, [0, 0, 0]
    for nm in a["n_members"]:
        ids, members = [], []
        for _ in range(nm):
            c = a["counts"][m]
            s, d, i = (a[k][at[j]:at[j] + c[j]] for j, k in enumerate(("subs", "dels", "inss")))
            members.append({"subs": [(int(x["pos"]), chr(x["alt"])) for x in s], "dels": [(int(x["pos"]), int(x["len"])) for x in d],
                            "inss": [(int(x["pos"]), a["ins_seq"][int(x["seq_off"]):int(x["seq_off"]) + int(x["len"])].decode()) for x in i]})
            ids.append(int(a["node_ids"][m]))
            at = [at[j] + int(c[j]) for j in range(3)]
            m += 1
        out.append((ids, members))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_merged_blocks_against_the_restatement(seed):
    rng = random.Random(seed)
    edit = lambda: {"subs": [(rng.randrange(50), rng.choice("ACGT")) for _ in range(rng.randrange(4))], "dels": [(rng.randrange(40), rng.randrange(10)) for _ in range(rng.randrange(3))],
                    "inss": [(rng.randrange(51), "".join(rng.choice("ACGT") for _ in range(rng.randrange(6)))) for _ in range(rng.randrange(3))]}
    nb = rng.randint(1, 6)
    ids = rng.sample(range(1, 1 << 62), 20 * nb)                           # (interleaved: every block draws both sides from one shuffled pool)
    blocks = []
    for b in range(nb):
        na, npm = rng.randint(0 if seed else 1, 8), rng.randint(0 if seed else 1, 8)
        pool = ids[20 * b:20 * b + na + npm]
        blocks.append(({n: edit() for n in pool[:na]}, {n: edit() for n in pool[na:]}))
    a_members = [e for a, _ in blocks for _, e in sorted(a.items())]
    p_members = [e for _, p in blocks for _, e in sorted(p.items())]
    a_counts, a_s, a_d, a_i, a_l = _pack(a_members)
    # the promise output: the members' lists are addressed by offsets, not packed in member order -- here in reverse member order
    rev = p_members[::-1]
    p_counts, p_s, p_d, p_i, p_l = _pack(rev)
    first = np.cumsum(p_counts.astype(np.int64), axis=0) - p_counts
    res = np.concatenate([p_counts, first], axis=1)[::-1]
    anchor = {"cons": [b"A" * 50] * nb, "n_members": [len(a) for a, _ in blocks], "node_ids": [n for a, _ in blocks for n in sorted(a)], "counts": a_counts,
              "subs": a_s, "dels": a_d, "inss": a_i, "ins_seq": a_l}
    append = {"n_members": [len(p) for _, p in blocks], "node_ids": [n for _, p in blocks for n in sorted(p)], "res": res, "subs": p_s, "dels": p_d, "inss": p_i, "ins_seq": p_l}
    got = _unpack(dt.merged_blocks(anchor, append))
    assert got == [dr.merged_block("A" * 50, a, p) for a, p in blocks]
    if seed == 0:
        append["node_ids"][0] = anchor["node_ids"][0]
        with pytest.raises(ValueError):
            dt.merged_blocks(anchor, append)


# ---------------------------------------------------------------- what the GPU tests rely on their batches for
def test_generated_batches_hold_what_the_gpu_tests_rely_on():
    for seed in range(40):
        blocks, who = dg.random_batch(seed)
        assert len(blocks) <= 30 and all(len(b["members"]) <= 12 and len(b["consensus"]) <= 300 for b in blocks)
        kept, fwd, rev, emptied = dg.batch_facts(blocks, who)
        assert kept and fwd and rev and emptied, (seed, kept, fwd, rev, emptied)
        assert all(o["status"] == 0 for o in dr.expected_call(blocks, who)["orphans"])
    blocks, who = dg.edge_batch()
    exp = dr.expected_call(blocks, who)
    assert all(o["status"] == 0 for o in exp["orphans"])
    un = [[dr.aligned_count(e, len(b["consensus"])) == 0 for e in b["members"]] for b in blocks]
    assert any(u[:2] == [True, False] for u in un) and any(u[-2:] == [False, True] for u in un) and any(len(u) > 1 and all(u) for u in un)
    assert any(u[:4] == [False, True, True, False] for u in un) and [] in un
    assert {len(b["consensus"]) for b in blocks} >= {0} and {o["len"] for o in exp["orphans"]} >= set(dg.ORPHAN_LENGTHS)
    kept = [e for b, u in zip(blocks, un) for e, x in zip(b["members"], u) if not x]
    for kind in ("subs", "dels", "inss"):
        assert {len(e[kind]) for e in kept} >= set(dg.LIST_LENGTHS)
    assert any(sum(n for _, n in e["dels"]) == len(b["consensus"]) - 1 for b, u in zip(blocks, un) for e, x in zip(b["members"], u) if not x)
    lens = {o["len"]: set() for o in exp["orphans"]}
    flat_who = [w for blk in who for w in blk]
    for o in exp["orphans"]:
        lens[o["len"]].add(flat_who[o["member"]][1])
    assert all(lens[n] == {False, True} for n in dg.ORPHAN_LENGTHS)
    flat = [e for b in blocks for e in b["members"]]
    assert any(len(flat[o["member"]]["dels"]) == 200 for o in exp["orphans"]) and any(len([1 for _, s in flat[o["member"]]["inss"] if s]) >= 3 for o in exp["orphans"])
    blocks, who = dg.status_batch()
    assert [o["status"] for o in dr.expected_call(blocks, who)["orphans"]] == [2, 3, 0, 0, 3]
