"""pga_assemble_blocks without a GPU: what the cases of tests/assemble_gen.py hold (pinned on host_assemble, the dict graph after of the host
reweave() flattened, which is the expectation of the GPU tests), host_assemble against detach.merged_blocks (the second oracle), the ctypes
mirrors against the header, the packing of pangraph_amd/assemble.py, and the kernels of pga_assemble_idx.h in a stand-alone program under
the host sanitizers (tests/emu/assemble_emu.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import apply_gen as ag
import assemble_gen as sg
from conftest import ROOT
from pangraph_amd import assemble as asm
from pangraph_amd import detach as dt
from pangraph_amd import slice as sl
from pangraph_amd.mapvar import res_t

M = asm.MERGED_ONLY


def _members(k, flags, block):
    """(first member, n_members) of an output block"""
    blocks = k["exp"][flags]["blocks"]
    return sum(b[1] for b in blocks[:block]), blocks[block][1]


# ---------------------------------------------------------------- every named case holds what it is named for
def test_reference_vector():
    k = sg.case("reference")
    assert len(k["t"]["promises"]) == 4 and k["exp"][0]["totals"][:2] == (6, 14) and k["exp"][M]["totals"][:2] == (4, 12)
    assert sorted(k["exp"][0]["origin"]) == sorted(-(1 + x) for x in range(14)) and [b for b in k["exp"][0]["blocks"] if b[1] == 0] == []


def test_anchor_and_append_members_alternate():
    k = sg.case("alternating")
    src = [-(o + 1) in k["k_append"] for o in k["exp"][M]["origin"]]
    assert len(src) == 8 and sum(src) == 4 and src != sorted(src) and src != sorted(src, reverse=True)
    ids = [w[0] for w in k["exp"][M]["who"]]
    assert ids == sorted(ids) and k["exp"][M]["blocks"] == [(b"A" * 20, 8)]
    first, n = _members(k, 0, [i for i, b in enumerate(k["exp"][0]["blocks"]) if b[1] == 8][0])
    assert k["exp"][0]["origin"][first:first + n] == k["exp"][M]["origin"] and k["exp"][0]["who"][first:first + n] == k["exp"][M]["who"]


def test_merged_blocks_of_one_side_only():
    k = sg.case("only_append")
    assert k["exp"][M]["blocks"] == [(b"A" * 20, 4)] and all(-(o + 1) in k["k_append"] for o in k["exp"][M]["origin"])
    k = sg.case("only_anchor")
    assert k["exp"][M]["blocks"] == [(b"A" * 20, 4)] and not k["k_append"] and k["t"]["res"] == [] and len(k["t"]["promises"]) == 1


def test_unaligned_slice_without_a_member():
    k = sg.case("empty_unaligned")
    assert [b[1] for b in k["exp"][0]["blocks"]] == [1, 2, 0, 2] and k["exp"][M]["totals"] == (0, 0, 0, 0, 0, 0) and k["t"]["promises"] == []


def test_single_deletion_result():
    k = sg.case("single_deletion")
    e = k["exp"][M]
    rows = [i for i, o in enumerate(e["origin"]) if -(o + 1) in k["k_append"]]
    assert len(rows) == 4 and all(e["counts"][i].tolist() == [0, 1, 0] for i in rows) and len(k["t"]["p_dels"]) == 4 and set(map(tuple, k["t"]["p_dels"].tolist())) == {(0, 20)}


def test_empty_cut():
    k = sg.case("no_cut")
    assert k["t"]["cut"] == [] and k["t"]["applied"] is None and k["exp"][0]["who"] is None and k["exp"][0]["origin"] == [0, 1, 2]
    assert k["exp"][0]["counts"].tolist() == np.asarray(k["t"]["counts"]).tolist() and k["exp"][M]["totals"] == (0, 0, 0, 0, 0, 0)
    assert sg.resolved(k["exp"][0]) == sg.resolved({"inss": k["t"]["inss"]}, k["t"]["ins_seq"])


def test_survivors_between_the_new_ids():
    k = sg.case("id_ranges")
    kinds = ["s" if o >= 0 else "n" for o in (k["exp"][0]["origin"][_members(k, 0, b)[0]] for b in range(7))]
    assert kinds == ["n", "s", "n", "n", "s", "n", "n"] and [b[0] for b in k["c"]["exp"]["blocks"]][-1] == (1 << 64) - 1


def test_block_index_above_2_16():
    k = sg.case("high_index")
    assert k["t"]["cut"][0][0] > 1 << 16 and k["t"]["blocks"][:5] == [(b"", 0)] * 5 and len(k["exp"][0]["blocks"]) == 4
    assert [o for o in k["exp"][0]["origin"] if o >= 0] == [2]                   # the survivor's member lies behind the two of the cut block


@pytest.mark.parametrize("n", [asm.TILE - 1, asm.TILE, asm.TILE + 1])
def test_member_counts_at_the_tile_edge(n):
    assert sg.case(f"members_{n}")["exp"][0]["totals"][1] == n


def test_block_straddles_a_tile_edge():
    k = sg.case("straddle")
    first, n = _members(k, 0, 1)
    assert first < asm.TILE < first + n and first == 1000 and n == 100


def test_one_member_with_thousands_of_edits():
    k = sg.case("one_heavy")
    c = k["exp"][0]["counts"]
    assert c[700].tolist() == [5000, 0, 3000] and int(c.sum()) == 8000 and len(c) >= 2001


def test_list_lengths_and_letter_counts():
    k = sg.case("list_lengths")
    assert set(range(131)) <= set(k["exp"][0]["counts"][:, 0].tolist()) and set(range(131)) <= set(k["exp"][0]["counts"][:, 2].tolist())
    k = sg.case("letters")
    for flags in (0, M):
        assert set(sg.INS_LETTERS) <= set(k["exp"][flags]["inss"]["len"].tolist())
    assert set(sg.INS_LETTERS) <= set(k["t"]["p_inss"]["len"].tolist())


def test_source_letters_are_shared_and_end_at_the_buffer():
    n_overlap = 0
    for name in sg.SMALL:
        t = sg.case(name)["t"]
        for pool, lists in ((t["ins_seq"], [t["inss"], t["s_inss"]]), (t["p_ins_seq"], [t["p_inss"]])):
            x = np.concatenate(lists)
            x = x[x["len"] > 0]
            if not len(x):
                continue
            assert int((x["seq_off"] + x["len"]).max()) == len(pool)                 # one insertion ends exactly at the end
            o = np.sort(x, order="seq_off")
            n_overlap += int((o["seq_off"][1:] < (o["seq_off"] + o["len"])[:-1]).sum())
            assert (np.diff(x["seq_off"].astype(np.int64)) < 0).any()                  # not in list order
    assert n_overlap >= 50


def test_second_level_of_the_scan():
    k = sg.case("second_level")
    assert int(k["exp"][M]["counts"][:, 0].max()) == asm.TILE * asm.TILE + 1 and k["exp"][0]["totals"][2] > asm.TILE * asm.TILE


def test_random_graphs_hold_what_the_gpu_tests_rely_on():
    n_merged = n_append = n_surv = n_empty = 0
    for seed in range(40):
        k = sg.random_case(seed)
        n_merged += len(k["t"]["promises"]); n_append += len(k["k_append"])
        n_surv += sum(1 for o in k["exp"][0]["origin"] if o >= 0); n_empty += sum(1 for b in k["exp"][0]["blocks"] if b[1] == 0)
    assert n_merged >= 100 and n_append >= 100 and n_surv >= 20, (n_merged, n_append, n_surv, n_empty)


# ---------------------------------------------------------------- the second oracle: the numpy gather of pangraph_amd/detach.py
def test_host_assemble_against_merged_blocks():
    n = 0
    for name, k in sg.all_cases():
        if not k["t"]["promises"]:
            continue
        assert [q["new_block_id"] for q in k["c"]["promises"]] == sorted(q["new_block_id"] for q in k["c"]["promises"]), name
        want, got = dt.merged_blocks(*sg.merged_blocks_input(k)), k["exp"][M]
        assert [b[0] for b in got["blocks"]] == [bytes(c) for c in want["cons"]] and [b[1] for b in got["blocks"]] == want["n_members"], name
        assert [w[0] for w in got["who"]] == want["node_ids"].tolist(), name
        assert got["counts"].tolist() == want["counts"].tolist() and got["subs"].tobytes() == want["subs"].tobytes() and got["dels"].tobytes() == want["dels"].tobytes(), name
        assert sg.resolved(got) == sg.resolved(want), name                         # (the two lay the letters out differently)
        n += len(want["cons"])
    assert n >= 100


# ---------------------------------------------------------------- the C interface
def test_assemble_structs_match_the_header(tmp_path):
    pairs = [("pga_assemble_out_t", asm.assemble_out_t), ("pga_slice_member_t", sl.slice_member_t), ("pga_mapvar_res_t", res_t)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pga_align.h"', 'int main(void) {']
    exp = []
    for name, ct in pairs:
        lines.append(f'  printf("%zu", sizeof({name}));')
        lines += [f'  printf(" %zu", offsetof({name}, {f[0]}));' for f in ct._fields_]
        lines.append('  printf("\\n");')
        exp.append([str(C.sizeof(ct))] + [str(getattr(ct, f[0]).offset) for f in ct._fields_])
    lines += ['  printf("%u %d\\n", PGA_ASSEMBLE_MERGED_ONLY, PGA_ASSEMBLE_TILE);', '  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert got == exp + [[str(asm.MERGED_ONLY), str(asm.TILE)]]
    # the record dtypes of the list level are those structs
    for dtype, ct in ((asm.SLICE_MEMBER, sl.slice_member_t), (asm.RES, res_t)):
        for name, _ in ct._fields_:
            if name in dtype.fields:
                assert dtype.fields[name][1] == getattr(ct, name).offset, name
    assert asm.SLICE_MEMBER.fields["n_subs"][1] == sl.slice_member_t.counts.offset


def test_library_exports_the_assemble_entries(product_so):
    out = subprocess.run(["nm", "-D", "--defined-only", product_so], check=True, capture_output=True, text=True).stdout
    assert {"pga_assemble_blocks", "pga_assemble_free", "pga_assemble_last_ms"} <= set(line.split()[-1] for line in out.splitlines() if " T " in line)


def test_tables_pack_what_the_case_holds():
    k = sg.case("alternating")
    K = asm.Tables(k["t"])
    t = k["t"]
    assert K.n_blocks == len(t["blocks"]) and [K.B[i].n_members for i in range(K.n_blocks)] == [b[1] for b in t["blocks"]] and K.n_cut == 2 and K.n_promises == 1
    assert [(K.K[i].block, K.K[i].n_intervals, K.K[i].first_interval) for i in range(2)] == t["cut"]
    assert (K.P[0].anchor_interval, K.P[0].append_interval) == t["promises"][0] and K.P[0].new_block_id == 900
    sm = np.asarray(t["s_members"])
    assert [(K.slice.members[i].counts.n_dels, K.slice.members[i].ins_off) for i in range(len(sm))] == [(int(r[1]), int(r[5])) for r in sm]
    assert [(K.slice.slices[i].member_off, K.slice.slices[i].n_kept) for i in range(4)] == [s[:2] for s in t["slices"]]
    a = K.applied
    assert (a.n_new_nodes, a.n_new_blocks, a.n_blocks, a.n_nodes) == (16, 3, 4, 17) and [a.member_src[i] for i in range(16)] == k["c"]["exp"]["member_src"]
    assert [(a.nodes[i].node_id, a.nodes[i].block, a.nodes[i].member, a.nodes[i].reverse) for i in range(17)] == [(n[0], n[3], n[4], n[5]) for n in k["c"]["exp"]["nodes"]]
    res = np.asarray(t["res"])
    assert [(int(K.R[i]["status"]), int(K.R[i]["n_inss"]), int(K.R[i]["sub_off"])) for i in range(len(res))] == [(int(r[0]), int(r[3]), int(r[4])) for r in res]


# ---------------------------------------------------------------- the kernels on the host
def test_assemble_kernels_under_emulation_and_sanitizers(tmp_path):
    """pga_assemble_idx.h: validation, every kernel (the three scans, the descriptors, who, the list copies, the letter gather) against a
    direct scalar construction in both modes, and every refusal of the host and of the kernels."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "assemble_emu")
    subprocess.run([cxx, "-std=c++17", "-g1", "-O1", "-DPGA_EMU", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "emu", "assemble_emu.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    noise = [ln for ln in r.stderr.splitlines() if ln and "doesn't fully support makecontext/swapcontext" not in ln]
    assert r.returncode == 0 and r.stdout.startswith("assemble_emu OK") and not noise, (r.returncode, r.stdout, r.stderr)


# ---------------------------------------------------------------- merge_round(blocks=stand-in): the tables and the reading back without a device
def test_restated_call_agrees_with_host_assemble():
    for name, k in sg.all_cases():
        if name != "second_level":                                               # (a million records in a Python loop)
            for flags in (0, M):
                assert sg.same(sg.list_assemble(k["t"], flags), k["exp"][flags]) is None, (name, flags)


def _canon(g):
    edit = lambda e: {f: [tuple(x) for x in e[f]] for f in ("subs", "dels", "inss")}
    return {"paths": {p: dict(v, nodes=list(v["nodes"])) for p, v in g["paths"].items()}, "nodes": {n: dict(v, position=tuple(v["position"])) for n, v in g["nodes"].items()},
            "blocks": {b: {"consensus": v["consensus"], "alignments": {n: edit(e) for n, e in v["alignments"].items()}} for b, v in g["blocks"].items()}}


def _round(run):
    try:
        return _canon(run())
    except asm.MergeError:
        return "MergeError"


def test_stand_in_blocks_against_the_round_in_dicts(oracle_lib):
    import json

    import promise_ref as pr
    import reweave_gen as rg
    import reweave_ref as rr
    from conftest import GOLDEN
    vec = json.load(open(os.path.join(GOLDEN, "reweave_vectors.json")))
    solve = lambda promises: [pr.solve_promise(oracle_lib.dll, q) for q in promises]
    calls = []

    def stand_in(t, flags):
        calls.append(flags)
        asm.Tables(t)                                                            # (the tables pack)
        return sg.list_assemble(t, flags)

    def both(make, thr, c):
        kw = dict(plan=rr.expected_call, slicer=ag.ref_slicer)
        g0, matches = make()
        g1, _ = make()
        want = _round(lambda: asm.merge_round(g0, matches, thr, solve, **kw))
        got = _round(lambda: asm.merge_round(g1, matches, thr, solve, blocks=stand_in, update=lambda *a: c["exp"], **kw))
        assert got == want
        return want

    want = both(lambda: rg.reference_graph(vec), vec["reweave"]["thr_len"], ag.case("reference"))
    assert want != "MergeError" and calls == [0] and sum(len(v["alignments"]) for v in want["blocks"].values()) == 14
    done = [both(lambda: ag.random_graph(seed), rg.THR, ag.random_case(seed)) != "MergeError" for seed in range(40)]
    assert sum(done) >= 6 and len(calls) == 1 + sum(done)                        # (random letters under random CIGARs: most rounds end in solve_promise's Err, on both sides)
