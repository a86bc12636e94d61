"""pga_rows.h without a GPU: the host row-table builder and k_rows (both instantiations) under dev/emu/hip_emu.h, in a stand-alone program under the
address and undefined-behaviour sanitizers (tests/emu/export_rows_emu.cpp), and what the GPU tests rely on their generated graphs for
(tests/export_gen.py), by the restatement tests/export_ref.py alone."""
import os
import shutil
import subprocess

import pytest

import export_gen as eg
import export_ref as er
from conftest import ROOT


def test_export_rows_under_emulation_and_sanitizers(tmp_path):
    """row tables of a few thousand rows, the kernel tile by tile into buffers of exactly the tile's size, every row against a direct
    scalar construction; the flags with and without an output buffer"""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "export_rows_emu")
    subprocess.run([cxx, "-std=c++17", "-g1", "-O0", "-DPGA_EMU", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "emu", "export_rows_emu.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    # (the one line the address sanitizer prints about swapcontext, which the emulator's fibers use, is no finding)
    noise = [ln for ln in r.stderr.splitlines() if ln and "doesn't fully support makecontext/swapcontext" not in ln]
    assert r.returncode == 0 and r.stdout.startswith("export_rows_emu OK") and not noise, (r.returncode, r.stdout, r.stderr)


def test_generated_graphs_hold_what_the_gpu_tests_rely_on():
    with_core = status2 = status3 = reverse = nodes = long_blocks = 0
    for seed in range(40):
        a, order_rows, order_members = eg.random_graph(seed)
        assert 1 <= a["n_paths"] <= 6 and 1 <= len(a["blocks"]) <= 8
        assert sorted(order_rows) == list(range(a["n_paths"])) and sorted(order_members) == list(range(len(a["member_path"])))
        for aligned in (True, False):
            rows, core = er.expected_results(aligned=aligned, **a)
            both = rows + er.expected_block_sequences(a["blocks"], aligned)
            status2 += sum(r["status"] == 2 for r in both); status3 += sum(r["status"] == 3 for r in both)
        with_core += bool(core)
        reverse += sum(1 for _, _, rev in a["guide_nodes"] if rev); nodes += len(a["guide_nodes"])
        long_blocks += sum(1 for b in a["blocks"] if len(b["consensus"]) >= 4000)
    assert with_core >= 30 and status2 >= 5 and status3 >= 5 and long_blocks >= 5 and 0.35 < reverse / nodes < 0.65, (with_core, status2, status3, long_blocks, reverse, nodes)
    a = eg.edge_graph()
    for aligned in (True, False):
        rows, core = er.expected_results(aligned=aligned, **a)
        assert all(r["status"] == 0 for r in rows) and len(core) == len(a["blocks"])
        assert {r["len"] for r in er.expected_block_sequences(a["blocks"], aligned)[:24:3]} == set(eg.UNIT_EDGE_LENGTHS)
    assert sum(len(b["consensus"]) for b in eg.big_graph()["blocks"]) * 6 > 290000


def test_export_structs_match_the_header(tmp_path):
    import ctypes as C
    from pangraph_amd import export as ex
    pairs = [("pga_export_seg_t", ex.export_seg_t), ("pga_export_res_t", ex.export_res_t), ("pga_core_block_t", ex.core_block_t)]
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
    assert ex.SEG_DTYPE.itemsize == C.sizeof(ex.export_seg_t) and [ex.SEG_DTYPE.fields[f[0]][1] for f in ex.export_seg_t._fields_] == [getattr(ex.export_seg_t, f[0]).offset for f in ex.export_seg_t._fields_]


def test_library_exports_the_export_entries(product_so):
    out = subprocess.run(["nm", "-D", "--defined-only", product_so], check=True, capture_output=True, text=True).stdout
    assert {"pga_block_sequences", "pga_core_alignment"} <= set(line.split()[-1] for line in out.splitlines() if " T " in line)


def test_core_records_refuses_shared_keys_before_any_device_call():
    import copy
    import json
    from conftest import GOLDEN
    from pangraph_amd.export import core_records
    g = copy.deepcopy(json.load(open(os.path.join(GOLDEN, "export_vectors.json")))["core_block_aln_general_case"]["graph"])
    for p in g["paths"].values():
        p["name"] = "Path A"
    with pytest.raises(ValueError, match="share a record key"):
        core_records(g, "Path A", dll=object())                          # (a library that cannot be called: the check comes first)
