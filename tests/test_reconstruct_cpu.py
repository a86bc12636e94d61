"""The restatement of reconstruct (tests/reconstruct_ref.py) on a graph the reference wrote: tests/golden/plasmids.json.gz (the reference's
packages/pypangraph/tests/data/plasmids.json.gz) must spell the 15 sequences of tests/golden/plasmids.fa.gz; the reference's rotate_right
vectors (tests/golden/reconstruct_vectors.json); the JSON loader of pangraph_amd.reconstruct; the ctypes mirrors against the header; the
export of the entry.  No GPU."""
import ctypes as C
import gzip
import json
import os
import subprocess

import pytest

import reconstruct_ref as rr
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def plasmids():
    from pangraph_amd.reconstruct import graph_from_json
    raw = json.load(gzip.open(os.path.join(GOLDEN, "plasmids.json.gz"), "rt"))
    blocks, paths, names = graph_from_json(raw)
    fa_names, fa_seqs = rr.read_fasta(os.path.join(GOLDEN, "plasmids.fa.gz"))
    return raw, blocks, paths, names, fa_names, fa_seqs


def test_restatement_reproduces_the_plasmid_sequences(plasmids):
    raw, blocks, paths, names, fa_names, fa_seqs = plasmids
    assert len(paths) == 15 and len(blocks) == 137 and sum(len(p["nodes"]) for p in paths) == 1042
    assert sum(rev for p in paths for _, _, rev in p["nodes"]) == 33
    edits = [e for b in blocks for e in b["members"]]
    assert [sum(len(e[k]) for e in edits) for k in ("subs", "dels", "inss")] == [15476, 419, 427]
    assert min(p["first_pos"] for p in paths) == 2331 and max(p["first_pos"] for p in paths) == 95666
    by_name = dict(zip(fa_names, fa_seqs))
    for p, name in zip(paths, names):
        assert rr.reconstruct_path(blocks, p) == by_name[name]
        got = rr.expected_result(blocks, p, by_name[name])
        assert (got["status"], got["first_mismatch"], got["n_mismatch"]) == (0, -1, 0)


def test_rotate_vectors():
    V = json.load(open(os.path.join(GOLDEN, "reconstruct_vectors.json")))["rotate_right"]
    assert len(V) == 5
    for c in V:
        assert rr.rotate_right(c["input"], c["mid"]) == c["expected"]
    with pytest.raises(rr.Panic):
        rr.rotate_right("abc", 4)


def test_compare_and_status_order():
    assert rr.compare("ACGT", "ACGT") == (-1, 0)
    assert rr.compare("ACGT", "TCGA") == (0, 2)
    E = lambda **k: {"subs": k.get("subs", []), "dels": k.get("dels", []), "inss": k.get("inss", [])}
    blocks = [{"consensus": "ACGTXACGT", "members": [E(), E(dels=[(4, 1)]), E(subs=[(0, "-")]), E(subs=[(4, "-")], dels=[(4, 1)])]}]
    P = lambda nodes, tot, pos=0: {"nodes": nodes, "tot_len": tot, "first_pos": pos}
    st = lambda path, exp=None: rr.expected_result(blocks, path, exp)["status"]
    assert st(P([(0, 0, False)], 9)) == 0 and st(P([(0, 0, True)], 9)) == 2 and st(P([(0, 0, True)], 8)) == 2
    assert st(P([(0, 1, True)], 8)) == 0 and st(P([(0, 1, True)], 7)) == 1 and st(P([(0, 1, True)], 8, 9)) == 4 and st(P([(0, 1, True)], 7, 9)) == 1
    assert st(P([(0, 2, False)], 9)) == 3 and st(P([(0, 2, False)], 8)) == 3 and st(P([(0, 2, False), (0, 0, True)], 18)) == 2
    assert st(P([(0, 3, False)], 8)) == 0                                            # the '-' lies under a deletion
    assert st(P([(0, 1, False)], 8), "ACGTACG") == 5 and st(P([], 77, 5)) == 0 and st(P([], 0), "A") == 5
    # ACGTACGT is its own reverse complement: the path spells it twice, rotated right by 3
    assert rr.expected_result(blocks, P([(0, 1, False), (0, 1, True)], 16, 3), "CGTACGTACGTACGTA") == dict(status=0, len=16, seq="CGTACGTACGTACGTA", first_mismatch=-1, n_mismatch=0)
    assert rr.expected_result(blocks, P([(0, 1, False), (0, 1, True)], 16, 3), "CGAACGTACGTACGTT") == dict(status=0, len=16, seq="CGTACGTACGTACGTA", first_mismatch=2, n_mismatch=2)


def test_loader_round_trip(plasmids):
    """member numbering, node order and first_pos of the flattened arrays against the JSON they came from"""
    from pangraph_amd.reconstruct import _Packed
    raw, blocks, paths, names, _, _ = plasmids
    K = _Packed(blocks, paths)
    block_ids = sorted(raw["blocks"], key=int)
    assert [b["consensus"] for b in blocks] == [raw["blocks"][b]["consensus"] for b in block_ids]
    member_node = []                                                                # global member index -> node id
    for b in block_ids:
        member_node += sorted((int(n) for n in raw["blocks"][b]["alignments"]))
    assert len(member_node) == K.n_mem == 1042 and K.n_nodes == 1042
    assert [K.B[i].n_members for i in range(K.n_blocks)] == [len(raw["blocks"][b]["alignments"]) for b in block_ids]
    k = 0
    for i, pid in enumerate(sorted(raw["paths"], key=int)):
        p = raw["paths"][pid]
        assert names[i] == p["name"] and K.P[i].n_nodes == len(p["nodes"]) and K.P[i].tot_len == p["tot_len"]
        assert K.P[i].first_pos == raw["nodes"][str(p["nodes"][0])]["position"][0]
        for nid in p["nodes"]:
            node = raw["nodes"][str(nid)]
            m = K.N[k].member
            assert member_node[m] == int(nid) and K.N[k].reverse == (node["strand"] == "-")
            e = raw["blocks"][str(node["block_id"])]["alignments"][str(nid)]
            assert (K.M[m].n_subs, K.M[m].n_dels, K.M[m].n_inss) == (len(e["subs"]), len(e["dels"]), len(e["inss"]))
            k += 1
    assert sorted(K.N[j].member for j in range(K.n_nodes)) == list(range(1042))       # every member is some path's node, once


def test_reconstruct_structs_match_the_header(tmp_path):
    from pangraph_amd import reconstruct as rc
    pairs = [("pga_recon_path_t", rc.recon_path_t), ("pga_recon_node_t", rc.recon_node_t), ("pga_recon_res_t", rc.recon_res_t), ("pga_rc_block_t", rc.rc_block_t)]
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


def test_library_exports_pga_reconstruct(product_so):
    out = subprocess.run(["nm", "-D", "--defined-only", product_so], check=True, capture_output=True, text=True).stdout
    assert "pga_reconstruct" in set(line.split()[-1] for line in out.splitlines() if " T " in line)
