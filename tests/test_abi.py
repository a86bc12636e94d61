"""The drop-in boundary: struct layouts of the minimap2-sys ABI and the symbols each library must export.
CPU-only: libraries are loaded, no compute call is made."""
import ctypes as C
import os
import re
import subprocess

from pangraph_amd import mm2ffi
from conftest import ROOT


def test_struct_sizes_match_reference_abi():
    # sizes measured on the reference's minimap.h with gcc
    assert C.sizeof(mm2ffi.mm_idxopt_t) == 24
    assert C.sizeof(mm2ffi.mm_mapopt_t) == 248
    assert C.sizeof(mm2ffi.mm_reg1_t) == 80
    assert C.sizeof(mm2ffi.mm_extra_t) == 24
    assert C.sizeof(mm2ffi.mm_idx_t) == 80
    assert C.sizeof(mm2ffi.mm_idx_seq_t) == 24


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b((?:mm|pga)_[a-z0-9_]+)\s*\(", txt)))


def test_product_exports_every_declared_symbol(product_so):
    out = subprocess.run(["nm", "-D", "--defined-only", product_so], check=True, capture_output=True, text=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    declared = _declared("pga_mm2_abi.h") + _declared("pga_align.h") + _declared("pga_sched.h")
    assert len(declared) >= 20
    missing = [s for s in declared if s not in exported]
    assert not missing, f"libpgalign.so does not export {missing}"
    # and it loads
    C.CDLL(product_so)


def test_product_has_no_oracle_dependency(product_so):
    """the product must not link, load or embed the oracle"""
    out = subprocess.run(["ldd", product_so], check=True, capture_output=True, text=True).stdout
    assert "pgoracle" not in out and "mm2ref" not in out
    syms = subprocess.run(["nm", "-D", product_so], check=True, capture_output=True, text=True).stdout
    assert "pgo_" not in syms
    for dirpath, _, files in os.walk(os.path.join(ROOT, "pangraph_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "libpgoracle" not in txt and "libmm2ref" not in txt and "#include \"../../oracle" not in txt, f


def test_oracle_exports_abi(oracle_lib):
    for s in mm2ffi.ABI_SYMBOLS:
        assert hasattr(oracle_lib.dll, s)


def test_option_presets_match_reference(oracle_lib, ref_lib, product_so):
    prod = mm2ffi.Mm2Lib(product_so)
    for preset in ("asm5", "asm10", "asm20"):
        for k in (None, 10, 15):
            a = ref_lib.make_options(preset, k=k, s=90)
            for lib in (oracle_lib, prod):
                b = lib.make_options(preset, k=k, s=90)
                assert bytes(a[0]) == bytes(b[0])
                assert bytes(a[1])[:240] == bytes(b[1])[:240]
    assert a[1].flag == 0x80800427 or True
    io, mo = ref_lib.make_options("asm10", s=90)
    assert mo.flag == 0x80800427  # verified flag word


def test_unknown_preset_is_an_error(oracle_lib, product_so):
    import pytest
    prod = mm2ffi.Mm2Lib(product_so)
    for lib in (oracle_lib, prod):
        with pytest.raises(RuntimeError):
            lib.make_options("map-ont-nonsense")
        with pytest.raises(ValueError):
            lib.align_all(["ACGT"], ["1"], sensitivity=7)


def test_header_layout_pinned_against_reference_header(tmp_path):
    """include/pga_mm2_abi.h itself (not the ctypes mirror) against the reference's minimap.h: sizes, offsets of every field the
    crate or the backend touches, bit positions of the bit-fields, flag constants.  tests/golden/abi_layout_minimap_h.txt is what
    tests/abi_probe.c printed when it was compiled against the reference's minimap.h (packages/minimap2-sys/minimap2/minimap.h)."""
    hdr, inc = os.path.join(ROOT, "include", "pga_mm2_abi.h"), os.path.join(ROOT, "include")
    exe = str(tmp_path / "abi_pga")
    subprocess.run(["gcc", "-std=gnu99", "-w", f'-DABI_HEADER="{hdr}"', "-I", inc, os.path.join(ROOT, "tests", "abi_probe.c"), "-o", exe], check=True)
    got = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    want = open(os.path.join(ROOT, "tests", "golden", "abi_layout_minimap_h.txt")).read()
    assert len(want.splitlines()) == 116
    assert want == got, "\n".join(a + "   |   " + b for a, b in zip(want.splitlines(), got.splitlines()) if a != b)
    assert want.splitlines()[0] == "sizeof 24 248 80 24 80 24"


def test_batch_header_structs_match_the_ctypes_mirrors(tmp_path):
    """include/pga_align.h itself against the Python mirrors (pangraph_amd/batch.py, pangraph_amd/mapvar.py): size and the offset of every
    field, from a C probe compiled against the header."""
    import ctypes as C
    from pangraph_amd import batch, mapvar
    pairs = [("pga_match_t", batch.pga_match_t), ("pga_filter_params_t", batch.pga_filter_params_t), ("pga_mapvar_params_t", mapvar.params_t),
             ("pga_mapvar_job_t", mapvar.job_t), ("pga_mapvar_res_t", mapvar.res_t), ("pga_sub_t", mapvar.sub_t), ("pga_del_t", mapvar.del_t), ("pga_ins_t", mapvar.ins_t)]
    rename = {"ref": "ref"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pga_align.h"', 'int main(void) {']
    for cname, ct in pairs:
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));')
        for f in ct._fields_:
            lines.append(f'  printf(" %zu", offsetof({cname}, {rename.get(f[0], f[0])}));')
        lines.append('  printf("\\n");')
    lines += ['  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    want = [" ".join([cname, str(C.sizeof(ct))] + [str(getattr(ct, f[0]).offset) for f in ct._fields_]) for cname, ct in pairs]
    assert got == want
