"""pga_tile_scan.h without a GPU: the three kernels of the two-level exclusive scan that the graph entries share, on their own, in a
stand-alone program under the host sanitizers (tests/emu/tile_scan_emu.cpp)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_tile_scan_kernels_under_emulation_and_sanitizers(tmp_path):
    """both word types against a scalar prefix sum: 0, 1, 1023, 1024, 1025 and 1024 * 256 + 1 items, one and seven quantities, grids of 1, 2
    and one workgroup per tile, 64-bit values that need their upper half, and 2 * 256 + 3 tile sums fed to the second level directly"""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "tile_scan_emu")
    subprocess.run([cxx, "-std=c++17", "-g1", "-O1", "-DPGA_EMU", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "emu", "tile_scan_emu.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    noise = [ln for ln in r.stderr.splitlines() if ln and "doesn't fully support makecontext/swapcontext" not in ln]
    assert r.returncode == 0 and r.stdout.startswith("tile_scan_emu OK") and not noise, (r.returncode, r.stdout, r.stderr)
