"""bench.py without --full: the line of a plain run and what --dump-outputs writes of the step it timed, on a small build (12 genomes of
150 kb).  Two runs with different numbers of steps write the same outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _plain_run(out_dir, steps, warmup):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--genomes", "12", "--length", "150000", "--steps", str(steps),
           "--warmup", str(warmup), "--dump-outputs", str(out_dir)]
    # (a process of its own beside the pytest process, whose block cache may hold much of the device: it keeps to a fifth of it)
    r = subprocess.run(cmd, env=dict(os.environ, PGA_MEM_SHARE="0.2"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_dumps_the_records_of_its_last_timed_step(tmp_path):
    a = _plain_run(tmp_path / "a", 2, 1)
    assert a["steps"] == 2 and a["warmup"] == 1 and a["ms_per_step"] > 0 and a["value"] > 0
    assert a["unit"] == "Gbp/s" and a["higher_is_better"] is True and a["dtype"] == "u8"
    assert "cpu_baseline" not in a and a["build_sha256"] is None and a["parity_checked_calls"] == 0
    out = {f: np.load(tmp_path / "a" / f"{f}.npy") for f in ("records_per_call", "matches", "cigars")}
    assert all(v.dtype == np.float64 for v in out.values())
    assert sum(v.nbytes for v in out.values()) <= 64 << 20
    m = out["matches"]
    assert len(m) == int(out["records_per_call"].sum()) == a["n_matches_gathered"] > 50
    assert np.all(np.diff(m[:, 0]) >= 0) and len(out["cigars"]) == int(m[:, -1].sum())
    b = _plain_run(tmp_path / "b", 1, 0)
    for f in out:
        assert np.array_equal(out[f], np.load(tmp_path / "b" / f"{f}.npy")), f
