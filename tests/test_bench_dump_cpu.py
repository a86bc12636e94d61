"""bench.py --dump-outputs on CPU: what dump_outputs writes from the per-batch results of a step (the form bench.py's parity check reads),
on hand-made records.  CPU only."""
import importlib.util
import os

import numpy as np

from conftest import ROOT
from pangraph_amd.dist import MATCH_DTYPE


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Task:
    def __init__(self, tid):
        self.tid = tid


def _word(tid, r, k):
    return (tid * 1000 + r * 10 + k) << 4 | 7


def _batch(tids, n_recs, rng):
    """one batch's result: records with group = index into the batch's tasks, each with a CIGAR of 1..4 words that name it"""
    recs, pool = [], []
    for gi, (tid, n) in enumerate(zip(tids, n_recs)):
        for r in range(n):
            m = np.zeros(1, MATCH_DTYPE)
            m["group"], m["qry"], m["ref"], m["divergence"] = gi, r, tid, 0.125 * r
            k = int(rng.integers(1, 5))
            m["cigar_off"], m["n_cigar"] = len(pool), k
            pool += [_word(tid, r, j) for j in range(k)]
            recs.append(m)
    return [_Task(t) for t in tids], np.concatenate(recs), np.asarray(pool, np.uint32), None


def _load(d):
    return {f: np.load(os.path.join(d, f + ".npy")) for f in ("records_per_call", "matches", "cigars")}


def _check_cigars(out):
    cg, pos = out["cigars"].astype(np.int64), 0
    for row in out["matches"]:
        tid, r, n = int(row[0]), int(row[1]), int(row[-1])
        assert cg[pos:pos + n].tolist() == [_word(tid, r, j) for j in range(n)]
        pos += n
    assert pos == len(cg)


def test_dump_is_in_task_order_whatever_order_the_batches_finished(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(3)
    results = [_batch([3, 0], [2, 3], rng), _batch([1, 2], [1, 0], rng), _batch([4], [4], rng)]
    bench.dump_outputs(results, 5, str(tmp_path / "a"), 7)
    bench.dump_outputs(results[::-1], 5, str(tmp_path / "b"), 7)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    for f in a:
        assert a[f].dtype == np.float64 and np.array_equal(a[f], b[f]), f
    assert a["records_per_call"].tolist() == [3, 1, 0, 2, 4]
    m = a["matches"]
    assert m.shape == (10, 1 + len(bench.DUMP_FIELDS))
    assert m[:, 0].tolist() == [0, 0, 0, 1, 3, 3, 4, 4, 4, 4]
    assert m[:, 1].tolist() == [0, 1, 2, 0, 0, 1, 0, 1, 2, 3]                        # a call's records keep the aligner's order
    assert m[:, 1 + bench.DUMP_FIELDS.index("divergence")].tolist() == [0.125 * r for r in m[:, 1]]
    _check_cigars(a)


def test_dump_of_a_gathered_list_takes_each_call_once(tmp_path):
    """N > 1: rank 0 holds gathered lists whose group is the global task id; `covered` says which calls a list speaks for"""
    bench = _bench()
    tasks, rec, pool, _ = _batch([0, 1, 2, 3, 4], [1, 2, 1, 1, 1], np.random.default_rng(5))
    bench.dump_outputs([(tasks, rec, pool, [1, 3, 4]), (tasks, rec, pool, [0, 2])], 5, str(tmp_path), 7)
    out = _load(str(tmp_path))
    assert out["records_per_call"].tolist() == [1, 2, 1, 1, 1]
    assert out["matches"][:, 0].tolist() == [0, 1, 1, 2, 3, 4]
    _check_cigars(out)


def test_dump_over_the_budget_keeps_a_fixed_sample_of_whole_calls(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(9)
    results = [_batch(list(range(i, i + 10)), [5] * 10, rng) for i in range(0, 40, 10)]
    bench.dump_outputs(results, 40, str(tmp_path / "a"), 11, budget=4000)
    bench.dump_outputs(results[::-1], 40, str(tmp_path / "b"), 11, budget=4000)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert a["records_per_call"].tolist() == [5] * 40                                # the counts of every call stay
    assert a["matches"].nbytes + a["cigars"].nbytes + a["records_per_call"].nbytes <= 4000
    calls = sorted(set(a["matches"][:, 0].astype(int).tolist()))
    assert 0 < len(calls) < 40 and len(a["matches"]) == 5 * len(calls)                # whole calls only
    for f in a:
        assert np.array_equal(a[f], b[f]), f
    _check_cigars(a)
