"""Sequences for the sketch tap pga_stage_sketch, aimed at the edges of the three sketch kernels (pga_sketch.hip): the 2048-base tile and its halo,
the staging slab and its retries, runs of clean bases around w + k - 1, every byte value as a letter, and (w, k) at the borders between the
kernels.  The expectation is the reference's mm_sketch; it asserts len > 0, so an empty sequence expects no minimizer.

A case is one call of the tap: a batch of sequences (bytes) under one (w, k), with pins: kernel -- the route counter that must answer;
n_mz -- {sequence: number of minimizers}.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from stagebind import mm128_t, mm128_v, _libc

TILE = 2048                         # SK_TILE: bases per workgroup of the tile kernels
WK3 = [(19, 19), (10, 19), (5, 11)]
# which kernel sketch_all picks: the tile kernels need an odd k and w + k <= 64; eight positions per thread with w = 19 or 10 and 2k + 13 <= 64
KERNEL = {(19, 19): "sk_tiles8_19", (10, 19): "sk_tiles8_10", (5, 11): "sk_tiles", (19, 25): "sk_tiles8_19", (19, 27): "sk_tiles", (10, 25): "sk_tiles8_10",
          (10, 27): "sk_tiles", (37, 27): "sk_tiles", (38, 27): "sk_serial", (63, 1): "sk_tiles", (1, 19): "sk_tiles", (255, 28): "sk_serial", (19, 28): "sk_serial"}


@dataclass
class Sk:
    name: str
    seqs: list
    w: int
    k: int
    pins: dict = field(default_factory=dict)


def rnd(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes())


def ref_minimizers(dll, seq: bytes, w, k, rid):
    if len(seq) == 0:
        return []
    v = mm128_v(0, 0, None)
    dll.mm_sketch.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.POINTER(mm128_v)]
    dll.mm_sketch.restype = None
    dll.mm_sketch(None, seq, len(seq), w, k, rid, 0, C.byref(v))
    out = [(v.a[i].x, v.a[i].y) for i in range(v.n)]
    if v.a:
        _libc.free(v.a)
    return out


def oracle_minimizers(dll, seq: bytes, w, k, rid):
    if len(seq) == 0:
        return []
    out, cap = C.POINTER(mm128_t)(), C.c_size_t(0)
    dll.pgo_sketch.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.POINTER(C.POINTER(mm128_t)), C.c_size_t, C.POINTER(C.c_size_t)]
    dll.pgo_sketch.restype = C.c_size_t
    n = dll.pgo_sketch(seq, len(seq), w, k, rid, C.byref(out), 0, C.byref(cap))
    res = [(out[i].x, out[i].y) for i in range(n)]
    if out:
        _libc.free(out)
    return res


def product_minimizers(dll, seqs, w, k):
    n = len(seqs)
    arr = (C.c_char_p * n)(*seqs)
    lens = (C.c_uint32 * n)(*[len(b) for b in seqs])
    mz, off = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
    dll.pga_stage_sketch.restype = C.c_int
    dll.pga_stage_sketch.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    if dll.pga_stage_sketch(n, arr, lens, w, k, C.byref(mz), C.byref(off)) != 0:
        dll.pga_last_error.restype = C.c_char_p
        raise RuntimeError(dll.pga_last_error().decode())
    offs = [off[i] for i in range(n + 1)]
    res = [[(mz[2 * j], mz[2 * j + 1]) for j in range(offs[i], offs[i + 1])] for i in range(n)]
    dll.pga_free.argtypes = [C.c_void_p]
    dll.pga_free(mz)
    dll.pga_free(off)
    return res


def slab_retries(S, fullest):
    """launches repeated for a fullest tile of that many records: the slab holds TILE / 6 records per tile with w >= 16, else TILE / 3, and grows
    fourfold until the tile fits"""
    cap, r = TILE // 6 if S.w >= 16 else TILE // 3, 0
    while fullest > cap:
        cap *= 4
        r += 1
    return r


def expected_routes(S, want):
    """the counters one call must leave: want = the reference's minimizers per sequence.  (kernel, launches of the serial kernel, fewest and most
    retries of the slab).  A tile counts the records EMITTED at its positions, which lie up to w positions in front of them, so the fullest
    tile by position fixes the count only to within w + 1 records; a case pins the exact number where it is built for it."""
    kern = KERNEL[(S.w, S.k)]
    if not S.seqs or (kern != "sk_serial" and not any(len(s) for s in S.seqs)):
        return None, 0, 0, 0
    if kern == "sk_serial":
        return kern, 2, 0, 0
    fullest = max([0] + [int(np.bincount(np.array([(y & 0xffffffff) >> 1 for _, y in m], dtype=np.int64) // TILE).max()) for m in want if m])
    return kern, 0, slab_retries(S, max(fullest - S.w - 1, 0)), slab_retries(S, fullest + S.w + 1)


def routes_failures(S, want, routes):
    """what the counters of one call differ in from expected_routes, as a list of strings"""
    kern, n_serial, lo, hi = expected_routes(S, want)
    bad = []
    for r in ("sk_tiles8_19", "sk_tiles8_10", "sk_tiles", "sk_serial"):
        exp = 0 if r != kern else n_serial if r == "sk_serial" else routes["sk_retry"] + 1
        if routes[r] != exp:
            bad.append(f"{r}: {routes[r]} launches, expected {exp}")
    if not lo <= routes["sk_retry"] <= hi:
        bad.append(f"{routes['sk_retry']} retries of the staging slab, expected {lo} to {hi}")
    if "retries" in S.pins and routes["sk_retry"] != S.pins["retries"]:
        bad.append(f"{routes['sk_retry']} retries of the staging slab, pinned {S.pins['retries']}")
    return bad


def repeat_cases():
    out = []
    for w, k in WK3:
        out.append(Sk(f"repeats/homopolymer ({w},{k})", [b"A" * 5000], w, k, dict(kernel=KERNEL[(w, k)], retries=2 if w >= 16 else 1)))
        out.append(Sk(f"repeats/period2 ({w},{k})", [b"AC" * 2100, b"GT" * 1030 + b"G"], w, k, dict(kernel=KERNEL[(w, k)])))
        out.append(Sk(f"repeats/period3 ({w},{k})", [b"ACG" * 1400, b"TTG" * 700 + b"TT"], w, k, dict(kernel=KERNEL[(w, k)])))
    return out


def n_cases():
    out = []
    for w, k in WK3:
        rng = np.random.default_rng(w * 100 + k)
        base = rnd(rng, 4300)
        seqs = []
        for p in (TILE - 1, TILE, TILE - (w + k - 1), TILE + (w + k - 1), TILE - (w + k), TILE + (w + k) - 2):
            seqs.append(base[:p] + b"N" + base[p + 1:])
        seqs.append(base[:TILE - 1] + b"NN" + base[TILE + 1:])
        out.append(Sk(f"n/around_2048 ({w},{k})", seqs, w, k))
    return out


def clean_run_cases():
    """runs of exactly w + k - 2 (no minimizer where an N follows), w + k - 1 (the first window) and w + k clean bases"""
    out = []
    for w, k in WK3:
        rng = np.random.default_rng(w * 1000 + k)
        for r in (w + k - 2, w + k - 1, w + k):
            run = rnd(rng, r)
            seqs = [run + b"N" * 40,                                                    # at the start
                    b"N" * (TILE - r // 2) + run + b"N" * 60,                            # across 2048
                    b"N" * (TILE - r) + run + b"N" * 60,                                 # ending at 2047
                    b"N" * TILE + run + b"N" * 60,                                       # starting at 2048
                    b"N" * 300 + run,                                                    # at the end
                    run]                                                                 # the whole sequence
            # (a run that ends with the sequence leaves its minimum at the end whatever its length, sketch.c:141-142: no pin for the last two)
            out.append(Sk(f"runs/r={r} ({w},{k})", seqs, w, k, dict(n_mz={i: 0 for i in range(4)}) if r < w + k - 1 else {}))
    return out


def length_cases():
    out = []
    for w, k in WK3:
        rng = np.random.default_rng(w * 7 + k)
        lens = [0, 1, k - 1, k, k + w - 2, k + w - 1, k + w, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1]
        out.append(Sk(f"lengths/all ({w},{k})", [rnd(rng, n) for n in lens], w, k, dict(n_mz={0: 0, 1: 0, 2: 0})))
        for n in lens[1:]:
            out.append(Sk(f"lengths/alone len={n} ({w},{k})", [rnd(rng, n)], w, k))
    return out


def empty_cases():
    out = []
    for w, k in WK3 + [(19, 28)]:
        rng = np.random.default_rng(w + k)
        a, b = rnd(rng, 700), rnd(rng, TILE + 300)
        out.append(Sk(f"empty/first_between_last ({w},{k})", [b"", a, b"", b"", b, b""], w, k, dict(n_mz={0: 0, 2: 0, 3: 0, 5: 0})))
        out.append(Sk(f"empty/all ({w},{k})", [b"", b""], w, k, dict(n_mz={0: 0, 1: 0})))
    return out


def halo_cases():
    """the second sequence starts at every residue mod 16 of the packed store, behind a sequence that ends in clean bases: the halo in front of a
    sequence's first tile must not read the neighbour"""
    out = []
    for w, k in WK3:
        rng = np.random.default_rng(w * 31 + k)
        for r in range(16):
            out.append(Sk(f"halo/start_mod_16={r} ({w},{k})", [rnd(rng, 96 + r), rnd(rng, TILE + 150), rnd(rng, w + k + r), rnd(rng, 333)], w, k))
    return out


def byte_cases():
    """all 256 byte values as letters: A C G T U in both cases are bases, everything else breaks the run (sketch.c:9-26)"""
    out = []
    for w, k in WK3:
        rng = np.random.default_rng(w * 3 + k)
        seq = b"".join(rnd(rng, w + k + 4) + bytes([v]) for v in range(256)) + rnd(rng, 50)
        low = bytes(rng.choice(np.frombuffer(b"ACGTUacgtu", dtype=np.uint8), 3000).tobytes())
        out.append(Sk(f"bytes/all_256 ({w},{k})", [seq, low], w, k))
    return out


def border_cases():
    out = []
    rng = np.random.default_rng(99)
    base = rnd(rng, 2 * TILE + 200)
    seqs = [base, base[:1500] + b"N" + base[1501:3000] + b"A" * 90 + base[3090:3500], rnd(rng, 70), b"ACGT" * 40]
    for w, k in ((19, 25), (19, 27), (10, 25), (10, 27), (37, 27), (38, 27), (63, 1), (1, 19), (255, 28), (19, 28)):
        out.append(Sk(f"borders/({w},{k})", seqs, w, k, dict(kernel=KERNEL[(w, k)])))
    return out


FAMILIES = {"repeats": repeat_cases, "n": n_cases, "runs": clean_run_cases, "lengths": length_cases, "empty": empty_cases, "halo": halo_cases, "bytes": byte_cases,
            "borders": border_cases}
_CACHE = {}


def family(name):
    if name not in _CACHE:
        _CACHE[name] = FAMILIES[name]()
    return _CACHE[name]
