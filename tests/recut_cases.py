"""Shapes made to order for the conflict domains of the BIG launches (schedule.cpp: find_conflict_domains), shared by
test_recut_host.py and test_recut_gpu.py.  A plain helper module (no fixtures, no collection hooks).

As shape_cases.arrow: dense diagonal blocks that couple to rows of a dense trailing border -- here to rows that are
named, not drawn, because what a case is about is which rows of the border two sources share.  Every block is one
supernode (analysed with shape_cases.ZRELAX), a level below the border; with PARSY_BIG_MINK=16 every update is a BIG one.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

import shape_cases as SC

KNOB = "PARSY_BIG_RECUT"


def rows_matrix(blocks, border, seed):
    """(A, S): blocks = [(w, rows of the border)], values as shape_cases.arrow_layout makes them."""
    rng = np.random.default_rng(seed)
    nb = sum(w for w, _ in blocks)
    n = nb + border
    mask = np.zeros((n, n), dtype=bool)
    mask[nb:, nb:] = True
    c0 = 0
    for w, rows in blocks:
        rows = np.asarray(rows, dtype=int)
        assert len(np.unique(rows)) == len(rows) and rows.min() >= 0 and rows.max() < border
        mask[c0:c0 + w, c0:c0 + w] = True
        mask[np.ix_(rows + nb, np.arange(c0, c0 + w))] = True
        c0 += w
    mask = mask | mask.T
    V = np.tril(rng.uniform(-1.0, 1.0, (n, n)), -1)
    S = np.where(mask, V + V.T, 0.0)
    S[np.arange(n), np.arange(n)] = np.abs(S).sum(axis=1) + rng.uniform(0.5, 1.5, n)
    return SC.lower_csc(S), S


@dataclass(frozen=True)
class Case:
    name: str
    blocks: tuple          # (w, rows of the border)
    border: int
    intent: str
    seed: int
    env: dict = field(default_factory=dict)

    @property
    def n(self) -> int:
        return sum(w for w, _ in self.blocks) + self.border


_BIG = {"PARSY_BIG_MINK": "16"}
_EVEN = tuple(range(0, 256, 2))
CASES = [
    Case("one_source", ((136, _EVEN),), 256, "(a) one source of K = 136 coupled to every other row of a 256-wide target", 31, _BIG),
    Case("same_rows", ((136, _EVEN), (72, _EVEN)), 256, "(b) two sources with the same rows in the target", 32, _BIG),
    Case("overlap", ((136, _EVEN), (72, tuple(range(128)))), 256,
         "(c) two sources whose rows overlap partially: one domain, not of one row set -- the tile cut stays", 33, _BIG),
    Case("two_pieces", ((136, _EVEN),), 256, "(d) a target of two pieces of 128 columns, the source's rows in both", 34,
         {**_BIG, "PARSY_PIECE_WIDTH": "128"}),
    Case("remainders", ((40, tuple(range(0, 3 * 133, 3))), (48, tuple(range(1, 3 * 144, 3))), (56, tuple(range(2, 3 * 145, 3)))), 435,
         "(e) three sources of 128 + 5, 128 + 16 and 128 + 17 rows that share no column: three domains of one launch", 35, _BIG),
]
CASE_BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
assert all(c.n <= 1000 for c in CASES)

_BUILT = {}


def build(case):
    """(A, S, sym), made once per process and left unchanged."""
    from parsy_bench_amd import inspector as I
    if case.name not in _BUILT:
        A, S = rows_matrix(case.blocks, case.border, case.seed)
        _BUILT[case.name] = (A, S, I.analyze(A, None, zrelax=SC.ZRELAX))
    return _BUILT[case.name]


def set_env(monkeypatch, case, recut):
    SC.set_env(monkeypatch, {**case.env, KNOB: "1" if recut else "0"})


TASK_FIELDS = ("launch", "piece", "domain", "row0", "col0", "entries", "dense", "frag_chunks", "chunks", "dense_chunks")


def big_tasks(plan) -> np.ndarray:
    """parsy_debug_big_tasks: one row of TASK_FIELDS per BIG task of the plan."""
    from parsy_bench_amd import _native as N
    lib = N.lib()
    lib.parsy_debug_big_tasks.restype = C.c_int64
    lib.parsy_debug_big_tasks.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    n = lib.parsy_debug_big_tasks(plan._h, None, 0)
    out = np.zeros((n, len(TASK_FIELDS)), dtype=np.int64)
    assert lib.parsy_debug_big_tasks(plan._h, out.ctypes.data, n) == n
    return out


def big_windows(plan) -> np.ndarray:
    """parsy_debug_big_windows: (task, launch, K, rows, columns, ia, ja, source, dense) per BIG entry."""
    from parsy_bench_amd import _native as N
    lib = N.lib()
    lib.parsy_debug_big_windows.restype = C.c_int64
    lib.parsy_debug_big_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    n = lib.parsy_debug_big_windows(plan._h, None, 0)
    out = np.zeros((n, 9), dtype=np.int64)
    assert lib.parsy_debug_big_windows(plan._h, out.ctypes.data, n) == n
    return out
