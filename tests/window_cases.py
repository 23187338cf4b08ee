"""Shapes made to order for the interval cut of the BIG launches' conflict domains (schedule.cpp: find_conflict_domains,
interval_bounds), shared by test_window_host.py and test_window_gpu.py.  A plain helper module (no fixtures, no collection
hooks).  Built as recut_cases.py builds its own: dense diagonal blocks, one supernode each, a level below a dense border
whose rows they name; with PARSY_BIG_MINK=16 every update is a BIG one.  Here the sources of a case share columns of the
target and their rows differ: one conflict domain that the knob's value 1 leaves on the tile grid.

PARSY_BIG_RECUT: 0 = the tile cut, 1 = domains of one row set in their own order, 2 = the other domains in intervals of the
target's positions where that issues less and the tail guard holds, 3 = as 2 without the guard.  Every plan here sets it:
unset, a job this small keeps 1.
"""
from __future__ import annotations

import recut_cases as RC
import shape_cases as SC

KNOB = RC.KNOB
KNOBS = (0, 1, 2, 3)
INTERVAL = 1 << 30   # schedule.hpp: kIntervalDomain -- interval domains are numbered from here

_BIG = {"PARSY_BIG_MINK": "16"}
_A145 = tuple(range(1, 3 * 145, 3))
CASES = [
    RC.Case("nested", ((136, tuple(range(0, 256, 2))), (72, tuple(range(0, 256, 4)))), 256,
            "(a) the rows of B (every fourth) are rows of A (every other) of a 256-wide target: one interval", 41, _BIG),
    RC.Case("off_grid", ((40, _A145), (48, tuple(range(100, 228)))), 435,
            "(b) A on rows 1, 4, 7, .. (145 of them), B on 128 consecutive rows: A's 129th row opens an interval at 385", 42, _BIG),
    RC.Case("piece_end", ((136, tuple(range(0, 512, 2))), (72, tuple(range(0, 512, 4)))), 512,
            "(c) a target of four pieces of 128 columns, both sources' rows in all of them", 43, {**_BIG, "PARSY_PIECE_WIDTH": "128"}),
    RC.Case("chain3", ((136, tuple(r for r in range(256) if r % 4 in (0, 1))), (72, tuple(r for r in range(256) if r % 4 in (1, 2))),
                       (40, tuple(r for r in range(256) if r % 4 in (2, 3)))), 256,
            "(d) A shares columns with B and B with C, A and C share none: one domain of three row sets", 44, _BIG),
    RC.Case("nested_all_dense", ((136, tuple(range(0, 256, 2))), (72, tuple(range(0, 256, 4)))), 256,
            "(e) as (a) where k_chol_dense takes every entry (PARSY_BIG_DENSE=4): a tile's task is as long as the one interval "
            "task, so the tail guard lets the intervals pass", 41, {**_BIG, "PARSY_BIG_DENSE": "4"}),
]
CASE_BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
assert all(c.n <= 1000 for c in CASES)

build = RC.build
big_tasks = RC.big_tasks
big_windows = RC.big_windows
TASK_FIELDS = RC.TASK_FIELDS


def case_of(name):
    return CASE_BY_NAME[name] if name in CASE_BY_NAME else RC.CASE_BY_NAME[name]


def set_env(monkeypatch, case, knob):
    SC.set_env(monkeypatch, {**case.env, KNOB: str(knob)})
