"""Host-side (no GPU): what the cuts of the conflict domains (schedule.cpp: find_conflict_domains) change in the BIG
launches -- per launch, for PARSY_BIG_RECUT=0, 1, 2 and 3: tasks, entries, dense entries, mean fill (issued fragments per
16-wide k chunk / 64), issued fragment-chunks, the longest dense and the longest ragged part of a task (16-wide k chunks),
the tasks of domains cut in their own row order (knob 1 on) and in intervals of the target's positions (2 on), and the
issued work by the model the domains decide by (schedule.hpp: kIssue*; ms, and ms / 512 workgroup slots: what the launch
takes if its tasks pack perfectly), with the longest task by that model (us).
Issued fragment-chunks: see parsy_debug_big_tasks (capi_exec.hip).  Usage: recut_stats.py [WORKLOAD]"""
import ctypes as C
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from parsy_bench_amd import _native as N, api, inspector as I, matrices as M  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "flan"
A, perm = M.workload(name)
sym = I.analyze(A, perm)
lib = N.lib()
for fn in (lib.parsy_debug_big_tasks, lib.parsy_debug_big_windows):
    fn.restype = C.c_int64
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
INTERVAL = 1 << 30                                   # schedule.hpp: kIntervalDomain
DENSE_NS, STRIP_NS, RAGGED_NS, FRAGMENT_NS = 2090, 260, 1000, 60   # schedule.hpp: kIssue*
SLOTS = 512                                          # schedule.hpp: kIssueSlots
KNOBS = (0, 1, 2, 3)


def table(fn, plan, width):
    n = fn(plan._h, None, 0)
    out = np.zeros((n, width), dtype=np.int64)
    fn(plan._h, out.ctypes.data, n)
    return out


def tasks_of(knob):
    """The rows of parsy_debug_big_tasks, with an 11th column: the task's issued ns by the model."""
    os.environ["PARSY_BIG_RECUT"] = str(knob)
    t0 = time.perf_counter()
    plan = api.Plan(sym, -1)
    sec = time.perf_counter() - t0
    t, w = table(lib.parsy_debug_big_tasks, plan, 10), table(lib.parsy_debug_big_windows, plan, 9)
    K, m, n, dense = w[:, 2], w[:, 3], w[:, 4], w[:, 8] != 0
    frag = -(-m // 16) * -(-n // 16)
    ns = np.where(dense, -(-K // 8) * DENSE_NS, -(-K // 16) * (RAGGED_NS + FRAGMENT_NS * frag))
    per_task = np.bincount(w[:, 0], weights=ns, minlength=len(t))
    # strips ride in their block's entry: 8 fragment-chunks = two 8-wide chunks each
    ragged_fc = np.bincount(w[:, 0], weights=np.where(dense, 0, -(-K // 16) * frag), minlength=len(t))
    per_task += (t[:, 7] - 64 * t[:, 9] - ragged_fc) / 8 * 2 * STRIP_NS
    return np.column_stack([t, np.rint(per_task).astype(np.int64)]), sec, plan.info


def per_launch(t):
    rows = {}
    for lid in np.unique(t[:, 0]):
        m = t[t[:, 0] == lid]
        own, ival = (m[:, 2] > 0) & (m[:, 2] < INTERVAL), m[:, 2] >= INTERVAL
        rows[int(lid)] = (len(m), int(m[:, 5].sum()), int(m[:, 6].sum()), m[:, 7].sum() / max(64.0 * m[:, 8].sum(), 1.0), int(m[:, 7].sum()),
                          int(m[:, 9].max()), int((m[:, 8] - m[:, 9]).max()), int(own.sum()), int(ival.sum()),
                          m[:, 10].sum() / 1e6, m[:, 10].sum() / 1e6 / SLOTS, m[:, 10].max() / 1e3)
    return rows


runs = {k: tasks_of(k) for k in KNOBS}
print(f"{name}: n = {sym.n}; plan built in " + ", ".join(f"{runs[k][1]:.2f} s (PARSY_BIG_RECUT={k})" for k in KNOBS))
for k in KNOBS:
    t, _, info = runs[k]
    print(f"PARSY_BIG_RECUT={k}: {len(t)} tasks, {int(t[:, 5].sum())} entries ({int(t[:, 6].sum())} dense, {info['dense_strip_entries']} with strips), "
          f"{int(t[:, 7].sum())} issued fragment-chunks, mean fill {t[:, 7].sum() / (64.0 * t[:, 8].sum()):.3f}, "
          f"tasks of own-order domains {int(((t[:, 2] > 0) & (t[:, 2] < INTERVAL)).sum())}, of interval domains {int((t[:, 2] >= INTERVAL).sum())}, "
          f"issued by the model {t[:, 10].sum() / 1e6:.1f} ms of work = {t[:, 10].sum() / 1e6 / SLOTS:.2f} ms on {SLOTS} slots")
rows = {k: per_launch(runs[k][0]) for k in KNOBS}
print("launches that a knob changes (a knob's row is left out where it equals the knob before)")
print("launch (source level, kind) | per knob: tasks entries dense fill fragment-chunks longest-dense longest-ragged own-order-tasks interval-tasks "
      "model-ms model-ms/512 longest-task-us")
for lid in sorted(rows[0]):
    # the launches a knob changes; of a knob's rows those that differ from the knob before
    if all(rows[k].get(lid) == rows[0][lid] for k in KNOBS):
        continue
    for k in KNOBS:
        x = rows[k][lid]
        if k and x == rows[k - 1][lid]:
            continue
        print(f"{lid >> 1:3d} {'push' if lid & 1 else 'next'} knob {k} | {x[0]:6d} {x[1]:6d} {x[2]:6d} {x[3]:.2f} {x[4]:10d} {x[5]:5d} {x[6]:5d} "
              f"{x[7]:6d} {x[8]:6d} {x[9]:8.2f} {x[10]:7.3f} {x[11]:7.1f}")
