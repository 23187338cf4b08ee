"""Host-side (no GPU): what the re-cut of the conflict domains (schedule.cpp: find_conflict_domains) changes in the BIG
launches -- per launch, for PARSY_BIG_RECUT=0 and 1: tasks, entries, mean fill (issued fragments per 16-wide k chunk / 64),
issued fragment-chunks, the longest dense and the longest ragged part of a task (16-wide k chunks) and, with the knob on, the tasks of re-cut domains.
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
lib.parsy_debug_big_tasks.restype = C.c_int64
lib.parsy_debug_big_tasks.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]


def tasks_of(recut):
    os.environ["PARSY_BIG_RECUT"] = str(recut)
    t0 = time.perf_counter()
    plan = api.Plan(sym, -1)
    sec = time.perf_counter() - t0
    n = lib.parsy_debug_big_tasks(plan._h, None, 0)
    out = np.zeros((n, 10), dtype=np.int64)
    lib.parsy_debug_big_tasks(plan._h, out.ctypes.data, n)
    return out, sec, plan.info


def per_launch(t):
    rows = {}
    for lid in np.unique(t[:, 0]):
        m = t[t[:, 0] == lid]
        rows[int(lid)] = (len(m), int(m[:, 5].sum()), m[:, 7].sum() / max(64.0 * m[:, 8].sum(), 1.0), int(m[:, 7].sum()),
                          int(m[:, 9].max()), int((m[:, 8] - m[:, 9]).max()), int((m[:, 2] > 0).sum()), int(m[:, 6].sum()))
    return rows


off, sec_off, info_off = tasks_of(0)
on, sec_on, info_on = tasks_of(1)
print(f"{name}: n = {sym.n}; plan built in {sec_off:.2f} s (PARSY_BIG_RECUT=0), {sec_on:.2f} s (1)")
for what, t, info in (("PARSY_BIG_RECUT=0", off, info_off), ("PARSY_BIG_RECUT=1", on, info_on)):
    print(f"{what}: {len(t)} tasks, {int(t[:, 5].sum())} entries ({int(t[:, 6].sum())} dense, {info['dense_strip_entries']} with strips), "
          f"{int(t[:, 7].sum())} issued fragment-chunks, mean fill {t[:, 7].sum() / (64.0 * t[:, 8].sum()):.3f}, "
          f"tasks of re-cut domains {int((t[:, 2] > 0).sum())}")
a, b = per_launch(off), per_launch(on)
total = sum(r[3] for r in a.values())
print("launch (source level, kind) | knob 0: tasks entries dense fill fragment-chunks longest-dense longest-ragged | knob 1: the same, re-cut tasks")
for lid in sorted(a):
    if a[lid][3] < 0.002 * total and b.get(lid, a[lid])[6] == 0:
        continue
    x, y = a[lid], b[lid]
    print(f"{lid >> 1:3d} {'push' if lid & 1 else 'next'} | {x[0]:6d} {x[1]:6d} {x[7]:6d} {x[2]:.2f} {x[3]:10d} {x[4]:5d} {x[5]:5d} | "
          f"{y[0]:6d} {y[1]:6d} {y[7]:6d} {y[2]:.2f} {y[3]:10d} {y[4]:5d} {y[5]:5d} {y[6]:6d}")
