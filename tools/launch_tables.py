"""The launch tables (parsy_debug_launches: one row of parsy::Launch's fields per launch of the factorization, the forward
and the backward solve) of host-only plans, one SHA-256 per plan over the three tables -- what a change of the launch
record is compared by (profiles/launch_record_evidence.md).  A change of the schedule builder is compared by
tools/schedule_digests.py, which hashes every array of the schedule, these tables among them.  Needs no device.
Usage: launch_tables.py [--rows]     (--rows: the tables themselves)"""
import ctypes as C
import hashlib
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
from parsy_bench_amd import _native as N, inspector as I, matrices as M   # noqa: E402
import shape_cases as SC   # noqa: E402
from conftest import shard_masks   # noqa: E402

FIELDS = 15
lib = N.lib()
lib.parsy_debug_launches.restype = C.c_int64
lib.parsy_debug_launches.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]

NAMED = ("tiny2d", "small3d", "mid3d", "lap30", "ex15", "nd24k", "13x13x13:27")
KNOBS = ({"PARSY_SUBTREES": "0"}, {"PARSY_FORCE_UNFUSED": "1"}, {"PARSY_CHAIN_SPLIT": "2"}, {"PARSY_BSOLVE_BELOW": "2"},
         {"PARSY_SOLVE_ONE": "0"})
CLEAR = set(SC.VARIABLES) | {k for e in KNOBS for k in e}
_SYM = {}


def sym_of(name):
    if name not in _SYM:
        A, perm = M.workload(name)
        _SYM[name] = I.analyze(A, perm)
    return _SYM[name]


def tables(sym, env, mask=None):
    for k in CLEAR:
        os.environ.pop(k, None)
    os.environ.update(env)
    h = lib.parsy_plan_from_symbolic(sym._handle, -1)
    assert h, N.last_error()
    try:
        if mask is not None:
            assert lib.parsy_plan_set_active(h, N.ptr(np.ascontiguousarray(mask))) == 0, N.last_error()
        out = []
        for which in range(3):
            n = lib.parsy_debug_launches(h, which, None, 0)
            t = np.zeros((n, FIELDS), dtype=np.int32)
            assert lib.parsy_debug_launches(h, which, t.ctypes.data, n) == n
            out.append(t)
        return out
    finally:
        lib.parsy_plan_destroy(h)
        for k in env:
            del os.environ[k]


def plans():
    for name in NAMED:
        yield name, sym_of(name), {}, None
    for case in SC.CASES:
        yield "shape:" + case.name, SC.build(case)[2], dict(case.env), None
    for name in ("mid3d", "lap30"):
        for env in KNOBS:
            yield name + " " + " ".join(f"{k}={v}" for k, v in env.items()), sym_of(name), env, None
    for name in ("small3d", "lap30"):
        for r, mask in enumerate(shard_masks(sym_of(name), 2)):
            yield f"{name} shard {r}/2", sym_of(name), {}, mask


if __name__ == "__main__":
    for label, sym, env, mask in plans():
        ts = tables(sym, env, mask)
        digest = hashlib.sha256(b"".join(np.int64(t.shape[0]).tobytes() + t.tobytes() for t in ts)).hexdigest()
        print(f"{digest[:16]}  {ts[0].shape[0]:5d} {ts[1].shape[0]:4d} {ts[2].shape[0]:4d}  {label}")
        if "--rows" in sys.argv:
            for which, t in zip(("chol", "solve", "bsolve"), ts):
                for row in t:
                    print("   ", which, *row)
