"""Digests of whole schedules (parsy_debug_schedule_digest: one 64-bit FNV-1a per data member of parsy::Schedule,
csrc/schedule_digest.hpp) of host-only plans -- what a change of the schedule builder that is meant to leave every
schedule as it was is compared by (profiles/schedule_passes_evidence.md).  The launch tables (tools/launch_tables.py) are
three of the fields; a wave entry, a split range or a slot number can move while they stay equal.  Needs no device.
The plans: those of launch_tables.plans(); the knob rows of tests/test_schedule_host.py; every knob of the builder that
those leave out, on lap30 and nd24k with pieces and BIG launches forced; parabolic_fem and 72x72x72 as they come; supernode
and piece masks, each followed by the plan with the mask taken off again.
Usage: schedule_digests.py [--fields] [--part K/N]   (one line per plan; --fields: one line per plan and field;
                                                      --part: plans K, K + N, ... of the list, to run N processes side by side)
       schedule_digests.py --device D NAME ...       (plans of named workloads on device D, one line per field, labelled
                                                      as tests/schedule_digest_check.cpp labels its own for 256 compute units)"""
import ctypes as C
import hashlib
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tools")]
import launch_tables as LT   # noqa: E402  (puts tests/ on the path too)
from parsy_bench_amd import _native as N, api   # noqa: E402
from conftest import shard_masks   # noqa: E402

lib = N.lib()
lib.parsy_debug_schedule_digest.restype = C.c_int
lib.parsy_debug_schedule_digest.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_char_p)]

FORCED = {"PARSY_PIECE_WIDTH": "256", "PARSY_BIG_MINK": "64"}   # pieces and BIG launches on inputs too small to take them
# (name, piece, mink, rest): the rows of tests/test_schedule_host.py
HOST_ROWS = (
    [(n, p, m, {"PARSY_BIG_SUPER": s}) for n, p, m, s in (("mid3d", 128, 16, "2"), ("mid3d", 128, 16, "4x2"), ("lap30", 128, 32, "2x4"),
                                                           ("lap30", 256, 64, "3"), ("nd24k", 256, 64, "2"), ("nd24k", 512, 128, "4"))]
    + [(n, p, m, {"PARSY_BIG_SUPER": s, "PARSY_BIG_DENSE": "2", **strips}) for n, p, m, s in (("nd24k", 256, 64, "2"), ("lap30", 128, 32, "2"),
                                                                                               ("lap30", 256, 64, "2x1"))
       for strips in ({}, {"PARSY_DENSE_STRIPS": "0"})]
    + [(n, p, m, {"PARSY_CHAIN_SPLIT": str(c)}) for n, p, m in (("mid3d", 128, 16), ("lap30", 128, 32), ("nd24k", 512, 128), ("nd24k", None, None))
       for c in (0, 1, 2)]
    + [(n, p, m, {"PARSY_PUSH_GROUP": str(g)}) for n, p, m, g in (("mid3d", 128, 16, 1), ("mid3d", 128, 48, 2), ("lap30", 128, 32, 1),
                                                                   ("lap30", 256, 64, 4), ("lap30", 0, 16, 1), ("nd24k", 512, 128, 1),
                                                                   ("nd24k", 256, 64, 2))]
    + [(n, None, None, {"PARSY_SUBTREES": "2"}) for n in ("tiny2d", "small3d", "ex15", "lap30", "mid3d")]
    + [(n, None, None, {"PARSY_SOLVE_ONE": "2"}) for n in ("tiny2d", "ex15", "small3d", "13x13x13:27", "24x24x2:27", "mid3d", "lap30", "nd24k")]
)
# the knobs those rows and launch_tables.KNOBS leave out, each on lap30 and nd24k under FORCED
BUILDER_KNOBS = (
    [{"PARSY_BIG_DENSE": str(d)} for d in range(5)]
    + [{"PARSY_DENSE_STRIPS": "0"}, {"PARSY_BIG_GROUP": "0"}, {"PARSY_BIG_GROUP": "2"},
       {"PARSY_BIG_SUPER_MIN": "1"}, {"PARSY_BIG_SUPER_MIN": "1", "PARSY_BIG_SUPER_FILL": "100"},
       {"PARSY_BIG_SUPER_MIN": "1", "PARSY_BIG_SUPER_FILL": "100", "PARSY_BIG_SUPER_HI": "4"}, {"PARSY_BIG_SUPER_FILL": "40"},
       {"PARSY_BIG_SUPER_HI": "3"},
       {"PARSY_DENSE_MIN_SHARE": "60"}, {"PARSY_DENSE_MIN_SHARE": "1"}, {"PARSY_DENSE_ALL_SHARE": "40"}, {"PARSY_DENSE_ALL_SHARE": "0"},
       {"PARSY_DENSE_FILL": "30"}, {"PARSY_DENSE_FILL": "100"},
       {"PARSY_SPLIT_CHUNKS": "16"}, {"PARSY_SPLIT_TARGET": "8"}, {"PARSY_SPLIT_MAX": "2"},
       {"PARSY_SPLIT_CHUNKS": "24", "PARSY_SPLIT_TARGET": "8", "PARSY_SPLIT_MAX": "7"},
       {"PARSY_CHOL_SUBTREES": "8"}, {"PARSY_CHOL_SUBTREES": "256"},
       {"PARSY_SUB_TIER_MIN_TREES": "0"}, {"PARSY_SUB_TIER_MIN_TREES": "32"}, {"PARSY_SUB_TIER_MIN_TREES": "32", "PARSY_SUBTREES": "4"}]
)


def label_of(name, env):
    return " ".join([name] + [f"{k}={v}" for k, v in env.items()])


def plans():
    """(label, symbolic, environment, mask steps): a step is (what, supernode mask | None, piece mask of rank r | None)."""
    for label, sym, env, mask in LT.plans():
        yield label, sym, env, ([] if mask is None else [("sn", mask)])
    for name, piece, mink, rest in HOST_ROWS:
        env = dict(rest) if piece is None else {"PARSY_PIECE_WIDTH": str(piece), "PARSY_BIG_MINK": str(mink), **rest}
        yield label_of(name, env), LT.sym_of(name), env, []
    for name in ("lap30", "nd24k"):
        for knobs in BUILDER_KNOBS:
            env = {**FORCED, **knobs}
            yield label_of(name, env), LT.sym_of(name), env, []
    for name in ("parabolic_fem", "72x72x72"):   # (analysed only by the process that takes them)
        yield name, (lambda name=name: LT.sym_of(name)), {}, []
    for name, env in (("lap30", {}), ("nd24k", FORCED)):
        sym = LT.sym_of(name)
        steps = []
        for nranks in (2, 3):
            for r, mask in enumerate(shard_masks(sym, nranks)):
                steps += [(f"shard {r}/{nranks}", "sn", mask), (f"shard {r}/{nranks} off", "sn", None)]
        for r in range(3):
            steps += [(f"pieces {r}/3", "pieces", r), (f"pieces {r}/3 off", "pieces", None)]
        yield label_of(name, env) + " masks", sym, env, steps


CLEAR = set(LT.CLEAR) | set(FORCED) | {k for row in HOST_ROWS for k in row[3]} | {k for e in BUILDER_KNOBS for k in e}


def set_env(env):
    for k in CLEAR:
        os.environ.pop(k, None)
    os.environ.update(env)


def digest(h):
    """[(field, hash)] of the plan behind the handle."""
    out, val, name = [], C.c_uint64(), C.c_char_p()
    n = lib.parsy_debug_schedule_digest(h, -1, None, None)
    assert n > 0
    for f in range(n):
        assert lib.parsy_debug_schedule_digest(h, f, C.byref(val), C.byref(name)) == n
        out.append((name.value.decode(), val.value))
    return out


def digests(label, sym, env, steps, device=-1):
    """(label, [(field, hash)]) of the plan, and of the plan after each mask step."""
    set_env(env)
    try:
        plan = api.Plan(sym() if callable(sym) else sym, device)
        if not steps or len(steps[0]) == 3:
            yield label, digest(plan._h)
        for step in steps:
            if len(step) == 2:   # (launch_tables: the one mask of a plan that is listed under it)
                plan.set_active(step[1])
                yield label, digest(plan._h)
                continue
            what, kind, arg = step
            if kind == "sn":
                plan.set_active(arg)
            else:
                plan.set_active_pieces(None if arg is None else api.Dist(plan, 3).mask(arg))
            yield f"{label}: {what}", digest(plan._h)
    finally:
        set_env({})


def show(label, d, fields):
    if fields:   # (the plan's line, then one line per field)
        print(label)
        for name, val in d:
            print(f"  {name} {val:016x}")
    else:
        whole = hashlib.sha256(b"".join(np.uint64(v).tobytes() for _, v in d)).hexdigest()
        print(f"{whole[:16]}  {label}")
    sys.stdout.flush()


if __name__ == "__main__":
    if "--device" in sys.argv:
        at = sys.argv.index("--device")
        dev = int(sys.argv[at + 1])
        for name in sys.argv[at + 2:]:
            for _, d in digests(name, LT.sym_of(name), {}, [], dev):
                for field, val in d:
                    print(f"check {name} cus=256\t{field}\t{val:016x}")
    else:
        k, n = (int(v) for v in sys.argv[sys.argv.index("--part") + 1].split("/")) if "--part" in sys.argv else (0, 1)
        for label, sym, env, steps in list(plans())[k::n]:
            for lab, d in digests(label, sym, env, steps):
                show(lab, d, "--fields" in sys.argv)
