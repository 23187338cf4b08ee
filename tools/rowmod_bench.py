"""Times of one row delete and one row add in the factor (parsy_factor_rowdel_device / parsy_factor_rowadd_device) next to
the same plan's full numeric factorization, with device events after warm-up.

Usage: python tools/rowmod_bench.py [--workloads ex15,nd24k,parabolic_fem,flan] [--reps 5]
                                    [--out profiles/rowmod_bench.json]

Per workload three rows of the factor's ordering, all in one process under the plan's ordering (sym.Perm):
  leaf  -- the last column of the first supernode: a reach of that supernode alone, the longest rotation path
  mid   -- the middle column of a supernode of the middle etree level: a separator half-way up
  last  -- row n - 1: the largest reach (every supernode whose row list ends in the root's last column), nothing below
and per row (median of --reps, ms; a delete and the add that puts the column back alternate, each timed by itself):
  rowdel_ms, rowadd_ms -- the whole call: the upload of its lists, its waits for the stream, every kernel
  factor_ms            -- the yardstick: parsy_factor_device on the same plan
  reach_supernodes, heights, row_launches, rotation_launches, entries_read, entries_walked -- parsy_rowmod_get_info
  model_bytes_del / _add -- 16 bytes (one read, one write) per walked entry of L, plus 8 bytes per entry the row pass of an
                            add reads
  hbm_fraction_del / _add -- model bytes over the time, over HBM_PEAK_TB_PER_S (the MI355X's 8 TB/s)
A workload whose factor does not fit the device's memory is skipped with a note.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from parsy_bench_amd import api, inspector as I, matrices as M  # noqa: E402

HBM_PEAK_TB_PER_S = 8.0


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def rows_of(sym):
    """{label: row in the factor's ordering}."""
    sup = np.asarray(sym.super)
    lp, ls = np.asarray(sym.levelPtr), np.asarray(sym.levelSet)
    nlev = lp.size - 1
    s = int(ls[lp[nlev // 2]])
    return {"leaf": int(sup[1]) - 1, "mid": (int(sup[s]) + int(sup[s + 1])) // 2, "last": sym.n - 1}


def column(sym, p):
    """(ci, cx) of column p (factor's ordering) of the symmetric matrix, in the caller's ordering, ascending."""
    A2p, A2i, A2x = np.asarray(sym.A2p), np.asarray(sym.A2i), np.asarray(sym.A2x)
    col = np.repeat(np.arange(sym.n), np.diff(A2p))
    lo, up = col == p, (A2i == p) & (col != p)
    other = np.concatenate([A2i[lo], col[up]])
    vals = np.concatenate([A2x[lo], A2x[up]])
    ci = np.asarray(sym.Perm)[other]
    order = np.argsort(ci)
    return ci[order].astype(np.int32), np.ascontiguousarray(vals[order])


def run(name, reps):
    import torch
    A, perm = M.workload(name)
    sym = I.analyze(A, perm)
    n, xsize = sym.n, int(sym.xsize)
    dev = torch.device("cuda", 0)
    free, _ = torch.cuda.mem_get_info(dev)
    if 8 * xsize * 1.5 > free:
        print(json.dumps({"workload": name, "skipped": f"lValues is {8 * xsize / 1e9:.1f} GB, {free / 1e9:.1f} GB free"}), flush=True)
        return []
    plan = api.Plan(sym, 0)
    plan.set_perm(sym.Perm)
    vals = torch.from_numpy(np.ascontiguousarray(sym.A2x)).to(dev)
    L = torch.empty(xsize, dtype=torch.float64, device=dev)

    def factor():
        plan.factor_device(vals.data_ptr(), L.data_ptr(), 0)

    factor()
    torch.cuda.synchronize()
    assert plan.status() == 0
    factor_ms = float(np.median([_timed(torch, factor) for _ in range(reps)]))
    out = []
    for label, p in rows_of(sym).items():
        k = int(sym.Perm[p])
        ci, cx = column(sym, p)
        d_cx = torch.from_numpy(cx).to(dev)

        def delete():
            plan.rowdel_device(L.data_ptr(), k)

        def add():
            plan.rowadd_device(L.data_ptr(), k, ci, d_cx.data_ptr())

        delete(), add()               # warm-up: the workspaces, the kernels
        torch.cuda.synchronize()
        assert plan.rowmod_status() == 0
        dels, adds = [], []
        for _ in range(reps):
            dels.append(_timed(torch, delete))
            idel = plan.rowmod_info
            adds.append(_timed(torch, add))
            iadd = plan.rowmod_info
            assert plan.rowmod_status() == 0
        del_ms, add_ms = float(np.median(dels)), float(np.median(adds))
        bytes_del = 16 * idel["entries_walked"]
        bytes_add = 16 * iadd["entries_walked"] + 8 * iadd["entries_read"]
        row = {"workload": name, "n": n, "xsize": xsize, "row": label, "p": p, "rowdel_ms": del_ms, "rowadd_ms": add_ms,
               "factor_ms": factor_ms, "speedup_del": factor_ms / del_ms, "speedup_add": factor_ms / add_ms,
               "reach_supernodes": iadd["reach_supernodes"], "heights": iadd["heights"],
               "row_launches": iadd["row_launches"], "rotation_launches": iadd["rotation_launches"],
               "entries_read": iadd["entries_read"], "entries_walked": iadd["entries_walked"],
               "model_bytes_del": bytes_del, "model_bytes_add": bytes_add,
               "hbm_fraction_del": bytes_del / (del_ms * 1e-3) / 1e12 / HBM_PEAK_TB_PER_S,
               "hbm_fraction_add": bytes_add / (add_ms * 1e-3) / 1e12 / HBM_PEAK_TB_PER_S,
               "device_bytes": iadd["device_bytes"]}
        print(json.dumps(row), flush=True)
        out.append(row)
        factor()                      # (the next row starts from the factor of A again)
        torch.cuda.synchronize()
    plan.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="ex15,nd24k,parabolic_fem,flan")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rowmod_bench.json"))
    a = ap.parse_args()
    rows = []
    for name in a.workloads.split(","):
        rows += run(name, a.reps)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
