"""Times of one update of the factor (parsy_factor_updown_device) next to the same plan's full numeric factorization,
with device events after warm-up.

Usage: python tools/updown_bench.py [--workloads nd24k,parabolic_fem,flan] [--k 1,8,16] [--reps 5]
                                    [--out profiles/updown_bench.json]

Per workload and number of columns k of W (median of --reps, ms), all in one process under the plan's ordering (sym.Perm):
  updown_ms     -- one update by a W whose k columns all start at column 0 of the factor's ordering, the bottom of the
                   tree, and fill the structure of that column: the longest kind of path, a leaf up to the root.  The
                   whole call: the upload of W's pattern, the scatter, two launches per block column, the clear.
  factor_ms     -- the yardstick: parsy_factor_device on the same plan
  path_supernodes, block_columns, launches, entries_touched -- parsy_updown_get_info
  model_bytes   -- 16 bytes (one read, one write) per walked entry of L per block of 8 columns of W: entries_touched * 16
  tb_per_s, hbm_fraction -- model_bytes over updown_ms, and that over HBM_PEAK_TB_PER_S (the MI355X's 8 TB/s)
Repeated updates keep adding W W' to the same factor: the time does not depend on the values, and an update cannot fail.
A workload whose factor does not fit the device's memory is skipped with a note (--workloads may name flan).
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


def _events(torch, fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def bottom_w(sym, k, seed=0):
    """(wp, wi, wx) in the caller's ordering: k columns on the whole structure of column 0 of L, values in (0.05, 1)."""
    c1 = int(sym.super[1])
    rows = np.asarray(sym.s[int(sym.i_ptr[0]): int(sym.i_ptr[c1])], dtype=np.int64)
    caller = np.sort(np.asarray(sym.Perm)[rows]).astype(np.int32)
    wp = (np.arange(k + 1) * caller.size).astype(np.int32)
    wx = np.random.default_rng(seed).uniform(0.05, 1.0, k * caller.size)
    return wp, np.tile(caller, k), wx


def run(name, ks, reps):
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
    factor_ms = _events(torch, factor, reps)
    out = []
    for k in ks:
        wp, wi, wx = bottom_w(sym, k, seed=k)
        d_wx = torch.from_numpy(wx).to(dev)

        def update():
            plan.updown_device(L.data_ptr(), wp, wi, d_wx.data_ptr(), sign=+1)

        update()                      # warm-up: the workspace, the kernels
        torch.cuda.synchronize()
        assert plan.updown_status() == 0
        ms = _events(torch, update, reps)
        info = plan.updown_info
        nbytes = 16 * info["entries_touched"]
        row = {"workload": name, "n": n, "xsize": xsize, "k": k, "updown_ms": ms, "factor_ms": factor_ms,
               "speedup": factor_ms / ms, "path_supernodes": info["path_supernodes"], "block_columns": info["block_columns"],
               "launches": info["last_launches"], "entries_touched": info["entries_touched"], "model_bytes": nbytes,
               "tb_per_s": nbytes / (ms * 1e-3) / 1e12, "hbm_fraction": nbytes / (ms * 1e-3) / 1e12 / HBM_PEAK_TB_PER_S,
               "device_bytes": info["device_bytes"]}
        print(json.dumps(row), flush=True)
        out.append(row)
        factor()                      # (the next k starts from the factor of A again)
        torch.cuda.synchronize()
    plan.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="nd24k,parabolic_fem,flan")
    ap.add_argument("--k", default="1,8,16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "updown_bench.json"))
    a = ap.parse_args()
    rows = []
    for name in a.workloads.split(","):
        rows += run(name, [int(v) for v in a.k.split(",")], a.reps)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
