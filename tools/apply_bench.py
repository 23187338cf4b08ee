"""Times of the factor's two products (parsy_factor_apply_device, PARSY_OP_G and PARSY_OP_GT) next to their yardsticks,
the existing solves on the same plan at the same number of right-hand sides, with device events after warm-up.

Usage: python tools/apply_bench.py [--workloads parabolic_fem,flan] [--nrhs 1,8,64] [--reps 5] [--out profiles/apply_bench.json]

Per workload and number of right-hand sides (median of --reps, ms), all in one process under the plan's ordering
(sym.Perm):
  g_ms, gt_ms           -- Y = P' L X and Y = L' P X, the whole call (every block of block_columns right-hand sides:
                           the panel pass, the sum pass and, for G', the staging of X)
  solve_ms, backsolve_ms -- the yardsticks: parsy_solve_device against G, parsy_backsolve_device against G'.  They read
                           the same bytes of lValues but sit behind a dependency chain; the products have none.
  bytes                 -- 8 xsize per block of block_columns right-hand sides (the read of lValues alone)
  g_tb_per_s, gt_tb_per_s -- bytes over the call's time, to set beside the measured copy rate of the device
                           (COPY_TB_PER_S below: a float4 copy on an MI355X)
The expectation: g_ms <= solve_ms and gt_ms <= backsolve_ms at every point ("g_within", "gt_within").
workspace_bytes and device_bytes come from parsy_factor_apply_get_info; workspace_bytes is known without a device
(--host-only prints it and the plan's sizes and exits).
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from parsy_bench_amd import api, inspector as I, matrices as M  # noqa: E402

COPY_TB_PER_S = 6.29


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


def host_sizes(name):
    A, perm = M.workload(name)
    sym = I.analyze(A, perm)
    plan = api.Plan(sym, -1)
    info = plan.apply_info
    row = {"workload": name, "n": sym.n, "ssize": int(sym.ssize), "xsize": int(sym.xsize), **info}
    plan.close()
    return row


def run(name, nrhs_list, reps):
    import torch
    A, perm = M.workload(name)
    sym = I.analyze(A, perm)
    plan = api.Plan(sym, 0)
    plan.set_perm(sym.Perm)
    dev = torch.device("cuda", 0)
    n, xsize = sym.n, int(sym.xsize)
    vals = torch.from_numpy(np.ascontiguousarray(sym.A2x)).to(dev)
    L = torch.empty(xsize, dtype=torch.float64, device=dev)
    plan.factor_device(vals.data_ptr(), L.data_ptr(), 0)
    torch.cuda.synchronize()
    assert plan.status() == 0
    out = []
    for nrhs in nrhs_list:
        g = torch.Generator(device="cpu").manual_seed(nrhs)
        B = torch.randn(nrhs * n, dtype=torch.float64, generator=g).to(dev)
        X = torch.empty_like(B)
        Y = torch.empty_like(B)

        def prod_g():
            plan.factor_apply_device(L.data_ptr(), "G", B.data_ptr(), n, nrhs, Y.data_ptr(), n)

        def prod_gt():
            plan.factor_apply_device(L.data_ptr(), "GT", B.data_ptr(), n, nrhs, Y.data_ptr(), n)

        def solve():
            plan.solve_device(L.data_ptr(), X.data_ptr(), nrhs, n, 0)

        def backsolve():
            plan.backsolve_device(L.data_ptr(), X.data_ptr(), nrhs, n, 0)

        X.copy_(B)
        for f in (prod_g, prod_gt, solve, backsolve):   # warm-up: the index, the workspaces, the kernels
            f()
        torch.cuda.synchronize()
        assert plan.solve_status() == 0
        # (the solves run in place on whatever the last one left: their time does not depend on the values)
        X.copy_(B)
        t = {"g_ms": _events(torch, prod_g, reps), "solve_ms": _events(torch, solve, reps),
             "gt_ms": _events(torch, prod_gt, reps), "backsolve_ms": _events(torch, backsolve, reps)}
        info = plan.apply_info
        nbytes = 8 * xsize * -(-nrhs // info["block_columns"])
        row = {"workload": name, "n": n, "xsize": xsize, "ssize": int(sym.ssize), "nrhs": nrhs,
               "block_columns": info["block_columns"], **t, "bytes": nbytes,
               "g_tb_per_s": nbytes / (t["g_ms"] * 1e-3) / 1e12, "gt_tb_per_s": nbytes / (t["gt_ms"] * 1e-3) / 1e12,
               "copy_tb_per_s": COPY_TB_PER_S, "g_within": t["g_ms"] <= t["solve_ms"],
               "gt_within": t["gt_ms"] <= t["backsolve_ms"], "workspace_bytes": info["workspace_bytes"],
               "device_bytes": info["device_bytes"]}
        print(json.dumps(row), flush=True)
        out.append(row)
    plan.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="parabolic_fem,flan")
    ap.add_argument("--nrhs", default="1,8,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-only", action="store_true", help="print the sizes known without a device and exit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "apply_bench.json"))
    a = ap.parse_args()
    if a.host_only:
        for name in a.workloads.split(","):
            print(json.dumps(host_sizes(name)), flush=True)
        return
    rows = []
    for name in a.workloads.split(","):
        rows += run(name, [int(v) for v in a.nrhs.split(",")], a.reps)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
