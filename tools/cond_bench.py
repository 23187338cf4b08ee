"""Times of the forward error bounds (parsy_error_bounds_device) and of the condition estimate (parsy_rcond_device) next
to as many plain solve pairs, with device events after warm-up.

Usage: python tools/cond_bench.py [--workloads ex15,nd24k,parabolic_fem] [--nrhs 1,8,64] [--reps 5] [--out profiles/cond_bench.json]

Per workload and number of right-hand sides (median of --reps, ms):
  bounds_ms     -- parsy_error_bounds_device on the refined solution (ferr and berr): the value gather, the two
                   permutations in, the residual, the weights, `applications` solve pairs with the step kernel and one
                   host read of the control word after each
  applications  -- the solve pairs that call enqueued (parsy_cond_get_info)
  pairs_ms      -- that many plain solve pairs on the same plan: parsy_solve_spd_device with max_steps = 0, no steps, no
                   berr (permutation in, forward + backward solve, permutation out; nothing synchronises inside)
  overhead_ms   -- bounds_ms - pairs_ms: the estimator's own share (weight and step kernels, residual, host reads)
  rcond_ms, rcond_applications, rcond -- parsy_rcond_device (one column) on the same plan, once per workload
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from parsy_bench_amd import _native as N, api, inspector as I, matrices as M  # noqa: E402


def _events(fn, reps):
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


def run(name, nrhs_list, reps):
    A, perm = M.workload(name)
    sym = I.analyze(A, perm)
    plan = api.Plan(sym, 0)
    dev = torch.device("cuda", 0)
    n = sym.n
    vals = torch.from_numpy(np.ascontiguousarray(sym.A2x)).to(dev)
    L = torch.empty(int(sym.xsize), dtype=torch.float64, device=dev)
    plan.factor_device(vals.data_ptr(), L.data_ptr(), 0)
    torch.cuda.synchronize()
    assert plan.status() == 0
    plan.set_perm(None)
    v, l = vals.data_ptr(), L.data_ptr()
    plan.rcond_device(v, l)   # warm-up: the full pattern, the workspace, the kernels
    t_rc = _events(lambda: plan.rcond_device(v, l), reps)
    rcond, anorm = plan.rcond_device(v, l)
    rc_apps = plan.cond_info["applications"]
    out = []
    for nrhs in nrhs_list:
        g = torch.Generator(device="cpu").manual_seed(nrhs)
        B = torch.randn(nrhs * n, dtype=torch.float64, generator=g).to(dev)
        X = torch.empty_like(B)
        b, x = B.data_ptr(), X.data_ptr()
        plan.solve_spd_device(v, l, b, n, x, n, nrhs, 5)

        def bounds():
            return plan.error_bounds_device(v, l, x, n, b, n, nrhs)

        ferr, berr = bounds()   # warm-up
        apps = plan.cond_info["applications"]
        Y = torch.empty_like(B)

        def pairs():
            for _ in range(apps):
                if N.lib().parsy_solve_spd_device(plan._h, v, l, b, n, Y.data_ptr(), n, nrhs, 0, None, None, None) != 0:
                    raise RuntimeError(N.last_error())

        pairs()
        torch.cuda.synchronize()
        t_b = _events(bounds, reps)
        t_p = _events(pairs, reps)
        assert plan.solve_status() == 0
        row = {"workload": name, "n": n, "nrhs": nrhs, "bounds_ms": t_b, "applications": apps, "pairs_ms": t_p,
               "overhead_ms": t_b - t_p, "overhead_over_pairs": (t_b - t_p) / t_p, "ferr_max": float(ferr.max()),
               "berr_max": float(berr.max()), "rcond_ms": t_rc, "rcond_applications": rc_apps, "rcond": rcond,
               "anorm": anorm, "cond_device_bytes": plan.cond_info["device_bytes"]}
        print(json.dumps(row), flush=True)
        out.append(row)
    plan.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="ex15,nd24k,parabolic_fem")
    ap.add_argument("--nrhs", default="1,8,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cond_bench.json"))
    a = ap.parse_args()
    rows = []
    for name in a.workloads.split(","):
        rows += run(name, [int(v) for v in a.nrhs.split(",")], a.reps)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
