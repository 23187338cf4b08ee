"""Times of the selected inversion (parsy_selinv_device), the inverse diagonal (parsy_inverse_diag_device) and the
log-determinant (parsy_logdet_device) next to the factorization of the same plan, with device events after warm-up.

Usage: python tools/selinv_bench.py [--workloads ex15,nd24k,parabolic_fem,flan] [--reps 5] [--sweep 0,32,64,96,128,1000000000]
                                    [--out profiles/selinv_bench.json]

Per workload (median of --reps, ms): factor, selinv (default PARSY_SELINV_TILED_MIN), inverse_diag, logdet (with its host
synchronisation), and info.flops / selinv time.  --sweep: the selinv time under each threshold (the measurement behind
the default; a very large value sends every block column to the small path, 0 every one to the tiled path).  The
per-kernel split between the paths comes from a separate run of this tool under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from parsy_bench_amd import api, inspector as I, matrices as M  # noqa: E402


def _events(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
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


def run(name, reps, sweep):
    t0 = time.time()
    A, perm = M.workload(name)
    sym = I.analyze(A, perm)
    plan = api.Plan(sym, 0)
    dev = torch.device("cuda", 0)
    vals = torch.from_numpy(np.ascontiguousarray(sym.A2x)).to(dev)
    L = torch.empty(int(sym.xsize), dtype=torch.float64, device=dev)
    Z = torch.empty(int(sym.xsize), dtype=torch.float64, device=dev)
    D = torch.empty(sym.n, dtype=torch.float64, device=dev)
    out = {"workload": name, "n": sym.n, "nsuper": sym.nsuper, "xsize": int(sym.xsize)}
    out["factor_ms"] = _events(lambda: plan.factor_device(vals.data_ptr(), L.data_ptr()), reps)
    assert plan.status() == 0
    os.environ.pop("PARSY_SELINV_TILED_MIN", None)
    out["selinv_ms"] = _events(lambda: plan.selinv_device(L.data_ptr(), Z.data_ptr()), reps)
    info = plan.selinv_info
    out["info"] = info
    out["selinv_gflops"] = info["flops"] / (out["selinv_ms"] * 1e-3) / 1e9
    out["selinv_over_factor"] = out["selinv_ms"] / out["factor_ms"]
    out["inverse_diag_ms"] = _events(lambda: plan.inverse_diag_device(Z.data_ptr(), D.data_ptr()), reps)
    out["logdet_ms"] = _events(lambda: plan.logdet_device(L.data_ptr()), reps)
    out["logdet"] = plan.logdet_device(L.data_ptr())[0]
    out["diag_finite_positive"] = bool(torch.all(D > 0).item())
    out["sweep"] = {}
    for t in sweep:
        os.environ["PARSY_SELINV_TILED_MIN"] = str(t)
        ms = _events(lambda: plan.selinv_device(L.data_ptr(), Z.data_ptr()), reps)
        si = plan.selinv_info
        out["sweep"][str(t)] = {"ms": ms, "tiled_block_columns": si["tiled_block_columns"], "launches": si["launches"]}
    os.environ.pop("PARSY_SELINV_TILED_MIN", None)
    out["wall_s"] = time.time() - t0
    plan.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="ex15,nd24k,parabolic_fem,flan")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sweep = [int(v) for v in a.sweep.split(",") if v]
    res = []
    for name in a.workloads.split(","):
        r = run(name, a.reps, sweep)
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
