"""Times of the product sampled on A's pattern (parsy_pattern_outer_device) next to the forward + backward solve that
produces lambda, with device events after warm-up, and its algorithmic bytes.

Usage: python tools/grad_bench.py [--workloads parabolic_fem,flan] [--nrhs 1,8,64] [--reps 5] [--out profiles/grad_bench.json]

Per workload and number of right-hand sides (median of --reps, ms):
  pattern_outer -- the whole call under the plan's ordering (sym.Perm): below PARSY_GRAD_MRHS_MIN the direct kernel,
                   from there on the staging of P lambda and P x and the lanes-per-entry kernel
  solve_fb      -- the plain forward + backward solve of the permuted system (parsy_solve_device + parsy_backsolve_device)
  bytes         -- 16 nnzA (row, col, g) + 16 n nrhs (lambda and x once each)
  inverse_pattern -- parsy_inverse_pattern_device on an arbitrary Z (24 nnzA bytes and a gather), for scale
  residual_call -- the yardstick, timed in the same run: parsy_residual_device (berr included, so with its host
                   synchronisation) at the same input, ordering and right-hand sides -- the value gather, two
                   permutations in, k_sym_sweep (one pass over the same pattern with one gathered operand where
                   pattern_outer has four) and the berr pass; tools/refine_bench.py records the same call
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from parsy_bench_amd import api, inspector as I, matrices as M  # noqa: E402


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
    plan.set_perm(sym.Perm)
    dev = torch.device("cuda", 0)
    n, nnz = sym.n, int(sym.nnzA)
    vals = torch.from_numpy(np.ascontiguousarray(sym.A2x)).to(dev)
    L = torch.empty(int(sym.xsize), dtype=torch.float64, device=dev)
    plan.factor_device(vals.data_ptr(), L.data_ptr(), 0)
    torch.cuda.synchronize()
    assert plan.status() == 0
    G = torch.empty(nnz, dtype=torch.float64, device=dev)
    plan.inverse_pattern_device(L.data_ptr(), G.data_ptr())   # (L stands in for Z: same layout, same gather)
    t_inv = _events(lambda: plan.inverse_pattern_device(L.data_ptr(), G.data_ptr()), reps)
    out = []
    for nrhs in nrhs_list:
        g = torch.Generator(device="cpu").manual_seed(nrhs)
        B = torch.randn(nrhs * n, dtype=torch.float64, generator=g).to(dev)
        X = torch.empty_like(B)
        Lam = torch.randn(nrhs * n, dtype=torch.float64, generator=g).to(dev)

        def solve_fb():
            X.copy_(B)
            plan.solve_device(L.data_ptr(), X.data_ptr(), nrhs, n, 0)
            plan.backsolve_device(L.data_ptr(), X.data_ptr(), nrhs, n, 0)

        def outer():
            plan.pattern_outer_device(Lam.data_ptr(), n, X.data_ptr(), n, nrhs, G.data_ptr(), alpha=-1.0)

        def resid():
            plan.residual_device(vals.data_ptr(), X.data_ptr(), n, B.data_ptr(), n, nrhs)

        for f in (solve_fb, outer, resid):   # warm-up: buffers, the coordinates, the full pattern, the kernels
            f()
        torch.cuda.synchronize()
        t_fb = _events(solve_fb, reps)
        assert plan.solve_status() == 0
        t_out = _events(outer, reps)
        t_res = _events(resid, reps)
        nbytes = 16 * nnz + 16 * n * nrhs
        row = {"workload": name, "n": n, "nnzA": nnz, "nrhs": nrhs, "lanes": plan.grad_info["last_lanes"],
               "pattern_outer_ms": t_out, "bytes": nbytes, "tb_per_s": nbytes / (t_out * 1e-3) / 1e12,
               "solve_fb_ms": t_fb, "outer_over_solve_fb": t_out / t_fb, "residual_call_ms": t_res,
               "outer_over_residual_call": t_out / t_res, "inverse_pattern_ms": t_inv}
        print(json.dumps(row), flush=True)
        out.append(row)
    plan.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="parabolic_fem,flan")
    ap.add_argument("--nrhs", default="1,8,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "grad_bench.json"))
    a = ap.parse_args()
    rows = []
    for name in a.workloads.split(","):
        rows += run(name, [int(v) for v in a.nrhs.split(",")], a.reps)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
