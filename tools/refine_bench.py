"""Times of A x = b with refinement (parsy_residual_device, parsy_solve_spd_device) next to the plain solve, with device
events after warm-up, and the algorithmic bytes of the residual.

Usage: python tools/refine_bench.py [--workloads flan,parabolic_fem] [--nrhs 1,8,64] [--reps 5] [--out profiles/refine_bench.json]

Per workload and number of right-hand sides (median of --reps, ms):
  solve_fb     -- the plain forward + backward solve of the permuted system (parsy_solve_device + parsy_backsolve_device)
  residual_call -- parsy_residual_device with the identity ordering and berr: the value gather, the two permutations in,
                  k_sym_sweep and the berr pass, with its host synchronisation
  gather, k_sym_sweep -- the kernels alone: run this tool under `rocprofv3 --kernel-trace --stats`
  step         -- one refinement step, host synchronisation included: the call with max_steps = 1 minus the call with
                  max_steps = 0 (both report berr and steps), on values 10 % of the diagonal shift away from the factor
  resid_bytes  -- full pattern values (8 B) and column indices (4 B), row pointers (8 B), z, pb, r once each
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


def stale(A, shift, frac=0.1, seed=11):
    delta = frac * shift * np.random.default_rng(seed).random(A.n)
    Ax = A.Ax.copy()
    diag_pos = A.Ap[:-1]   # (rows are sorted: the diagonal is a column's first entry of the lower triangle)
    assert (A.Ai[diag_pos] == np.arange(A.n)).all()
    Ax[diag_pos] += delta
    return Ax


def run(name, nrhs_list, reps):
    A, perm = M.workload(name)
    sym = I.analyze(A, perm)
    plan = api.Plan(sym, 0)
    dev = torch.device("cuda", 0)
    n = sym.n
    vals = torch.from_numpy(np.ascontiguousarray(sym.A2x)).to(dev)
    svals = torch.from_numpy(sym.permute_values(stale(A, M.WORKLOADS[name][4]))).to(dev)
    L = torch.empty(int(sym.xsize), dtype=torch.float64, device=dev)
    plan.factor_device(vals.data_ptr(), L.data_ptr(), 0)
    torch.cuda.synchronize()
    assert plan.status() == 0
    nnz_full = 2 * int(sym.nnzA) - n
    out = []
    for nrhs in nrhs_list:
        g = torch.Generator(device="cpu").manual_seed(nrhs)
        B = torch.randn(nrhs * n, dtype=torch.float64, generator=g).to(dev)
        X = torch.empty_like(B)

        def solve_fb():
            X.copy_(B)
            plan.solve_device(L.data_ptr(), X.data_ptr(), nrhs, n, 0)
            plan.backsolve_device(L.data_ptr(), X.data_ptr(), nrhs, n, 0)

        def resid():
            plan.residual_device(vals.data_ptr(), X.data_ptr(), n, B.data_ptr(), n, nrhs)

        def refined(k):
            return lambda: plan.solve_spd_device(svals.data_ptr(), L.data_ptr(), B.data_ptr(), n, X.data_ptr(), n,
                                                 nrhs, k)

        plan.set_perm(None)
        for f in (solve_fb, resid, refined(0), refined(1)):   # warm-up: buffers, the full pattern, the kernels
            f()
        torch.cuda.synchronize()
        t_fb = _events(solve_fb, reps)
        assert plan.solve_status() == 0
        t_res = _events(resid, reps)
        t0 = _events(refined(0), reps)
        t1 = _events(refined(1), reps)
        steps, berr = plan.solve_spd_device(svals.data_ptr(), L.data_ptr(), B.data_ptr(), n, X.data_ptr(), n, nrhs, 1)
        resid_bytes = nnz_full * 12 + (n + 1) * 8 + 3 * n * nrhs * 8
        row = {"workload": name, "n": n, "nnz_full": nnz_full, "nrhs": nrhs, "solve_fb_ms": t_fb,
               "residual_call_ms": t_res, "refine0_ms": t0, "refine1_ms": t1, "step_ms": t1 - t0,
               "step_over_solve_fb": (t1 - t0) / t_fb, "resid_bytes": resid_bytes,
               "steps_taken_at_1": int(steps.min()), "berr_after_1": float(berr.max())}
        print(json.dumps(row), flush=True)
        out.append(row)
    plan.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="flan,parabolic_fem")
    ap.add_argument("--nrhs", default="1,8,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "refine_bench.json"))
    a = ap.parse_args()
    rows = []
    for name in a.workloads.split(","):
        rows += run(name, [int(v) for v in a.nrhs.split(",")], a.reps)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
