"""Times of parsy_eigs_device (the k smallest eigenpairs of A v = lambda M v through the factor) next to the time of the
same number of right-hand sides sent through the plan's plain solves, with device events after a warm-up.

Usage: python tools/eigs_bench.py [--workloads ex15,nd24k,parabolic_fem] [--ks 1,8,32] [--reps 5] [--max-iter 200]
                                  [--kernel-stats FILE_kernel_stats.csv] [--out profiles/eigs_bench.json]
The Flan-class input gets a run of its own (--workloads flan), as with the other feature tools.

Per workload, k in --ks and M in {I, a mass-like M}: tol = 1e-10, block = min(k, 8), the default basis, the factor of A,
the start block numpy.random.default_rng(0).standard_normal((n, block)).  A row of the result holds
  eigs_ms        -- device-event time of the whole call (median of --reps after a warm-up): its waits for the stream
                    and the host's small dense work included
  iterations, restarts, solve_columns, nconv, basis, dropped -- parsy_eigs_get_info of the last call
  solves_ms      -- in the same process: solve_columns right-hand sides through parsy_solve_spd_device(max_steps = 0)
                    in blocks of `block` (median of --reps)
  outside_share  -- 1 - solves_ms / eigs_ms: the headline, the share of the call spent outside those solves
  resid_max      -- the largest returned eta
The mass-like M: on A's pattern, |a_ij| / 8 off the diagonal and the row sum of those plus 1 on it (diagonally dominant,
positive).

--kernel-stats: the *_kernel_stats.csv of a separate `rocprofv3 --kernel-trace --stats -- python tools/eigs_bench.py
--workloads W --ks K --reps 1` run.  For k_eigs_gram and k_eigs_rotate the tool then prints calls, mean time and -- with
the model bytes of the largest shape of the run, 8 n (p + q) with p = q = basis for the Gram kernel and 8 n (p + 2 q)
with p = basis, q = 16 for the rotation -- the fraction of the MI355X's 8 TB/s that shape would need at the mean time
(an upper estimate: most calls are smaller).  Without the file those cells are "not measured".
A workload whose factor and basis do not fit the device's memory is skipped with a note.
"""
import argparse
import csv
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from parsy_bench_amd import api, inspector as I, matrices as M  # noqa: E402

HBM_PEAK_TB_PER_S = 8.0
TOL = 1e-10


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def mass_like(sym):
    """A2-order values of a diagonally dominant positive M on A's pattern."""
    A2p, A2i, A2x = np.asarray(sym.A2p), np.asarray(sym.A2i), np.asarray(sym.A2x)
    col = np.repeat(np.arange(sym.n), np.diff(A2p))
    off = A2i != col
    v = np.where(off, np.abs(A2x) / 8, 0.0)
    rows = np.zeros(sym.n)
    np.add.at(rows, A2i[off], v[off])
    np.add.at(rows, col[off], v[off])
    v[~off] = rows[A2i[~off]] + 1.0
    return v


def default_basis(n, k, block):
    return min(max(3 * k, k + 4 * block), n, 128)


def run(name, ks, reps, max_iter):
    import torch
    A, perm = M.workload(name)
    sym = I.analyze(A, perm)
    n, xsize = sym.n, int(sym.xsize)
    dev = torch.device("cuda", 0)
    free, _ = torch.cuda.mem_get_info(dev)
    need = 8 * (xsize * 1.5 + 3 * n * 128 + 8 * n * 16)
    if need > free:
        print(json.dumps({"workload": name, "skipped": f"needs {need / 1e9:.1f} GB, {free / 1e9:.1f} GB free"}), flush=True)
        return []
    plan = api.Plan(sym, 0)
    plan.set_perm(sym.Perm)
    vals = torch.from_numpy(np.ascontiguousarray(sym.A2x)).to(dev)
    mvals = torch.from_numpy(mass_like(sym)).to(dev)
    L = torch.empty(xsize, dtype=torch.float64, device=dev)
    plan.factor_device(vals.data_ptr(), L.data_ptr(), 0)
    torch.cuda.synchronize()
    assert plan.status() == 0
    out = []
    for k in ks:
        block = min(k, 8)
        if k + 2 * block > default_basis(n, k, block):
            continue
        x0 = torch.from_numpy(np.asfortranarray(np.random.default_rng(0).standard_normal((n, block))).T.copy()).to(dev)
        y = torch.zeros(n * k, dtype=torch.float64, device=dev)
        for mname, mptr in (("I", 0), ("mass", mvals.data_ptr())):
            res = {}

            def call():
                rc, lam, resid, nconv = plan.eigs_device(vals.data_ptr(), mptr, L.data_ptr(), k, x0.data_ptr(), n, block,
                                                         y.data_ptr(), n, tol=TOL, max_iter=max_iter)
                assert rc == 0
                res.update(resid=resid, nconv=nconv)

            call()   # warm-up: the workspace, the kernels
            ms = float(np.median([_timed(torch, call) for _ in range(reps)]))
            info = plan.eigs_info
            cols = int(info["solve_columns"])
            B = torch.from_numpy(np.asfortranarray(np.random.default_rng(1).standard_normal((n, block))).T.copy()).to(dev)
            X = torch.empty_like(B)

            def solves():
                left = cols
                while left > 0:
                    q = min(block, left)
                    plan.solve_spd_device(vals.data_ptr(), L.data_ptr(), B.data_ptr(), n, X.data_ptr(), n, q, max_steps=0)
                    left -= q

            solves()
            solves_ms = float(np.median([_timed(torch, solves) for _ in range(reps)]))
            row = {"workload": name, "n": n, "xsize": xsize, "k": k, "block": block, "M": mname, "tol": TOL,
                   "eigs_ms": ms, "solves_ms": solves_ms, "outside_share": 1.0 - solves_ms / ms,
                   "iterations": info["iterations"], "restarts": info["restarts"], "solve_columns": cols,
                   "nconv": int(res["nconv"]), "basis": info["basis"], "dropped": info["dropped"],
                   "resid_max": float(np.max(res["resid"])), "device_bytes": info["device_bytes"]}
            print(json.dumps(row), flush=True)
            out.append(row)
    plan.close()
    return out


def kernel_cells(path, rows):
    """{kernel: {calls, mean_us, model_bytes, hbm_fraction}} from a rocprofv3 kernel_stats csv, or "not measured"."""
    cells = {"k_eigs_gram": "not measured", "k_eigs_rotate": "not measured"}
    if not path or not rows:
        return cells
    n = max(r["n"] for r in rows)
    p = max(default_basis(r["n"], r["k"], r["block"]) for r in rows)
    model = {"k_eigs_gram": 8 * n * (p + p), "k_eigs_rotate": 8 * n * (p + 2 * 16)}
    with open(path, newline="") as f:
        for rec in csv.DictReader(f):
            for kname in list(cells):
                if kname in rec.get("Name", "") and "reduce" not in rec.get("Name", ""):
                    calls, total_ns = int(rec["Calls"]), float(rec["TotalDurationNs"])
                    prev = cells[kname] if isinstance(cells[kname], dict) else {"calls": 0, "total_ns": 0.0}
                    cells[kname] = {"calls": prev["calls"] + calls, "total_ns": prev["total_ns"] + total_ns}
    for kname, c in cells.items():
        if isinstance(c, dict):
            mean_s = c["total_ns"] / c["calls"] * 1e-9
            c.update(mean_us=mean_s * 1e6, model_bytes=model[kname],
                     hbm_fraction=model[kname] / mean_s / 1e12 / HBM_PEAK_TB_PER_S)
    return cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="ex15,nd24k,parabolic_fem")
    ap.add_argument("--ks", default="1,8,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=200)
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "eigs_bench.json"))
    a = ap.parse_args()
    rows = []
    for name in a.workloads.split(","):
        rows += run(name, [int(k) for k in a.ks.split(",")], a.reps, a.max_iter)
    cells = kernel_cells(a.kernel_stats, [r for r in rows if "eigs_ms" in r])
    print(json.dumps({"kernels": cells}), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps({"rows": rows, "kernels": cells}, indent=1) + "\n")


if __name__ == "__main__":
    main()
