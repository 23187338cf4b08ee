"""Times of the solve with sparse right-hand sides (parsy_solve_sparse_device, PARSY_SPARSE_A) next to the same plan's full
forward + backward solve at the same number of right-hand sides, with device events after warm-up, one process.

Usage: python tools/sparse_solve_bench.py [--workloads ex15,parabolic_fem,nd24k,flan] [--reps 7]
                                          [--out profiles/sparse_solve.json] [--table profiles/sparse_solve.txt]

Per workload (matrices.workload: from a 2-D grid up to the Flan-class stand-in), under the plan's ordering (sym.Perm), B =
nrhs unit columns at rows drawn once per workload (seed 0; the first is also the one selected row), for nrhs = 1 and 8 and
for one selected row and all rows:
  sparse_ms       -- the whole call: every kernel of the forward pass over F, the backward pass over K, gather and clearing
  full_ms         -- the yardstick: parsy_solve_device + parsy_backsolve_device on an n x nrhs block of the same plan
  reach_share     -- (fwd_entries + bwd_entries) / (2 xsize): what the sparse call reads of L against the two full solves
  fwd_steps, bwd_steps, kernels, fwd_supernodes, bwd_supernodes, device_bytes -- parsy_reach_get_info
  model_bytes     -- 8 bytes per entry of L read, once per block of 8 right-hand sides
  hbm_fraction    -- model bytes over the time, over HBM_PEAK_TB_PER_S (the MI355X's 8 TB/s)
  wins            -- sparse_ms < full_ms
The call never falls back to the full solve by itself: where `wins` is false the full solve is the one to call, and the
counts of parsy_reach_get_info (known before any solve) are what a caller chooses by.
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
COLUMNS = ("workload", "n", "nrhs", "rows", "reach_share", "fwd_steps", "bwd_steps", "kernels", "sparse_ms", "full_ms", "wins")


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _median(torch, fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    return float(np.median([_timed(torch, fn) for _ in range(reps)]))


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
    plan.factor_device(vals.data_ptr(), L.data_ptr(), 0)
    torch.cuda.synchronize()
    assert plan.status() == 0
    picks = np.random.default_rng(0).choice(n, size=8, replace=False).astype(np.int32)
    out = []
    for nrhs in (1, 8):
        cols = picks[:nrhs]
        X = torch.zeros(n * nrhs, dtype=torch.float64, device=dev)

        def full():
            plan.solve_device(L.data_ptr(), X.data_ptr(), nrhs, n)
            plan.backsolve_device(L.data_ptr(), X.data_ptr(), nrhs, n)

        full_ms = _median(torch, full, reps)
        assert plan.solve_status() == 0
        bx = torch.ones(nrhs, dtype=torch.float64, device=dev)
        for label, rows in (("one", cols[:1]), ("all", None)):
            S = api.SparseSolve(plan, (np.arange(nrhs + 1, dtype=np.int32), cols), rows)
            d_x = torch.zeros(S.nx * nrhs, dtype=torch.float64, device=dev)

            def sparse():
                S.solve_device(L.data_ptr(), bx.data_ptr(), d_x.data_ptr(), S.nx, op="A")

            sparse_ms = _median(torch, sparse, reps)
            info = S.info()
            blocks = (nrhs + 7) // 8
            model = 8 * (info["fwd_entries"] + info["bwd_entries"]) * blocks
            row = {"workload": name, "n": n, "xsize": xsize, "nrhs": nrhs, "rows": label, "sparse_ms": sparse_ms,
                   "full_ms": full_ms, "wins": bool(sparse_ms < full_ms),
                   "reach_share": (info["fwd_entries"] + info["bwd_entries"]) / (2.0 * xsize),
                   "fwd_supernodes": info["fwd_supernodes"], "bwd_supernodes": info["bwd_supernodes"],
                   "fwd_steps": info["fwd_steps"], "bwd_steps": info["bwd_steps"], "kernels": info["last_kernels"],
                   "fwd_entries": info["fwd_entries"], "bwd_entries": info["bwd_entries"], "model_bytes": model,
                   "hbm_fraction": model / (sparse_ms * 1e-3) / 1e12 / HBM_PEAK_TB_PER_S, "device_bytes": info["device_bytes"]}
            print(json.dumps(row), flush=True)
            out.append(row)
            S.close()
    plan.close()
    return out


def table(rows) -> str:
    def cell(v):
        return f"{v:.3f}" if isinstance(v, float) else str(v)
    lines = ["  ".join(f"{c:>13}" for c in COLUMNS)]
    lines += ["  ".join(f"{cell(r[c]):>13}" for c in COLUMNS) for r in rows]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="ex15,parabolic_fem,nd24k,flan")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sparse_solve.json"))
    ap.add_argument("--table", default=str(ROOT / "profiles" / "sparse_solve.txt"))
    a = ap.parse_args()
    rows = []
    for name in a.workloads.split(","):
        rows += run(name, a.reps)
    for path, text in ((a.out, json.dumps(rows, indent=1) + "\n"), (a.table, table(rows))):
        Path(path).parent.mkdir(parents=True, exist_ok=True)
        Path(path).write_text(text)
    print(table(rows), end="")


if __name__ == "__main__":
    main()
