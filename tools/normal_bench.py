"""Times of the normal-matrix calls (api.NormalEquations) next to the same plan's factorization and solve pair, with
device events: medians of --reps after a warm-up, everything of a workload in one process.

Usage: python tools/normal_bench.py [--workloads ex15,parabolic_fem,nd24k,flan] [--reps 20]
                                    [--out profiles/normal_bench.json]

F is grid_edges on the 5-point plans (ex15, parabolic_fem) and grid_cells on the 27-point ones (nd24k, flan), so the
workloads' own plans serve without a new analysis.  Weights uniform in (0.5, 1.5), beta = the workload's shift.
Per workload (ms):
  values_ms      -- one parsy_normal_values_device call (w given, beta, no A0)
  model_bytes    -- 12 bytes of triples per pair + 8 bytes per entry written (the gathers of fx and w are not counted:
                    they live in L2 / Infinity Cache)
  pairs_per_s, tb_per_s, hbm_fraction -- pairs and model_bytes over values_ms; the latter over HBM_PEAK_TB_PER_S
  f_ms[nrhs], ft_ms[nrhs] -- parsy_normal_apply_device at nrhs = 1 and 8; their model: 16 (F: rpos, rcol, fx) or 12
                    (F': fi, fx) bytes per entry of F + 8 bytes per element of X and Y
  lstsq_ms       -- parsy_lsq_solve_device, nrhs = 1, steps = 1, with r and g: two solve pairs, three products by F,
                    two by F'
  factor_ms, solve_pair_ms -- the yardsticks: parsy_factor_device on the assembled values, one forward + backward solve
  inspector_s    -- host seconds of parsy_normal_create (once per pattern)
A workload whose factor does not fit the device's memory is skipped with a note.  The output file is
{"kernel_resources": ..., "rows": [...]}: a run replaces the rows of its own workloads and keeps the rest.
"""
import argparse
import json
import sys
import time
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


def run(name, reps):
    import torch
    nx, ny, nz, stencil, shift = M.WORKLOADS[name]
    A, perm = M.workload(name)
    sym = I.analyze(A, perm)
    n, xsize, nnzA = sym.n, int(sym.xsize), int(A.nnz)
    dev = torch.device("cuda", 0)
    free, _ = torch.cuda.mem_get_info(dev)
    if 8 * xsize * 1.5 > free:
        print(json.dumps({"workload": name, "skipped": f"lValues is {8 * xsize / 1e9:.1f} GB, {free / 1e9:.1f} GB free"}), flush=True)
        return []
    F = M.grid_edges(nx, ny, nz) if stencil in (5, 7) else M.grid_cells(nx, ny, nz)
    plan = api.Plan(sym, 0)
    t0 = time.perf_counter()
    ne = api.NormalEquations(plan, F)
    inspector_s = time.perf_counter() - t0
    info = ne.info
    rng = np.random.default_rng(1)
    d_fx = torch.from_numpy(F.data).to(dev)
    d_w = torch.from_numpy(rng.uniform(0.5, 1.5, F.m)).to(dev)
    vals = torch.empty(nnzA, dtype=torch.float64, device=dev)
    L = torch.empty(xsize, dtype=torch.float64, device=dev)

    def values():
        ne.values_device(d_fx.data_ptr(), vals.data_ptr(), d_w=d_w.data_ptr(), beta=shift)

    def factor():
        plan.factor_device(vals.data_ptr(), L.data_ptr(), 0)

    values()
    factor()
    torch.cuda.synchronize()
    assert plan.status() == 0
    values_ms = _events(torch, values, reps)
    factor_ms = _events(torch, factor, reps)
    nbytes = 12 * info["pairs"] + 8 * nnzA
    row = {"workload": name, "n": n, "m": F.m, "nnzF": info["nnzF"], "nnzA": nnzA, "pairs": info["pairs"],
           "longest_list": info["longest_list"], "class_entries": info["class_entries"], "chunks": info["chunks"],
           "entries_untouched": info["entries_untouched"], "launches": info["launches"], "inspector_s": inspector_s,
           "values_ms": values_ms, "model_bytes": nbytes, "pairs_per_s": info["pairs"] / (values_ms * 1e-3),
           "tb_per_s": nbytes / (values_ms * 1e-3) / 1e12,
           "hbm_fraction": nbytes / (values_ms * 1e-3) / 1e12 / HBM_PEAK_TB_PER_S, "factor_ms": factor_ms}
    xs = torch.from_numpy(rng.standard_normal(max(n, F.m) * 8)).to(dev)
    ys = torch.empty(max(n, F.m) * 8, dtype=torch.float64, device=dev)
    for op, nxr, nyr, per in (("F", F.m, n, 16), ("FT", n, F.m, 12)):
        for nrhs in (1, 8):
            def product():
                ne.apply_device(op, d_fx.data_ptr(), xs.data_ptr(), nxr, nrhs, ys.data_ptr(), nyr, d_w=d_w.data_ptr())
            product()
            torch.cuda.synchronize()
            ms = _events(torch, product, reps)
            b = per * info["nnzF"] + 8 * (n + F.m) * nrhs
            row[f"{op.lower()}_ms_{nrhs}"] = ms
            row[f"{op.lower()}_hbm_fraction_{nrhs}"] = b / (ms * 1e-3) / 1e12 / HBM_PEAK_TB_PER_S
    c = torch.from_numpy(rng.standard_normal(F.m)).to(dev)
    x = torch.empty(n, dtype=torch.float64, device=dev)
    r = torch.empty(F.m, dtype=torch.float64, device=dev)
    g = torch.empty(n, dtype=torch.float64, device=dev)

    def lstsq():
        ne.lstsq_device(d_fx.data_ptr(), L.data_ptr(), c.data_ptr(), F.m, x.data_ptr(), n, 1, steps=1, d_w=d_w.data_ptr(),
                        beta=shift, d_r=r.data_ptr(), ldr=F.m, d_g=g.data_ptr(), ldg=n)

    def solve_pair():
        plan.solve_device(L.data_ptr(), x.data_ptr(), 1, n, 0)
        plan.backsolve_device(L.data_ptr(), x.data_ptr(), 1, n, 0)

    lstsq()
    torch.cuda.synchronize()
    assert plan.solve_status() == 0
    gn, cn = float(g.abs().max()), float(c.abs().max())
    row["lstsq_ms"] = _events(torch, lstsq, reps)
    row["lstsq_gradient_over_c"] = gn / cn
    x.fill_(1.0)
    solve_pair()
    torch.cuda.synchronize()
    row["solve_pair_ms"] = _events(torch, solve_pair, reps)
    row["device_bytes"] = ne.info["device_bytes"]
    print(json.dumps(row), flush=True)
    ne.close()
    plan.close()
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="ex15,parabolic_fem,nd24k,flan")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "normal_bench.json"))
    a = ap.parse_args()
    if api.device_count() < 1:
        raise SystemExit("normal_bench: no HIP device visible (times come from the device only)")
    rows = []
    for name in a.workloads.split(","):
        rows += run(name, a.reps)
    # the file keeps what it holds besides these workloads' rows: the rows of other runs (the Flan-class input usually
    # runs by itself) and "kernel_resources", the compiler's report on the kernels, recorded by hand
    out = Path(a.out)
    doc = json.loads(out.read_text()) if out.exists() else {}
    done = {r["workload"] for r in rows}
    doc["rows"] = [r for r in doc.get("rows", []) if r["workload"] not in done] + rows
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
