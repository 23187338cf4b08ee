"""Record which kernels the device solves of a source tree launch, by the kernel witness (needs a GPU).

    python tools/solve_witness_record.py [--tree DIR] --out FILE.json

For every point of the grid one forward or backward device solve is made and the non-zero witness counts are written
down.  The tool uses api.Plan, api.kernel_launches and api.reset_kernel_launches only, so any commit that has the witness
runs it unchanged (--tree: the checkout whose package and tests/solve_cases.py are used; default: this one).  Run on the
parent of a change to the solves' dispatch, the file is the record that tests/test_solve_route_host.py holds the change's
route to, point by point, without a GPU.

The grid: every (shape, plan_env) a cell of solve_cases.CELLS uses and every shape under L0, ONE and with
PARSY_SOLVE_ONE unset; times NRHS; times both directions; times the default gates and every distinct solve_env of the
cells.  And the workloads WORKLOADS of matrices.py with PARSY_SOLVE_ONE unset, the default gates, WORKLOAD_NRHS: their
block counts pass kOneSmallBlocks and kOneMidBlocks, which no shape of the catalogue can.

The file: "kernels" (the witness table's names), "counts" (the distinct results, each a list of [kernel index, launches]),
and "points": plan key -> solve-env key -> [forward, backward], each a list over the plan's nrhs list of indices into
"counts".  Keys are "name|VAR=value,..." and "VAR=value,..." with the variables sorted.
"""
import argparse
import json
import os
import sys
from pathlib import Path

NRHS = (1, 2, 4, 5, 6, 8, 9, 16, 17, 32, 33, 64, 65)
WORKLOADS = ("nd24k", "parabolic_fem")
WORKLOAD_NRHS = (1, 4, 5, 8, 9, 64)


def env_key(env):
    return ",".join(f"{k}={v}" for k, v in sorted(env.items()))


def grid(V):
    """[(shape name, plan_env)] and [solve_env] of the catalogue, in a fixed order."""
    plans, solves = [], [{}]
    for name in V.SHAPES:
        for env in (V.L0, V.ONE, {}):
            plans.append((name, dict(env)))
    for c in V.CELLS:
        if (c.shape, dict(c.plan_env)) not in plans:
            plans.append((c.shape, dict(c.plan_env)))
        if dict(c.solve_env) not in solves:
            solves.append(dict(c.solve_env))
    return plans, solves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=str(Path(__file__).resolve().parents[1]))
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    tree = Path(args.tree).resolve()
    sys.path[:0] = [str(tree), str(tree / "tests")]
    import numpy as np
    import torch
    import solve_cases as V
    from parsy_bench_amd import api, inspector as I, matrices as M

    dev = torch.device("cuda", 0)
    names = list(api.kernel_launches())
    counts, index, points = [], {}, {}

    def set_env(env):
        for k in V.VARIABLES:
            os.environ.pop(k, None)
        os.environ.update(env)

    def record(plan, n, lv, plan_env, solve_envs, nrhs_list):
        Ld = torch.from_numpy(lv).to(dev)
        out = {}
        for senv in solve_envs:
            set_env({**plan_env, **senv})
            both = []
            for forward in (True, False):
                row = []
                for nrhs in nrhs_list:
                    X = torch.from_numpy(np.random.default_rng(nrhs).standard_normal((nrhs, n))).to(dev)
                    torch.cuda.synchronize()
                    api.reset_kernel_launches()
                    (plan.solve_device if forward else plan.backsolve_device)(Ld.data_ptr(), X.data_ptr(), nrhs, n)
                    torch.cuda.synchronize()
                    seen = api.kernel_launches()
                    assert plan.solve_status() == 0, (plan_env, senv, nrhs, forward)
                    got = tuple((i, seen[k]) for i, k in enumerate(names) if seen[k])
                    if got not in index:
                        index[got] = len(counts)
                        counts.append([list(p) for p in got])
                    row.append(index[got])
                both.append(row)
            out[env_key(senv)] = both
        return out

    plans, solves = grid(V)
    for shape_name, plan_env in plans:
        shape = V.SHAPES[shape_name]
        A, S, sym = V.build(shape)
        set_env(plan_env)
        plan = api.Plan(sym, 0)
        lv, _ = plan.factor(V.values(shape, A, sym, False))
        assert plan.status() == 0, shape_name
        points[f"{shape_name}|{env_key(plan_env)}"] = record(plan, sym.n, lv, plan_env, solves, NRHS)
        print(f"{shape_name} {env_key(plan_env) or '-'}: done", flush=True)
    for name in WORKLOADS:
        A, perm = M.workload(name)
        sym = I.analyze(A, perm)
        set_env({})
        plan = api.Plan(sym, 0)
        lv, _ = plan.factor(sym.A2x)
        assert plan.status() == 0, name
        points[f"workload:{name}|"] = record(plan, sym.n, lv, {}, [{}], WORKLOAD_NRHS)
        print(f"workload {name}: done", flush=True)
    doc = {"nrhs": list(NRHS), "workload_nrhs": list(WORKLOAD_NRHS), "kernels": names, "counts": counts, "points": points}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, separators=(",", ":")) + "\n")
    print(f"{sum(len(r) for p in points.values() for b in p.values() for r in b)} solves, {len(counts)} distinct results -> {args.out}")


if __name__ == "__main__":
    main()
