"""The dispatch of the solves (csrc/solve_route.hpp) without a GPU.

* It is in one place: no launch function of the trsv sources names a gate, the executor names none that chooses a kernel,
  and the gates are read in solve_route.cpp only.
* It is the parent's: tests/golden/solve_route_parent_witness.json holds the witness counts of one device solve per point
  of a grid, recorded on an MI355X by tools/solve_witness_record.py in a checkout of the commit before the route
  existed.  The route of a host-only plan (parsy_debug_solve_route) gives exactly those counts at every point.
* It agrees with the tests' independent copy, solve_cases.predict, at every point of the grid that names its ONE-launch
  mode.
* tests/solve_route_check.cpp holds routes of plans with every launch kind and form to their invariants under the address
  and undefined-behaviour sanitizers, stand-alone.
"""
import json
import re
import subprocess
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import solve_cases as V
from conftest import problem
from parsy_bench_amd import api
from test_kernel_witness import CSRC, SOLVE_SOURCES, source_text

ROOT = Path(__file__).resolve().parents[1]
RECORD = json.loads((ROOT / "tests" / "golden" / "solve_route_parent_witness.json").read_text())
SHAPE_KEYS = [k for k in RECORD["points"] if not k.startswith("workload:")]
WORKLOAD_KEYS = [k for k in RECORD["points"] if k.startswith("workload:")]


def _env(key):
    return dict(kv.split("=", 1) for kv in key.split(",") if kv)


# ---------------------------------------------------------------------------
# one place
# ---------------------------------------------------------------------------
def test_dispatch_is_in_one_place():
    gates = re.search(r"struct SolveGates \{(.*?)\};", source_text(CSRC / "solve_route.hpp"), flags=re.S).group(1)
    fields = set(re.findall(r"(?:int|bool) (\w+) =", gates))
    assert len(fields) == 13 and {"wait_bias", "sub_abl", "mrhs_min", "xt_min_set"} <= fields, fields
    sources = sorted(CSRC.glob(SOLVE_SOURCES))
    assert len(sources) == 4
    for src in sources:
        text = source_text(src)
        assert not re.search(r"\bgates\b|\bSolveGates\b", text), f"{src.name} names the gates"
        assert not [f for f in fields - {"wait_bias", "sub_abl"} if re.search(rf"\b{f}\b", text)], src.name
    executor = source_text(CSRC / "executor.hip")
    named = {f for f in fields if re.search(rf"\b{f}\b", executor)}
    assert named <= {"wait_bias", "sub_abl"}, f"executor.hip names the gates {sorted(named)}"
    defined = [src.name for src in sorted(CSRC.iterdir()) if src.suffix in (".hip", ".hpp", ".cpp")
               and re.search(r"SolveGates\s+read_solve_gates\s*\(\s*\)\s*\{", source_text(src))]
    assert defined == ["solve_route.cpp"], defined
    # (no device pattern carries gates any more; the route's source is host C++: no HIP header)
    assert "gates" not in re.search(r"struct DevicePattern \{(.*?)\n\};", source_text(CSRC / "kernels.hpp"), flags=re.S).group(1)
    for name in ("solve_route.hpp", "solve_route.cpp"):
        assert not re.search(r"#include\s*[<\"]hip", source_text(CSRC / name)), name
    from parsy_bench_amd import build
    assert "solve_route.cpp" in build.HOST_SOURCES


# ---------------------------------------------------------------------------
# the parent's record, and the independent copy
# ---------------------------------------------------------------------------
def test_record_is_the_grid():
    """The record holds every point the grid of tools/solve_witness_record.py has with today's catalogue."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("solve_witness_record", ROOT / "tools" / "solve_witness_record.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    plans, solves = tool.grid(V)
    assert RECORD["kernels"] == list(api.kernel_launches()) and tuple(RECORD["nrhs"]) == tool.NRHS
    assert tuple(RECORD["workload_nrhs"]) == tool.WORKLOAD_NRHS
    assert SHAPE_KEYS == [f"{name}|{tool.env_key(env)}" for name, env in plans]
    assert {(c.shape, tool.env_key(c.plan_env)) for c in V.CELLS} <= {tuple(k.split("|")) for k in SHAPE_KEYS}
    for name in V.SHAPES:
        assert {f"{name}|{tool.env_key(e)}" for e in (V.L0, V.ONE, {})} <= set(SHAPE_KEYS)
    want = [tool.env_key(e) for e in solves]
    assert {tool.env_key(c.solve_env) for c in V.CELLS} | {""} == set(want)
    for key in SHAPE_KEYS:
        assert list(RECORD["points"][key]) == want, key
        assert all(len(rows) == 2 and all(len(r) == len(tool.NRHS) for r in rows) for rows in RECORD["points"][key].values())
    assert WORKLOAD_KEYS == [f"workload:{w}|" for w in tool.WORKLOADS]
    for key in WORKLOAD_KEYS:
        assert list(RECORD["points"][key]) == [""] and all(len(r) == len(tool.WORKLOAD_NRHS) for r in RECORD["points"][key][""])


def _recorded(index):
    return Counter({RECORD["kernels"][k]: c for k, c in RECORD["counts"][index]})


def _check_plan(monkeypatch, key, sym, nrhs_list, against_predict):
    plan_env = _env(key.split("|", 1)[1])
    V.set_env(monkeypatch, plan_env)
    plan = api.Plan(sym, -1)
    assert plan.check() == 0
    info, tables = plan.info, V.launch_tables(plan)
    wrong, points = [], 0
    for solve_key, rows in RECORD["points"][key].items():
        solve_env = _env(solve_key)
        V.set_env(monkeypatch, {**plan_env, **solve_env})
        for forward, row in zip((True, False), rows):
            for nrhs, index in zip(nrhs_list, row):
                route = V.route(plan, nrhs, sym.n, forward)
                points += 1
                if Counter(route) != _recorded(index):
                    wrong.append((key, solve_key, nrhs, forward, "route", dict(Counter(route)), "recorded", dict(_recorded(index))))
                if against_predict and plan_env.get("PARSY_SOLVE_ONE") in ("0", "2"):
                    pred = V.predict(info, tables, plan_env, solve_env, nrhs, forward)
                    if set(route) != pred:
                        wrong.append((key, solve_key, nrhs, forward, "route", sorted(set(route)), "predict", sorted(pred)))
    assert not wrong, wrong[:6]
    return points


@pytest.mark.parametrize("key", SHAPE_KEYS)
def test_route_is_the_parents_record_and_the_prediction(monkeypatch, key):
    """At every recorded point of the plan: Counter(route) == the parent's witness counts, exactly; and where the plan
    names its ONE-launch mode, the set of the route's names == solve_cases.predict."""
    A, S, sym = V.build(V.SHAPES[key.split("|")[0]])
    assert _check_plan(monkeypatch, key, sym, RECORD["nrhs"], True) == 2 * len(RECORD["nrhs"]) * len(RECORD["points"][key])


@pytest.mark.parametrize("key", WORKLOAD_KEYS)
def test_route_of_a_workload_is_the_parents_record(monkeypatch, key):
    """nd24k and parabolic_fem with PARSY_SOLVE_ONE unset: block counts past kOneSmallBlocks and kOneMidBlocks."""
    A, perm, sym = problem(key.split("|")[0].split(":")[1])
    assert _check_plan(monkeypatch, key, sym, RECORD["workload_nrhs"], False) == 2 * len(RECORD["workload_nrhs"])


def test_route_export(monkeypatch):
    """parsy_debug_solve_route: the count whatever the capacity, at most cap entries written, arguments checked; the gates are
    read at the call."""
    from parsy_bench_amd import _native as N
    V.set_env(monkeypatch, V.L0)
    A, S, sym = V.build(V.SHAPES["tall_65"])
    plan = api.Plan(sym, -1)
    full = V.route(plan, 2, sym.n, True)
    assert len(full) > 2 and full[:2] == ["k_solve_arm_wide", "k_diag_inverse"]
    f = N.lib().parsy_debug_solve_route
    out = np.full(len(full), -7, dtype=np.int32)
    assert f(plan._h, 2, sym.n, 0, out.ctypes.data, len(full) - 1) == len(full)
    assert out[-1] == -7 and (out[:-1] >= 0).all()
    assert f(plan._h, 0, sym.n, 0, None, 0) == -1 and f(plan._h, 1, sym.n - 1, 0, None, 0) == -1
    assert "k_solve_chain_w<2>" in V.route(plan, 1, sym.n, True)
    monkeypatch.setenv("PARSY_CHAIN_FEW_CHUNKS", "0")
    assert "k_solve_chain_w<4>" in V.route(plan, 1, sym.n, True) and "k_solve_chain_w<2>" not in V.route(plan, 1, sym.n, True)
    # in steps of levels: the prologue in the first step, between them every launch of the one-call route
    monkeypatch.delenv("PARSY_CHAIN_FEW_CHUNKS")
    nl = int(plan.solve_levels().max()) + 1
    for forward in (True, False):
        steps = [V.route_levels(plan, 1, sym.n, forward, lev, lev + 1, k == 0, k == nl - 1)
                 for k, lev in enumerate(range(nl) if forward else range(nl - 1, -1, -1))]
        assert steps[0][0] == "k_diag_inverse" and all("k_diag_inverse" not in s for s in steps[1:])
        assert Counter(k for s in steps for k in s) == Counter(V.route(plan, 1, sym.n, forward))


# ---------------------------------------------------------------------------
# under the sanitizers, stand-alone
# ---------------------------------------------------------------------------
def test_routes_under_the_sanitizers(tmp_path):
    from parsy_bench_amd.build import _hipcc
    exe = tmp_path / "solve_route_check"
    # (the sanitizers are for the host compilation only: -Xarch_host keeps them off any device pass of the driver)
    cmd = [_hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-g", "-O0", f"-I{CSRC}", str(ROOT / "tests" / "solve_route_check.cpp"),
           *(str(CSRC / s) for s in ("solve_route.cpp", "schedule.cpp", "inspector.cpp", "gen.cpp")), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "solve_route:" in ran.stdout and "every routed kernel seen" in ran.stdout
