"""The factor and solve kernels on the engineered shapes of shape_cases.py (the -m gpu tier).

Every entry of the catalogue, with its own values and under a bad symmetric scaling D A D (D = diag(2^k), |k| <= 20):
the componentwise backward errors rho_factor / rho_solve in units of u = 2^-53, formed in extended precision, against
Higham's bound n + 1 (shape_cases.py says where it is from); the padding of the diagonal blocks; bitwise reproducibility;
the normwise comparison with the oracle; homogeneity under the scaling; and the kernel witness: which factor kernels
each entry launched, all seven between them.  test_shape_cases_host.py pins every entry to its schedule path without a GPU.

Every measured value is printed (pytest -rP shows it for passing tests) and stands in the assertion messages.
"""
import numpy as np
import pytest

import shape_cases as SC
from parsy_bench_amd import inspector as I

pytestmark = pytest.mark.gpu

FACTOR_TOL = 1e-11   # the normwise comparison of test_gpu_parity.py
NAMES = [c.name for c in SC.CASES]
_RUNS = {}
_DENSE = {}


def _values(case, sym, A, scaled):
    return sym.permute_values(SC.scaled_values(A, 100 + case.seed)) if scaled else sym.A2x


def _run(api, monkeypatch, name):
    """One plan per entry (its variables set while the plan is built), both sets of values factored through it, each
    twice; the witness of the first factorization.  Made once, never changed."""
    if name not in _RUNS:
        case = SC.CASE_BY_NAME[name]
        A, S, sym = SC.build(case)
        SC.set_env(monkeypatch, case.env)
        plan = api.Plan(sym, 0)
        run = {"case": case, "sym": sym, "plan": plan, "info": plan.info, "S": S, "A": A}
        for scaled in (False, True):
            values = _values(case, sym, A, scaled)
            api.reset_kernel_launches()
            lv, _ = plan.factor(values)
            seen = api.kernel_launches()
            status = plan.status()
            lv2, _ = plan.factor(values)
            run[scaled] = {"lv": lv, "status": status, "again": bool(np.array_equal(lv, lv2)) and plan.status() == 0,
                           "seen": {k: seen[k] for k in SC.FACTOR_KERNELS}}
        _RUNS[name] = run
    return _RUNS[name]


def _dense(run, scaled):
    key = (run["case"].name, scaled)
    if key not in _DENSE:
        _DENSE[key] = I.bcsc_to_dense(run["sym"], run[scaled]["lv"])
    return _DENSE[key]


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("name", NAMES)
def test_factor_on_engineered_shape(api, oracle, monkeypatch, name, scaled):
    run = _run(api, monkeypatch, name)
    case, sym, got = run["case"], run["sym"], run[scaled]
    lv = got["lv"]
    assert got["status"] == 0, f"{name}: factor status {got['status']}"
    S = SC.scaled(run["S"], 100 + case.seed) if scaled else run["S"]
    rho = SC.rho_factor(S[np.ix_(sym.Perm, sym.Perm)], _dense(run, scaled))
    print(f"RHO_FACTOR family={case.family} case={name} scaled={int(scaled)} n={sym.n} rho={rho:.3f} limit={SC.limit(sym.n)}")
    assert rho <= SC.limit(sym.n), f"{name} scaled={scaled}: rho_factor = {rho:.4g} > n + 1 = {SC.limit(sym.n)}"
    # the padding above the diagonal of every diagonal block is exactly zero
    for w, r, base in zip(np.diff(sym.super), [r for _, r in SC.supernodes_of(sym)], sym.p[sym.super[:-1]]):
        for c in range(1, int(w)):
            b = int(base) + c * r
            assert not lv[b: b + c].any(), f"{name}: padding of the diagonal block at column {c} of a supernode of width {w}"
    assert got["again"], f"{name} scaled={scaled}: a second factorization is not bitwise the first"
    if not scaled:
        ok, lo, _ = oracle.cholesky_05(sym, sym.A2x, I.trivial_hlevel(sym))
        assert ok
        err = np.abs(lv - lo).max() / np.abs(lo).max()
        print(f"NORMWISE case={name} err={err:.3e}")
        assert err <= FACTOR_TOL, f"{name}: max|L - L_oracle| / max|L| = {err:.3e}"


@pytest.mark.parametrize("name", NAMES)
def test_factor_is_homogeneous_under_scaling(api, monkeypatch, name):
    """L(D A D) == D L(A) bitwise, D = diag(2^k): a pivot scaled by 4^k keeps its mantissa through the reciprocal square
    root and its correction step, and every other operation is a product or a fused multiply-add of terms that carry the
    same power of two."""
    run = _run(api, monkeypatch, name)
    sym = run["sym"]
    assert run[False]["status"] == 0 and run[True]["status"] == 0
    d = SC.scaling(sym.n, 100 + run["case"].seed)[sym.Perm]
    want = d[:, None] * _dense(run, False)
    got = _dense(run, True)
    diff = int((want != got).sum())
    print(f"SCALING case={name} entries_that_differ={diff}")
    assert diff == 0, f"{name}: {diff} entries of L(D A D) differ from D L(A); first at {np.argwhere(want != got)[0]}"


@pytest.mark.parametrize("one", ["default", "0"])
@pytest.mark.parametrize("name", NAMES)
def test_solves_on_engineered_shape(api, monkeypatch, name, one):
    """Forward and backward, 1, 3 and 17 right-hand sides, with the plan's own factor (plain and scaled): rho_solve of
    every column; under the default gates (one launch per solve on plans this small) and with the level launches
    (PARSY_SOLVE_ONE=0, read when the plan is built)."""
    run = _run(api, monkeypatch, name)
    case, sym = run["case"], run["sym"]
    plan = run["plan"]
    if one == "0":
        SC.set_env(monkeypatch, {**case.env, "PARSY_SOLVE_ONE": "0"})
        plan = api.Plan(sym, 0)
        assert plan.info["solve_one"] == 0
    n = sym.n
    worst = {}
    for scaled in (False, True):
        assert run[scaled]["status"] == 0
        lv, Ld = run[scaled]["lv"], _dense(run, scaled)
        for nrhs in (1, 3, 17):
            B = np.random.default_rng(1000 * nrhs + case.seed).standard_normal((n, nrhs))
            for forward in (True, False):
                arg = B[:, 0] if nrhs == 1 else B
                X, _ = plan.solve(lv, arg) if forward else plan.solve2(lv, arg, forward=False)
                assert plan.solve_status() == 0
                rho = SC.rho_solve(Ld if forward else Ld.T, X, B)
                what = f"{name} scaled={scaled} {'forward' if forward else 'backward'} nrhs={nrhs} PARSY_SOLVE_ONE={one}"
                assert rho.max() <= SC.limit(n), f"{what}: rho_solve = {rho.max():.4g} (column {int(rho.argmax())}) > n + 1 = {SC.limit(n)}"
                key = "forward" if forward else "backward"
                worst[key] = max(worst.get(key, 0.0), float(rho.max()))
    print(f"RHO_SOLVE family={case.family} case={name} one={one} n={n} forward={worst['forward']:.3f} "
          f"backward={worst['backward']:.3f} limit={SC.limit(n)}")


def test_factor_coverage_reaches_every_factor_kernel(api, monkeypatch):
    """The witness of every entry's factorization: the kernels the entry must launch, those it must not, and all seven
    factor kernels between the entries, none excepted."""
    union = dict.fromkeys(SC.FACTOR_KERNELS, 0)
    for name in NAMES:
        run = _run(api, monkeypatch, name)
        case, info = run["case"], run["info"]
        for scaled in (False, True):
            seen = run[scaled]["seen"]
            must = {"k_scatter_a", *case.kernels}
            never = set(case.absent)
            if "PARSY_BIG_MINK" not in case.env:
                never |= {"k_chol_big", "k_chol_dense"}
            if case.env.get("PARSY_BIG_DENSE") == "4":   # (the ragged kernel keeps the entries of K < 8 only)
                (must if info["big_entries"] > info["dense_entries"] else never).add("k_chol_big")
            if case.family != "g":
                never.add("k_chol_chain_rows")
            assert not must & never
            assert all(seen[k] > 0 for k in must) and not any(seen[k] for k in never), (name, seen, sorted(must), sorted(never))
            if not scaled:
                print(f"WITNESS case={name} {seen}")
            for k, v in seen.items():
                union[k] += v
    assert set(union) == set(SC.FACTOR_KERNELS)
    missing = sorted(k for k, v in union.items() if v == 0)
    assert not missing, f"factor kernels no entry reached: {missing}"


def _factor_with(api, monkeypatch, case, **override):
    A, S, sym = SC.build(case)
    SC.set_env(monkeypatch, {**case.env, **override})
    plan = api.Plan(sym, 0)
    lv, _ = plan.factor(sym.A2x)
    assert plan.status() == 0
    return plan.info, lv


@pytest.mark.parametrize("sup", ["2", "2x1"])
def test_super_tiles_are_bitwise_single_tiles(api, monkeypatch, sup):
    """Which task forms a product changes nothing in its value, and the sources keep their order (PARSY_BIG_DENSE=0: which
    entries are dense blocks depends on the windows)."""
    case = SC.CASE_BY_NAME["big_ragged"]
    info1, lv1 = _factor_with(api, monkeypatch, case, PARSY_BIG_SUPER="1")
    info, lv = _factor_with(api, monkeypatch, case, PARSY_BIG_SUPER=sup)
    assert 0 < info["big_tasks"] < info1["big_tasks"] and info["big_flops"] == info1["big_flops"]
    assert np.array_equal(lv, lv1)
    assert np.array_equal(lv1, _run(api, monkeypatch, "big_ragged")[False]["lv"])


@pytest.mark.parametrize("name,base", [("tiles_130_split", "tiles_130"), ("big_ragged_split", "big_ragged")])
def test_split_chain_launches_are_bitwise_one_launch(api, monkeypatch, name, base):
    split, whole = _run(api, monkeypatch, name), _run(api, monkeypatch, base)
    assert split["info"]["chol_launches"] > whole["info"]["chol_launches"]
    for scaled in (False, True):
        assert np.array_equal(split[scaled]["lv"], whole[scaled]["lv"])


@pytest.mark.parametrize("names", [("streams_split", "streams_whole"), ("push_1", "push_2", "push_3")])
def test_other_orders_of_sums_agree_to_rounding(api, monkeypatch, names):
    """Split early streams and the groups of the pushes change the order of sums: each plan passes rho_factor and is
    bitwise reproducible (test_factor_on_engineered_shape); here the plans differ and their factors agree to rounding."""
    runs = [_run(api, monkeypatch, k) for k in names]
    ref = runs[0][False]["lv"]
    for r in runs[1:]:
        err = np.abs(r[False]["lv"] - ref).max() / np.abs(ref).max()
        assert err <= FACTOR_TOL, f"{names}: {err:.3e}"
    infos = [r["info"] for r in runs]
    assert len({(i["split_parts"], i["big_tasks"], i["big_entries"]) for i in infos}) == len(infos)
