"""The shapes of recut_cases.py factored on the device (the -m gpu tier), with the conflict domains re-cut and on the tile
grid (PARSY_BIG_RECUT=1 / 0), with their own values and under a bad symmetric scaling D A D: the measure of
test_factor_shapes_gpu.py -- the componentwise backward error rho_factor in units of u = 2^-53 against n + 1 --, bitwise
reproducibility, and the kernel witness: re-cut, (a) and (b) are full blocks and run through k_chol_dense.
test_recut_host.py pins the plans without a GPU."""
import numpy as np
import pytest

import recut_cases as RC
import shape_cases as SC
from parsy_bench_amd import inspector as I

pytestmark = pytest.mark.gpu

_RUNS = {}


def _run(api, monkeypatch, name, recut):
    """One plan per (case, knob), both sets of values factored through it, each twice.  Made once, never changed."""
    if (name, recut) not in _RUNS:
        case = RC.CASE_BY_NAME[name]
        A, S, sym = RC.build(case)
        RC.set_env(monkeypatch, case, recut)
        plan = api.Plan(sym, 0)
        run = {"sym": sym, "S": S, "info": plan.info, "domains": int((RC.big_tasks(plan)[:, 2] > 0).sum())}
        for scaled in (False, True):
            values = sym.permute_values(SC.scaled_values(A, 100 + case.seed)) if scaled else sym.A2x
            api.reset_kernel_launches()
            lv, _ = plan.factor(values)
            seen = api.kernel_launches()
            status = plan.status()
            lv2, _ = plan.factor(values)
            run[scaled] = {"lv": lv, "status": status, "again": bool(np.array_equal(lv, lv2)) and plan.status() == 0,
                           "seen": {k: seen[k] for k in SC.FACTOR_KERNELS}}
        _RUNS[(name, recut)] = run
    return _RUNS[(name, recut)]


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("recut", [False, True], ids=["tile", "recut"])
@pytest.mark.parametrize("name", RC.NAMES)
def test_factor_with_and_without_the_recut(api, monkeypatch, name, recut, scaled):
    run = _run(api, monkeypatch, name, recut)
    case, sym, got = RC.CASE_BY_NAME[name], run["sym"], run[scaled]
    assert got["status"] == 0, f"{name}: factor status {got['status']}"
    S = SC.scaled(run["S"], 100 + case.seed) if scaled else run["S"]
    rho = SC.rho_factor(S[np.ix_(sym.Perm, sym.Perm)], I.bcsc_to_dense(sym, got["lv"]))
    print(f"RHO_FACTOR case={name} recut={int(recut)} scaled={int(scaled)} n={sym.n} rho={rho:.3f} limit={SC.limit(sym.n)} "
          f"recut_tasks={run['domains']} seen={got['seen']}")
    assert rho <= SC.limit(sym.n), f"{name} recut={recut} scaled={scaled}: rho_factor = {rho:.4g} > n + 1 = {SC.limit(sym.n)}"
    assert got["again"], f"{name} recut={recut} scaled={scaled}: a second factorization is not bitwise the first"
    assert got["seen"]["k_chol_big"] + got["seen"]["k_chol_dense"] > 0
    assert (run["domains"] > 0) == (recut and name != "overlap")
    if recut and name in ("one_source", "same_rows"):
        # every BIG entry of these plans is a full block of a re-cut domain
        assert got["seen"]["k_chol_dense"] > 0 and got["seen"]["k_chol_big"] == 0, got["seen"]
        assert run["info"]["dense_entries"] == run["info"]["big_entries"] > 0


@pytest.mark.parametrize("name", RC.NAMES)
def test_the_two_cuts_agree_to_rounding(api, monkeypatch, name):
    """Re-classifying an entry moves it in the order of sums (dense entries of a task come first), so the factors need not
    be bitwise equal; each passes rho_factor above, and they agree normwise as the plans of other orders of sums do
    (test_factor_shapes_gpu.py: 1e-11).  Where the plans are equal (c) the factors are bitwise equal."""
    tile, cut = _run(api, monkeypatch, name, False), _run(api, monkeypatch, name, True)
    for scaled in (False, True):
        a, b = tile[scaled]["lv"], cut[scaled]["lv"]
        if name == "overlap":
            assert np.array_equal(a, b)
        d = SC.scaling(tile["sym"].n, 100 + RC.CASE_BY_NAME[name].seed)[tile["sym"].Perm] if scaled else None
        La, Lb = I.bcsc_to_dense(tile["sym"], a), I.bcsc_to_dense(tile["sym"], b)
        if scaled:   # (compare in the unscaled frame: the rows of L(D A D) = D L(A) differ by up to 2^40)
            La, Lb = La / d[:, None], Lb / d[:, None]
        err = np.abs(La - Lb).max() / np.abs(La).max()
        print(f"CUTS case={name} scaled={int(scaled)} err={err:.3e}")
        assert err <= 1e-11, f"{name} scaled={scaled}: {err:.3e}"
