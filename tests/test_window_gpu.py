"""The shapes of window_cases.py factored on the device (the -m gpu tier), on the tile grid and with the conflict domains of
differing rows cut in intervals, the tail guard off (PARSY_BIG_RECUT=0 / 3), with their own values and under a bad symmetric
scaling D A D: the measure of test_factor_shapes_gpu.py -- the componentwise backward error rho_factor in units of
u = 2^-53 against n + 1 --, bitwise reproducibility, agreement of the two cuts, and the kernel witness: in the nested case
the one interval task holds a full block (k_chol_dense) and a 64 x 64 window (k_chol_big).
test_window_host.py pins the plans without a GPU."""
import numpy as np
import pytest

import shape_cases as SC
import window_cases as WC
from parsy_bench_amd import inspector as I

pytestmark = pytest.mark.gpu

_RUNS = {}


def _run(api, monkeypatch, name, knob):
    """One plan per (case, knob), both sets of values factored through it, each twice.  Made once, never changed."""
    if (name, knob) not in _RUNS:
        case = WC.CASE_BY_NAME[name]
        A, S, sym = WC.build(case)
        WC.set_env(monkeypatch, case, knob)
        plan = api.Plan(sym, 0)
        run = {"sym": sym, "S": S, "info": plan.info, "check": plan.check(),
               "intervals": int((WC.big_tasks(plan)[:, 2] >= WC.INTERVAL).sum())}
        for scaled in (False, True):
            values = sym.permute_values(SC.scaled_values(A, 100 + case.seed)) if scaled else sym.A2x
            api.reset_kernel_launches()
            lv, _ = plan.factor(values)
            seen = api.kernel_launches()
            status = plan.status()
            lv2, _ = plan.factor(values)
            run[scaled] = {"lv": lv, "status": status, "again": bool(np.array_equal(lv, lv2)) and plan.status() == 0,
                           "seen": {k: seen[k] for k in SC.FACTOR_KERNELS}}
        _RUNS[(name, knob)] = run
    return _RUNS[(name, knob)]


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("knob", [0, 3], ids=["tile", "intervals"])
@pytest.mark.parametrize("name", WC.NAMES)
def test_factor_on_the_grid_and_in_intervals(api, monkeypatch, name, knob, scaled):
    run = _run(api, monkeypatch, name, knob)
    case, sym, got = WC.CASE_BY_NAME[name], run["sym"], run[scaled]
    assert run["check"] == 0
    assert got["status"] == 0, f"{name}: factor status {got['status']}"
    S = SC.scaled(run["S"], 100 + case.seed) if scaled else run["S"]
    rho = SC.rho_factor(S[np.ix_(sym.Perm, sym.Perm)], I.bcsc_to_dense(sym, got["lv"]))
    print(f"RHO_FACTOR case={name} knob={knob} scaled={int(scaled)} n={sym.n} rho={rho:.3f} limit={SC.limit(sym.n)} "
          f"interval_tasks={run['intervals']} seen={got['seen']}")
    assert rho <= SC.limit(sym.n), f"{name} knob={knob} scaled={scaled}: rho_factor = {rho:.4g} > n + 1 = {SC.limit(sym.n)}"
    assert got["again"], f"{name} knob={knob} scaled={scaled}: a second factorization is not bitwise the first"
    assert got["seen"]["k_chol_big"] + got["seen"]["k_chol_dense"] > 0
    assert (run["intervals"] > 0) == (knob == 3)
    if knob == 3 and name == "nested":
        assert got["seen"]["k_chol_dense"] > 0 and got["seen"]["k_chol_big"] > 0, got["seen"]


@pytest.mark.parametrize("name", WC.NAMES)
def test_the_two_cuts_agree_to_rounding(api, monkeypatch, name):
    """An entry that changes class moves in its task's order of sums (dense entries come first), so the factors need not be
    bitwise equal; each passes rho_factor above, and they agree normwise as the plans of other orders of sums do
    (test_factor_shapes_gpu.py: 1e-11), in the unscaled frame."""
    tile, cut = _run(api, monkeypatch, name, 0), _run(api, monkeypatch, name, 3)
    for scaled in (False, True):
        a, b = tile[scaled]["lv"], cut[scaled]["lv"]
        d = SC.scaling(tile["sym"].n, 100 + WC.CASE_BY_NAME[name].seed)[tile["sym"].Perm] if scaled else None
        La, Lb = I.bcsc_to_dense(tile["sym"], a), I.bcsc_to_dense(tile["sym"], b)
        if scaled:   # (compare in the unscaled frame: the rows of L(D A D) = D L(A) differ by up to 2^40)
            La, Lb = La / d[:, None], Lb / d[:, None]
        err = np.abs(La - Lb).max() / np.abs(La).max()
        print(f"CUTS case={name} scaled={int(scaled)} err={err:.3e}")
        assert err <= 1e-11, f"{name} scaled={scaled}: {err:.3e}"
