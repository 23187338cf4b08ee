"""Solves with sparse right-hand sides for selected rows on the device (api.SparseSolve, Plan.inverse_entries,
api.blockedPrunedLSolve) on the cases of sparse_solve_cases.py.  The factor is the plan's own.

Limits (theorems, independent of the order of the sums; nothing is measured -- shape_cases.py, Higham Thm 8.5 / 10.4):
GINV and GINVT within n + 1 units of u componentwise (rho_solve), A and inverse_entries within 3 n + 2 (rho_spd: the
factor as the device holds it, extended precision, rows with a zero denominator exactly zero).  Equality as numbers
(np.array_equal) wherever the interface promises the same arithmetic.  Every measured value is printed (pytest -rP).
"""
import numpy as np
import pytest

import shape_cases as SC
import sparse_solve_cases as SPC
import sparse_solve_ref as SR

pytestmark = pytest.mark.gpu

NAMES = list(SPC.CASE_BY_NAME)
_CTX, _INV_PLANS, _SOLVED = {}, {}, {}
_SENTINEL = -7.25e300


def _ctx(api, name):
    """The case on the device, made once: the plan under the case's ordering, its own factor (lValues and dense), and a
    full solve of the plan to compare with after the sparse calls."""
    if name not in _CTX:
        made = dict(SPC.make(SPC.CASE_BY_NAME[name]))
        plan = api.Plan(made["sym"], 0)
        plan.set_perm(made["perm"])
        lv, _ = plan.factor(made["values"])
        assert plan.status() == 0
        rhs = np.random.default_rng(5).standard_normal((made["n"], 3))
        made.update(plan=plan, lv=lv, L=SR.dense_factor(made["sym"], lv), rhs=rhs, back=plan.solve2(lv, rhs, forward=False)[0])
        _CTX[name] = made
    return _CTX[name]


def _handle(api, c, xrows, pattern=None):
    bp, bi = pattern if pattern is not None else (c["bp"], c["bi"])
    return api.SparseSolve(c["plan"], (bp, bi), SPC.caller_rows(c, xrows))


def _solve(api, c, op, xkind):
    """X of the case's own B for an op and a kind of Xset, solved once per (case, op, kind) and left unchanged."""
    key = (c["case"].name, op, xkind)
    if key not in _SOLVED:
        h = _handle(api, c, SPC.xset_rows(c["sym"], xkind))
        _SOLVED[key] = h.solve(c["lv"], c["bx"], op=op)[0]
        h.close()
    return _SOLVED[key]


def _to_factor(c, X):
    """An all-rows result (rows in the caller's ordering) in the factor's ordering."""
    return X if c["perm"] is None else X[c["perm"], :]


def _undisturbed(c):
    """Nothing of the plan was disturbed.  The plan's backward solve has one order for every sum (test_solve_shapes_gpu.py):
    it gives the bits it gave before the first sparse call.  Its forward solve adds the chain's updates by float atomics
    and does not give the same bits twice even with nothing in between (measured on an MI355X, a fresh plan and no
    sparse call: 3 of 5 repeats of sp_widths-perm-8 and 5 of 5 of sp_widths-id-9 and chain-id-9 differ from the first
    run, every backward repeat equals it), so the full solve is held to its error limit, 3 n + 2 units of u, instead."""
    plan, n = c["plan"], c["n"]
    again = plan.solve2(c["lv"], c["rhs"], forward=False)[0]
    assert plan.solve_status() == 0
    assert np.array_equal(again, c["back"]), "the plan's backward solve changed its bits after a sparse call"
    full = plan.solve2(c["lv"], c["rhs"], forward=True)[0]
    assert plan.solve_status() == 0
    rho = SR.rho_spd(c["L"], full, c["rhs"])
    assert (rho <= 3 * n + 2).all(), ("the plan's full solve after a sparse call", rho, 3 * n + 2)


@pytest.mark.parametrize("name", NAMES)
def test_ginv_all_rows_within_the_limit_and_zero_outside_the_reach(api, name):
    c = _ctx(api, name)
    sym, n = c["sym"], c["n"]
    Yf = _to_factor(c, _solve(api, c, "GINV", "all"))
    rho = SC.rho_solve(c["L"], Yf, c["Bf"])
    print(f"{name}: GINV rho = {rho.max():.2f} u (limit {n + 1})")
    assert (rho <= n + 1).all(), (rho, n + 1)
    for q, seeds in enumerate(c["seeds"]):
        inside = np.zeros(n, dtype=bool)
        inside[SR.columns_of(sym, SR.closure(sym, seeds))] = True
        assert not Yf[~inside, q].any(), f"column {q}: a non-zero outside the closure of its own seeds"
        if not seeds:
            assert not Yf[:, q].any(), "an empty column of B gives a column of exactly zero"
    _undisturbed(c)


@pytest.mark.parametrize("name", NAMES)
def test_ginvt_on_the_columns_of_the_reach_within_the_limit(api, name):
    c = _ctx(api, name)
    sym, n = c["sym"], c["n"]
    for xkind in SPC.XSETS:
        K = SPC.reaches(c, SPC.xset_rows(sym, xkind))[1]
        cols = SR.columns_of(sym, K)
        h = _handle(api, c, cols)          # the same reach, every column of it selected
        assert h.reach()[1].tolist() == K
        X = h.solve(c["lv"], c["bx"], op="GINVT")[0]
        h.close()
        Lt = c["L"].T[np.ix_(cols, cols)]
        assert not c["L"].T[np.ix_(cols, np.setdiff1d(np.arange(n), cols))].any(), "row j of L' has its non-zeros in C"
        rho = SC.rho_solve(Lt, X, c["Bf"][cols, :])
        print(f"{name}/{xkind}: GINVT rho = {rho.max():.2f} u on {cols.size} columns (limit {n + 1})")
        assert (rho <= n + 1).all(), (xkind, rho, n + 1)
    _undisturbed(c)


@pytest.mark.parametrize("name", NAMES)
def test_a_all_rows_within_the_limit(api, name):
    c = _ctx(api, name)
    n = c["n"]
    Xf = _to_factor(c, _solve(api, c, "A", "all"))
    rho = SR.rho_spd(c["L"], Xf, c["Bf"])
    print(f"{name}: A rho = {rho.max():.2f} u (limit {3 * n + 2})")
    assert (rho <= 3 * n + 2).all(), (rho, 3 * n + 2)
    for q, seeds in enumerate(c["seeds"]):
        if not seeds:
            assert not Xf[:, q].any(), "an empty column of B gives a column of exactly zero"
    _undisturbed(c)


def _inv_plan(api, c):
    """A plan of the case's pattern that inverse_entries may give sym.Perm to (the case's own keeps its ordering)."""
    key = c["shape"].name
    if key not in _INV_PLANS:
        _INV_PLANS[key] = api.Plan(c["sym"], 0)
    return _INV_PLANS[key]


@pytest.mark.parametrize("name", NAMES)
def test_inverse_entries(api, name):
    c = _ctx(api, name)
    sym, n = c["sym"], c["n"]
    P = np.asarray(sym.Perm)
    plan = _inv_plan(api, c)
    fcols = sorted({0, int(sym.super[sym.nsuper - 1]), n - 1, n // 2, int(sym.super[1]) - 1 if sym.nsuper > 1 else 1})
    cols = P[fcols]                                     # the caller's ordering is A's own here
    Z = plan.inverse_entries(c["lv"], np.arange(n), cols)
    assert Z.shape == (n, len(fcols))
    E = np.zeros((n, len(fcols)))
    E[fcols, np.arange(len(fcols))] = 1.0
    rho = SR.rho_spd(c["L"], Z[P, :], E)
    print(f"{name}: inverse_entries rho = {rho.max():.2f} u (limit {3 * n + 2})")
    assert (rho <= 3 * n + 2).all(), (rho, 3 * n + 2)
    rows = P[SPC.xset_rows(sym, "dozen", seed=1)]
    assert np.array_equal(plan.inverse_entries(c["lv"], rows, cols), Z[rows, :]), "a block against the all-rows block"
    assert np.array_equal(plan.inverse_entries(c["lv"], rows[:1], cols[-1:]), Z[rows[:1], -1:]), "a single entry"


@pytest.mark.parametrize("name", NAMES)
def test_same_call_twice_and_every_column_alone(api, name):
    c = _ctx(api, name)
    sym = c["sym"]
    for op, xkind in (("A", "all"), ("GINVT", "dozen"), ("GINV", "all")):
        X = _solve(api, c, op, xkind)
        xrows = SPC.xset_rows(sym, xkind)
        h = _handle(api, c, xrows)
        assert np.array_equal(h.solve(c["lv"], c["bx"], op=op)[0], X), f"{op}: the same call twice"
        assert np.array_equal(h.solve(c["lv"], c["bx"], op=op)[0], X), f"{op}: ... and a third time on one handle"
        h.close()
        for q in range(c["case"].nrhs):
            lo, hi = int(c["bp"][q]), int(c["bp"][q + 1])
            h1 = _handle(api, c, xrows, (np.array([0, hi - lo], np.int32), c["bi"][lo:hi]))
            X1 = h1.solve(c["lv"], c["bx"][lo:hi], op=op)[0]
            h1.close()
            assert np.array_equal(X1[:, 0], X[:, q]), f"{op}: column {q} alone differs from the block call"
    _undisturbed(c)


@pytest.mark.parametrize("name", NAMES)
def test_subset_of_rows_against_all_rows(api, name):
    c = _ctx(api, name)
    sym = c["sym"]
    for op in ("A", "GINVT", "GINV"):
        Xall = _solve(api, c, op, "all")
        for xkind in ("leaf", "border", "dozen"):
            rows = SPC.caller_rows(c, SPC.xset_rows(sym, xkind))
            assert np.array_equal(_solve(api, c, op, xkind), Xall[rows, :]), f"{op}/{xkind}: differs from the all-rows call"


@pytest.mark.parametrize("name", NAMES)
def test_superset_pattern_with_zeros_changes_nothing(api, name):
    c = _ctx(api, name)
    sym = c["sym"]
    sup = np.asarray(sym.super)
    have = set(c["seeds"][0])
    extra = [int(sup[s]) + 1 if sup[s + 1] - sup[s] > 1 else int(sup[s]) for s in SPC.leaves_of(sym)]
    extra = [r for r in extra if r not in have][-1:] or [r for r in range(c["n"]) if r not in have][:1]
    crow = int(SPC.caller_rows(c, extra)[0])
    lo, hi = int(c["bp"][0]), int(c["bp"][1])
    col0 = np.concatenate([c["bi"][lo:hi], [crow]])
    val0 = np.concatenate([c["bx"][lo:hi], [0.0]])
    order = np.argsort(col0)
    bi = np.concatenate([col0[order], c["bi"][hi:]]).astype(np.int32)
    bx = np.concatenate([val0[order], c["bx"][hi:]])
    bp = c["bp"].copy()
    bp[1:] += 1
    for op, xkind in (("A", "all"), ("GINV", "all"), ("A", "dozen")):
        h = _handle(api, c, SPC.xset_rows(sym, xkind), (bp, bi))
        assert set(h.reach()[0].tolist()) >= set(SPC.reaches(c, None)[0])
        X = h.solve(c["lv"], bx, op=op)[0]
        h.close()
        assert np.array_equal(X, _solve(api, c, op, xkind)), f"{op}/{xkind}: an entry of B that carries 0.0 changed the result"


@pytest.mark.parametrize("name", NAMES)
def test_drop_in_against_ginv_on_the_same_closed_list(api, name):
    c = _ctx(api, name)
    sym, n = c["sym"], c["n"]
    F = SR.closure(sym, c["seeds"][0] or [0])
    cols = SR.columns_of(sym, F)
    rng = np.random.default_rng(77)
    x = np.full(n, _SENTINEL)
    x[cols] = rng.standard_normal(cols.size)
    x0 = x.copy()
    bpset = np.array([s + 1 for s in reversed(F)], dtype=np.int32)      # (any order)
    assert api.blockedPrunedLSolve(n, sym.p, sym.s, c["lv"], int(sym.xsize), sym.i_ptr, bpset, bpset.size, sym.super,
                                   sym.nsuper, x) == 1
    outside = np.setdiff1d(np.arange(n), cols)
    assert np.array_equal(x[outside], x0[outside]), "x was written outside the columns of the listed supernodes"
    rows_c = SPC.caller_rows(c, cols)
    order = np.argsort(rows_c)
    h = api.SparseSolve(c["plan"], (np.array([0, cols.size], np.int32), rows_c[order]), rows_c)
    assert h.reach()[0].tolist() == F and h.reach()[1].tolist() == F
    X = h.solve(c["lv"], x0[cols][order], op="GINV")[0]
    h.close()
    assert np.array_equal(X[:, 0], x[cols]), "the drop-in and GINV on the same closed list differ"
    rho = SC.rho_solve(c["L"][np.ix_(cols, cols)], x[cols], x0[cols])
    print(f"{name}: drop-in rho = {rho.max():.2f} u on {cols.size} columns (limit {n + 1})")
    assert (rho <= n + 1).all()


@pytest.mark.parametrize("name", NAMES)
def test_device_call_path_and_bookkeeping(api, name):
    import torch
    c = _ctx(api, name)
    sym, nrhs = c["sym"], c["case"].nrhs
    dev = torch.device("cuda", 0)
    dL = torch.from_numpy(c["lv"]).to(dev)
    d_bx = torch.from_numpy(c["bx"]).to(dev)
    for op, xkind, pad in (("A", "dozen", 3), ("GINV", "leaf", 0), ("GINVT", "border", 1), ("A", "all", 0)):
        xrows = SPC.xset_rows(sym, xkind)
        F, K = SPC.reaches(c, xrows)
        h = _handle(api, c, xrows)
        nx = h.nx
        ldx = nx + pad
        before = h.info()
        assert before["device_bytes"] == 0 and before["last_op"] == -1
        bytes_seen = []
        for _ in range(2):
            d_x = torch.full((ldx * nrhs + 5,), _SENTINEL, dtype=torch.float64, device=dev)
            api.reset_kernel_launches()
            h.solve_device(dL.data_ptr(), d_bx.data_ptr(), d_x.data_ptr(), ldx, op=op)
            torch.cuda.synchronize()
            assert not any(api.kernel_launches().values()), "the plan's solve schedule ran"
            out = d_x.cpu().numpy()
            X = out[:ldx * nrhs].reshape(nrhs, ldx).T
            assert np.array_equal(X[:nx, :], _solve(api, c, op, xkind)), f"{op}/{xkind}: device call and host call differ"
            assert (X[nx:, :] == _SENTINEL).all() and (out[ldx * nrhs:] == _SENTINEL).all(), "written outside nx x nrhs"
            info = h.info()
            want = SR.kernels_of(sym, F, K, SR.OPS[op])
            assert info["last_op"] == SR.OPS[op] and info["last_kernels"] == want, (op, xkind, info["last_kernels"], want)
            bytes_seen.append(info["device_bytes"])
        assert bytes_seen[0] > 0 and bytes_seen[1] == bytes_seen[0], "device_bytes grew between the first and the second call"
        assert np.array_equal(dL.cpu().numpy(), c["lv"]) and np.array_equal(d_bx.cpu().numpy(), c["bx"]), "an input was written"
        h.close()
        _undisturbed(c)
