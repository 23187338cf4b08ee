"""Forward error bounds and the condition estimate (parsy_error_bounds_device, parsy_solve_spd_bounds_*, parsy_rcond_*)
on the CPU tier: the test suite's own numpy restatement of LAPACK dlacn2 / dporfs's FERR / dpocon (the checker the GPU
tests lean on) against dense exact values and against LAPACK, the structure's size, and what a host-only plan answers.

Acceptance conditions (every estimate, here and on the GPU): exact / 3 <= est <= exact (1 + 1e-6) -- the lower factor is
Higham's accepted bound for this estimator, the upper margin covers the rounding of the solves -- and the true error
||x - x_t||_inf / ||x||_inf <= ferr."""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sla

from conftest import problem
from test_refine_host import EPS, SAFMIN, dporfs, full_matrix
from test_selinv_host import edge

UPPER = 1 + 1e-6


# ---- inputs: all small enough for a dense inverse ---------------------------------------------------------------
def scaled(A, k):
    """A's values times d_i d_j, d = 10**U(-k, k) (default_rng(7)): the same matrix badly scaled."""
    from parsy_bench_amd import matrices as M
    d = 10.0 ** np.random.default_rng(7).uniform(-k, k, A.n)
    cols = np.repeat(np.arange(A.n), np.diff(A.Ap))
    return M.LowerCSC(A.n, A.Ap.copy(), A.Ai.copy(), A.Ax * d[A.Ai] * d[cols])


_INPUTS = {}
UNSCALED = ["tiny2d", "small3d", "random300", "grid1e-8", "dense150", "n1", "n2", "n3"]
SCALED = [f"{nm}*1e{k}" for nm in ("tiny2d", "small3d", "random300") for k in (2, 3)]
ALL = UNSCALED + SCALED


def cond_input(name):
    """(A lower CSC, perm or None) of a named input of these tests, cached."""
    from parsy_bench_amd import matrices as M
    if name in _INPUTS:
        return _INPUTS[name]
    if "*" in name:
        base, _, k = name.partition("*1e")
        A, perm = cond_input(base)
        out = (scaled(A, int(k)), perm)
    elif name in ("tiny2d", "small3d"):
        A, perm, _ = problem(name)
        out = (A, perm)
    elif name == "random300":
        out = (M.random_spd(300, density=0.03, seed=5), None)
    elif name == "dense150":   # (a dense row: 32 lanes per row in the sweeps)
        A = edge(name)[0]
        out = (A, np.arange(A.n, dtype=np.int32))
    elif name == "grid1e-8":
        out = (M.grid_spd(24, 24, 1, 5, 1e-8), M.grid_nd(24, 24, 1))
    else:
        out = (M.grid_spd(int(name[1:]), 1, 1), None)
    _INPUTS[name] = out
    return out


# ---- the restatement ------------------------------------------------------------------------------------------------
def lacn2(n, apply, apply_t):
    """LAPACK dlacn2's estimate of ||M||_1 given x -> M x and x -> M' x; returns (est, applications)."""
    x = np.full(n, 1.0 / n)
    x = apply(x)
    apps = 1
    if n == 1:
        return abs(x[0]), apps
    est = np.abs(x).sum()
    sgn = np.where(x >= 0, 1.0, -1.0)
    x = apply_t(sgn.copy())
    apps += 1
    j = int(np.argmax(np.abs(x)))   # (the first index of the maximum, as idamax)
    it = 2
    while True:
        e = np.zeros(n)
        e[j] = 1.0
        x = apply(e)
        apps += 1
        estold, est = est, np.abs(x).sum()
        s = np.where(x >= 0, 1.0, -1.0)
        if (s == sgn).all() or est <= estold:
            break
        sgn = s
        x = apply_t(sgn.copy())
        apps += 1
        jlast, j = j, int(np.argmax(np.abs(x)))
        if abs(x[jlast]) != abs(x[j]) and it < 5:
            it += 1
            continue
        break
    i = np.arange(n)
    x = apply(np.where(i % 2 == 0, 1.0, -1.0) * (1.0 + i / (n - 1)))
    apps += 1
    return max(est, 2.0 * np.abs(x).sum() / (3.0 * n)), apps


def weights(A, x, b, r=None):
    """dporfs's w = |r| + nz eps (|A||x| + |b|) (+ safe1 where the sum is <= safe2) of every column (A: scipy, both
    triangles).  r: the residual to take (default: b - A x in numpy)."""
    x, b = x.reshape(A.shape[0], -1), b.reshape(A.shape[0], -1)
    r = b - A @ x if r is None else r.reshape(x.shape)
    nz = int(np.diff(A.tocsr().indptr).max()) + 1
    safe1 = nz * SAFMIN
    safe2 = safe1 / EPS
    s = abs(A) @ np.abs(x) + np.abs(b)
    return np.abs(r) + nz * EPS * s + np.where(s > safe2, 0.0, safe1)


def ferr_restated(solve, w, x):
    """dporfs's FERR of one column: dlacn2 on W A^-1 (transposed: A^-1 W), over ||x||_inf when that is not 0."""
    est, apps = lacn2(len(w), lambda v: w * solve(v), lambda v: solve(w * v))
    top = np.abs(x).max()
    return (est / top if top != 0 else est), apps


def rcond_restated(solve, anorm, n):
    est, apps = lacn2(n, solve, solve)
    return (0.0 if est == 0 else 1.0 / (anorm * est)), apps


def ferr_exact(Ainv, w, x):
    """|| |A^-1| w ||_inf / ||x||_inf per column."""
    top = np.abs(x).max(axis=0)
    return (np.abs(Ainv) @ w).max(axis=0) / np.where(top != 0, top, 1.0)


def check_estimate(est, exact, what):
    assert exact / 3 <= est <= exact * UPPER, f"{what}: estimate {est:.17g}, exact {exact:.17g} (ratio {est / exact:.12f})"


def two_solvers(Ad):
    """Two differently rounded solvers of the dense SPD Ad: Cholesky, and an LU of a symmetric permutation of it."""
    n = Ad.shape[0]
    c = sla.cho_factor(Ad, lower=True)
    p = np.random.default_rng(3).permutation(n)
    lu = sla.lu_factor(Ad[p][:, p])

    def lu_solve(v):
        out = np.empty_like(v)
        out[p] = sla.lu_solve(lu, v[p])
        return out
    return {"cholesky": lambda v: sla.cho_solve(c, v), "lu": lu_solve}


@pytest.mark.parametrize("name", ALL)
def test_restatement_against_dense(name):
    A, _ = cond_input(name)
    As = full_matrix(A)
    Ad = As.toarray()
    n = A.n
    Ainv = np.linalg.inv(Ad)
    anorm = np.abs(Ad).sum(axis=0).max()
    exact = np.abs(Ainv).sum(axis=0).max()
    xt = np.random.default_rng(17).standard_normal(n)
    b = Ad @ xt
    for nm, solve in two_solvers(Ad).items():
        rc, apps = rcond_restated(solve, anorm, n)
        assert apps <= 11 and (n > 1 or apps == 1)
        check_estimate(1.0 / (anorm * rc), exact, f"{name} / {nm}: ||A^-1||_1")
        x, _, _ = dporfs(As, solve, b, 5)
        w = weights(As, x, b)[:, 0]
        fe, apps = ferr_restated(solve, w, x)
        assert apps <= 11
        check_estimate(fe, ferr_exact(Ainv, w[:, None], x[:, None])[0], f"{name} / {nm}: ferr")
        err = np.abs(x - xt).max() / np.abs(x).max()
        assert err <= fe, f"{name} / {nm}: the error {err:.3e} is above ferr {fe:.3e}"


@pytest.mark.parametrize("name", UNSCALED)
def test_restatement_against_dpocon(name):
    A, _ = cond_input(name)
    Ad = full_matrix(A).toarray()
    anorm = np.abs(Ad).sum(axis=0).max()
    c, info = sla.lapack.dpotrf(Ad, lower=0)
    assert info == 0
    want, info = sla.lapack.dpocon(c, anorm, uplo="U")
    assert info == 0
    got, _ = rcond_restated(lambda v: sla.cho_solve((c, False), v), anorm, A.n)
    assert abs(got - want) <= 1e-8 * want, f"{name}: rcond {got:.17g}, dpocon {want:.17g}"


# ---- the library on the CPU tier --------------------------------------------------------------------------------------
def test_cond_info_size():
    from parsy_bench_amd import _native as N
    assert ctypes.sizeof(N.CondInfo) == 16


def test_host_only_plan_refuses_and_reports_zeros():
    from parsy_bench_amd import api
    A, perm, sym = problem("tiny2d")
    plan = api.Plan(sym, -1)
    n = sym.n
    assert plan.cond_info == {"applications": 0, "columns": 0, "device_bytes": 0}
    lv = np.zeros(int(sym.xsize))
    with pytest.raises(RuntimeError, match="without a device"):
        plan.error_bounds_device(1, 1, 1, n, 1, n, 1)
    with pytest.raises(RuntimeError, match="without a device"):
        plan.solve_spd_bounds_device(1, 1, 1, n, 1, n, 1)
    with pytest.raises(RuntimeError, match="without a device"):
        plan.rcond_device(1, 1)
    with pytest.raises(RuntimeError, match="without a device"):
        plan.rcond(sym.A2x, lv)
    with pytest.raises(RuntimeError, match="without a device"):
        plan.solve_refined(sym.A2x, lv, np.ones(n), bounds=True)
    assert plan.cond_info == {"applications": 0, "columns": 0, "device_bytes": 0}


@pytest.mark.parametrize("name", ["n1", "n2", "n3"])
def test_smallest_inputs_make_a_host_plan(name):
    from parsy_bench_amd import api, inspector as I
    A, perm = cond_input(name)
    sym = I.analyze(A, perm)
    plan = api.Plan(sym, -1)
    assert plan.info["n"] == A.n and plan.check() == 0
