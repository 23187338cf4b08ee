"""A x = b in the caller's ordering (parsy_plan_set_perm, parsy_residual_device, parsy_solve_spd_*) on the CPU tier:
the argument checks a host-only plan can reach, and the test suite's own numpy restatement of LAPACK dporfs's loop (the
checker the GPU tests lean on), run with a scipy LU as the "factor"."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import splu

from conftest import problem

EPS = 2.0 ** -53
SAFMIN = np.finfo(np.float64).tiny


def full_matrix(A):
    return A.to_scipy().tocsr()


def berr_of(A, x, b, r=None):
    """dporfs's componentwise backward error of every column of x (A: scipy, both triangles)."""
    x, b = x.reshape(A.shape[0], -1), b.reshape(A.shape[0], -1)
    r = b - A @ x if r is None else r.reshape(x.shape)
    nz = int(np.diff(A.indptr).max()) + 1
    safe1 = nz * SAFMIN
    safe2 = safe1 / EPS
    den = abs(A) @ np.abs(x) + np.abs(b)
    ratio = np.where(den > safe2, np.abs(r) / np.where(den > safe2, den, 1.0), (np.abs(r) + safe1) / (den + safe1))
    return ratio.max(axis=0)


def dporfs(A, solve, b, max_steps):
    """dporfs's loop for one column: returns (x, steps, berr of the returned x)."""
    x = solve(b)
    lstres, count = 3.0, 0
    while True:
        r = b - A @ x
        berr = float(berr_of(A, x, b, r)[0])
        if berr > EPS and 2 * berr <= lstres and count < max_steps:
            x = x + solve(r)
            lstres = berr
            count += 1
            continue
        return x, count, berr


def stale_values(A, shift, frac, seed):
    """A + diag(delta), delta_i = frac * shift * U(0, 1) (fixed seed): the lower-CSC values of the new matrix."""
    delta = frac * shift * np.random.default_rng(seed).random(A.n)
    Ax = A.Ax.copy()
    for j in range(A.n):
        rows = A.Ai[A.Ap[j]:A.Ap[j + 1]]
        Ax[A.Ap[j] + int(np.nonzero(rows == j)[0][0])] += delta[j]
    return Ax, delta


@pytest.fixture(scope="module")
def host_plan():
    from parsy_bench_amd import api
    A, perm, sym = problem("ex15")
    return api.Plan(sym, -1), sym


def test_set_perm_accepts_permutations(host_plan):
    plan, sym = host_plan
    plan.set_perm(sym.Perm)
    plan.set_perm(None)
    plan.set_perm(np.arange(sym.n)[::-1])


@pytest.mark.parametrize("bad", ["duplicate", "negative", "too_large"])
def test_set_perm_rejects_non_permutations(host_plan, bad):
    plan, sym = host_plan
    p = sym.Perm.copy()
    if bad == "duplicate":
        p[1] = p[0]
    elif bad == "negative":
        p[3] = -1
    else:
        p[5] = sym.n
    with pytest.raises(RuntimeError, match="not a permutation"):
        plan.set_perm(p)
    with pytest.raises(ValueError):
        plan.set_perm(sym.Perm[:-1])


def test_host_only_plan_refuses_device_calls(host_plan):
    plan, sym = host_plan
    n = sym.n
    with pytest.raises(RuntimeError, match="without a device"):
        plan.residual_device(1, 1, n, 1, n, 1)
    with pytest.raises(RuntimeError, match="without a device"):
        plan.solve_spd_device(1, 1, 1, n, 1, n, 1)
    with pytest.raises(RuntimeError, match="without a device"):
        plan.solve_refined(sym.A2x, np.zeros(int(sym.xsize)), np.ones(n))


def test_numpy_dporfs_converges_with_a_stale_factor():
    """The restatement converges on ex15 when the factor is of A and the system is A + diag(0.1 shift U(0,1)); the
    halving test stops it after one step at 0.9 shift."""
    from parsy_bench_amd import matrices as M
    A, _, _ = problem("ex15")
    shift = M.WORKLOADS["ex15"][4]
    lu = splu(full_matrix(A).tocsc())
    Anew_vals, delta = stale_values(A, shift, 0.1, 11)
    Anew = full_matrix(A) + sp.diags(delta)
    b = np.random.default_rng(2).standard_normal(A.n)
    x, steps, berr = dporfs(Anew, lu.solve, b, 30)
    assert berr <= 1e-14 and steps >= 3
    xref = sp.linalg.spsolve(Anew.tocsc(), b)
    assert np.abs(x - xref).max() <= 1e-10 * np.abs(xref).max()
    _, steps0, berr0 = dporfs(Anew, lu.solve, b, 0)
    assert steps0 == 0 and berr0 >= 1e-6
    Afar = full_matrix(A) + sp.diags(stale_values(A, shift, 0.9, 11)[1])
    xf, stepsf, berrf = dporfs(Afar, lu.solve, b, 30)
    assert stepsf <= 2 and berrf > 1e-6 and np.isfinite(xf).all()
