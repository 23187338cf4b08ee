"""The PyTorch layer (parsy_bench_amd.autograd.SpdSolver): gradients of solve and logdet with respect to the values and
the right-hand side against dense CPU torch autograd of the same loss, against the analytic formula with scipy solves on
the larger inputs, the forward values, the factor cache and the refusal of a matrix that is not positive definite."""
import numpy as np
import pytest

from conftest import problem
from test_selinv_host import edge

pytestmark = pytest.mark.gpu

# The two CPU restatements of these gradients (dense autograd, the analytic formula) agree to 5e-15 relative on these
# inputs, and the matrices are well conditioned (a 0.1 / 0.01 shift or diagonal dominance): an error above 1e-10 of the
# largest gradient entry is an indexing or weighting bug, not rounding.
TOL = 1e-10
_SOLVERS = {}


def _solver(api, name):
    """(A lower CSC, SpdSolver) per name, cached."""
    if name not in _SOLVERS:
        from parsy_bench_amd import inspector as I, matrices as M
        from parsy_bench_amd.autograd import SpdSolver
        if name == "random":
            A = M.random_spd(300, density=0.03, seed=5)
            arg = I.analyze(A, None)
        elif name in ("dense150", "tridiag300", "diag37"):
            A, arg = edge(name)
        elif name == "tiny2d":
            A = problem(name)[0]
            arg = A                      # the solver analyses a LowerCSC itself
        else:
            A, _, arg = problem(name)
        _SOLVERS[name] = (A, SpdSolver(arg, 0))
    return _SOLVERS[name]


def _coords(A):
    return np.asarray(A.Ai, dtype=np.int64), np.repeat(np.arange(A.n, dtype=np.int64), np.diff(A.Ap))


def _inputs(A, shape_k, seed):
    rng = np.random.default_rng(seed)
    shape = (A.n,) if shape_k == 0 else (A.n, shape_k)
    return rng.standard_normal(shape), rng.standard_normal(shape)


def _device_grads(solver, A, b, W, with_logdet, max_steps=0):
    import torch
    values = torch.tensor(np.asarray(A.Ax, dtype=np.float64), device="cuda", requires_grad=True)
    bt = torch.tensor(b, device="cuda", requires_grad=True)
    Wt = torch.tensor(W, device="cuda")
    loss = (Wt * solver.solve(values, bt, max_steps=max_steps)).sum()
    if with_logdet:
        loss = loss + 0.37 * solver.logdet(values)
    loss.backward()
    return float(loss.detach()), values.grad.cpu().numpy(), bt.grad.cpu().numpy()


@pytest.mark.parametrize("shape_k", [0, 5])
@pytest.mark.parametrize("name", ["tiny2d", "small3d", "random", "dense150", "tridiag300", "diag37"])
def test_gradients_against_dense_autograd(api, name, shape_k):
    import torch
    A, solver = _solver(api, name)
    b, W = _inputs(A, shape_k, 21)
    loss, gv, gb = _device_grads(solver, A, b, W, True)
    rows, cols = _coords(A)
    vals = torch.tensor(np.asarray(A.Ax, dtype=np.float64), requires_grad=True)
    bt = torch.tensor(b, requires_grad=True)
    D = torch.zeros((A.n, A.n), dtype=torch.float64).index_put((torch.from_numpy(rows), torch.from_numpy(cols)), vals)
    Af = D + D.T - torch.diag(torch.diag(D))
    ref = (torch.tensor(W) * torch.linalg.solve(Af, bt)).sum() + 0.37 * torch.logdet(Af)
    ref.backward()
    rv, rb = vals.grad.numpy(), bt.grad.numpy()
    assert gv.shape == rv.shape and gb.shape == rb.shape
    assert np.abs(gv - rv).max() <= TOL * np.abs(rv).max(), (name, float(np.abs(gv - rv).max()), float(np.abs(rv).max()))
    assert np.abs(gb - rb).max() <= TOL * np.abs(rb).max()
    assert abs(loss - float(ref)) <= TOL * max(1.0, abs(float(ref)))


@pytest.mark.parametrize("shape_k", [0, 5])
@pytest.mark.parametrize("name", ["ex15", "mid3d"])
def test_solve_gradients_against_the_formula(api, name, shape_k):
    from scipy.sparse.linalg import splu
    A, solver = _solver(api, name)
    b, W = _inputs(A, shape_k, 22)
    _, gv, gb = _device_grads(solver, A, b, W, False)
    lu = splu(A.to_scipy().tocsc())
    x, lam = lu.solve(b).reshape(A.n, -1), lu.solve(W).reshape(A.n, -1)
    rows, cols = _coords(A)
    rv = -((lam[rows] * x[cols]).sum(axis=1) + np.where(rows != cols, (lam[cols] * x[rows]).sum(axis=1), 0.0))
    assert np.abs(gv - rv).max() <= TOL * np.abs(rv).max()
    assert np.abs(gb.reshape(A.n, -1) - lam).max() <= TOL * np.abs(lam).max()


@pytest.mark.parametrize("name", ["small3d", "random"])
def test_forward_values(api, name):
    import torch
    A, solver = _solver(api, name)
    sym, plan = solver.sym, solver.plan
    b, _ = _inputs(A, 3, 23)
    values = torch.tensor(np.asarray(A.Ax, dtype=np.float64), device="cuda")
    x = solver.solve(values, torch.tensor(b, device="cuda"), max_steps=2)
    x1 = solver.solve(values, torch.tensor(b[:, 0].copy(), device="cuda"), max_steps=2)
    ld = solver.logdet(values)
    assert x.shape == b.shape and x1.shape == (A.n,) and ld.dim() == 0
    a2 = sym.permute_values(np.asarray(A.Ax, dtype=np.float64))
    lv, _ = plan.factor(a2)
    xr, _ = plan.solve_refined(a2, lv, b, max_steps=2)
    # The solve kernels sum with FP64 atomics, so two solves of one system agree to rounding only
    # and bitwise equality cannot be asked.  What both must meet after refinement is a bound known beforehand: the
    # refinement stops once the componentwise backward error is at 2^-53 or no longer halves, and its limiting accuracy
    # in working precision is the rounding of the residual itself, gamma = (nz + 1) 2^-53 (nz = the longest row of A);
    # numpy's residual adds as much again.  So each of x (this layer) and xr (Plan.solve_refined) must have
    #     |b - A v| <= 2 (nz + 2) 2^-53 (|A||v| + |b|)   componentwise,
    # a test that a wrong or wrongly ordered v fails by many orders of magnitude; and then, since
    # x - xr = A^-1 (r_xr - r_x), |x - xr| <= |A^-1| times the sum of those two bounds.
    Ad = A.to_dense()
    Ainv = np.abs(np.linalg.inv(Ad))
    nz = int((Ad != 0).sum(axis=1).max())
    c = 2 * (nz + 2) * 2.0 ** -53

    def residual_bound(v, rhs):
        scale = np.abs(Ad) @ np.abs(v) + np.abs(rhs)
        ratio = np.abs(rhs - Ad @ v) / scale
        print(name, "backward error", float(ratio.max()), "allowed", c)
        assert (ratio <= c).all(), (float(ratio.max()), c)
        return c * scale

    def check_close(got, ref, rhs):
        bound = Ainv @ (residual_bound(got, rhs) + residual_bound(ref, rhs))
        assert (np.abs(got - ref) <= bound).all(), float((np.abs(got - ref) - bound).max())

    check_close(x.cpu().numpy(), xr, b)
    check_close(x1.cpu().numpy(), xr[:, 0], b[:, 0])
    ldr, col = plan.logdet_device(torch.from_numpy(lv).cuda().data_ptr())
    assert col == 0 and float(ld) == ldr
    assert np.abs(A.to_scipy() @ xr - b).max() <= 1e-10 * np.abs(b).max()


def test_one_factorization_per_version(api):
    import torch
    A, solver = _solver(api, "small3d")
    b, W = _inputs(A, 0, 24)
    values = torch.tensor(np.asarray(A.Ax, dtype=np.float64), device="cuda", requires_grad=True)
    bt = torch.tensor(b, device="cuda")
    count = solver.factor_count
    x = solver.solve(values, bt)
    ld = solver.logdet(values)
    solver.solve(values, bt)
    assert solver.factor_count == count + 1
    (x.sum() + ld).backward()                      # the backward passes factor nothing
    assert solver.factor_count == count + 1
    diag0 = int(A.Ap[0])                           # column 0's first entry is its diagonal
    with torch.no_grad():
        values[diag0] += 0.5                       # an in-place change bumps the version: the factor is stale
    x2 = solver.solve(values, bt)
    assert solver.factor_count == count + 2
    Ax = np.asarray(A.Ax, dtype=np.float64).copy()
    Ax[diag0] += 0.5
    from parsy_bench_amd import matrices as M
    A2 = M.LowerCSC(A.n, A.Ap, A.Ai, Ax)
    assert np.abs(A2.to_scipy() @ x2.detach().cpu().numpy() - b).max() <= 1e-10 * np.abs(b).max()
    other = values.detach().clone()                # another tensor with equal contents: its own factorization
    solver.logdet(other)
    assert solver.factor_count == count + 3


def test_not_positive_definite_raises(api):
    import torch
    A, solver = _solver(api, "tiny2d")
    Ax = np.asarray(A.Ax, dtype=np.float64).copy()
    Ax[int(A.Ap[A.n // 2])] *= -1.0
    values = torch.tensor(Ax, device="cuda", requires_grad=True)
    with pytest.raises(RuntimeError, match="not positive definite.*pivot at column [0-9]+"):
        solver.solve(values, torch.zeros(A.n, dtype=torch.float64, device="cuda"))
    with pytest.raises(RuntimeError, match="not positive definite"):
        solver.logdet(values)
    good = torch.tensor(np.asarray(A.Ax, dtype=np.float64), device="cuda")
    assert torch.isfinite(solver.logdet(good))
    with pytest.raises(ValueError):
        solver.solve(good[:-1], torch.zeros(A.n, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        solver.solve(good, torch.zeros(A.n + 1, dtype=torch.float64, device="cuda"))
