"""A x = b in the caller's ordering on the device (parsy_residual_device, parsy_solve_spd_device / _host): the
symmetric residual and its backward error against scipy, refinement with the exact factor and with a factor of older
values (LAPACK dporfs's loop), and the call's other forms and refusals.  Checked against scipy / numpy only."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import splu

from conftest import problem
from test_refine_host import EPS, berr_of, stale_values

pytestmark = pytest.mark.gpu

_SENTINEL = -7.25e300
_PAD = 37
_CASES = {}


def _case(api, name):
    """(A lower CSC, sym, plan on device 0, lValues of sym.A2x, A as scipy CSR with both triangles), per name."""
    if name not in _CASES:
        from parsy_bench_amd import inspector as I, matrices as M
        if name == "random":
            A = M.random_spd(300, density=0.03, seed=5)
            sym = I.analyze(A, None)
        else:
            A, _, sym = problem(name)
        plan = api.Plan(sym, 0)
        lv, _ = plan.factor(sym.A2x)
        assert plan.status() == 0
        _CASES[name] = (A, sym, plan, lv, A.to_scipy().tocsr())
    return _CASES[name]


def _shift(name):
    from parsy_bench_amd import matrices as M
    return M.WORKLOADS[name][4]


def _padded(M_, ld):
    """Column-major n x k with leading dimension ld, the rows n .. ld - 1 and a tail filled with the sentinel."""
    n, k = M_.shape
    buf = np.full(ld * k + 11, _SENTINEL)
    buf[:ld * k].reshape(k, ld)[:, :n] = M_.T
    return buf


def _unpad(buf, n, k, ld):
    return buf[:ld * k].reshape(k, ld)[:, :n].T.copy()


def _pad_intact(buf, n, k, ld):
    v = buf[:ld * k].reshape(k, ld)[:, n:]
    return (v.view(np.int64) == np.float64(_SENTINEL).view(np.int64)).all() and \
        (buf[ld * k:].view(np.int64) == np.float64(_SENTINEL).view(np.int64)).all()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _lu_solver(Afull_perm_csc):
    lu = splu(Afull_perm_csc, permc_spec="NATURAL")
    return lambda B: lu.solve(B)


def _reference_solve(Afull, sym, B):
    """A^-1 B through an LU of P A P' in the fill-reducing order (what spsolve computes, at a fraction of its cost)."""
    P = sym.Perm
    solve = _lu_solver(Afull[P][:, P].tocsc())
    X = np.empty_like(B)
    X[P] = solve(np.ascontiguousarray(B[P]))
    return X


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---- 1. residual against scipy ------------------------------------------------------------------------------
_RESID = [(nm, k) for nm in ("tiny2d", "ex15", "mid3d", "lap30", "random") for k in (1, 3, 8, 17, 64)] + \
         [("small3d", k) for k in (2, 4, 12)] + [("parabolic_fem", 1)]   # small3d: 16 lanes per row; 2, 4 and 9-16 columns


@pytest.mark.parametrize("name,nrhs", _RESID)
def test_residual_matches_scipy(api, name, nrhs):
    import torch
    A, sym, plan, lv, Afull = _case(api, name)
    n, ld = sym.n, sym.n + _PAD
    nz = int(np.diff(Afull.indptr).max()) + 1
    rng = np.random.default_rng(1000 + nrhs)
    X, B = rng.standard_normal((n, nrhs)), rng.standard_normal((n, nrhs))
    P = sym.Perm
    vals = _dev(sym.A2x)
    for perm in ("identity", "perm"):
        # identity: the plan's own system P A P'; perm: the caller's A with sym.Perm
        Aref = Afull[P][:, P].tocsr() if perm == "identity" else Afull
        plan.set_perm(None if perm == "identity" else P)
        Xd, Bd = _dev(_padded(X, ld)), _dev(_padded(B, ld))
        outs = []
        for _ in range(2):
            Rd = _dev(np.full(ld * nrhs + 11, _SENTINEL))
            berr = plan.residual_device(vals.data_ptr(), Xd.data_ptr(), ld, Bd.data_ptr(), ld, nrhs, Rd.data_ptr(), ld)
            torch.cuda.synchronize()
            outs.append((Rd.cpu().numpy(), berr))
        rbuf, berr = outs[0]
        assert _pad_intact(rbuf, n, nrhs, ld), "the padding of R was written"
        assert np.array_equal(rbuf.view(np.int64), outs[1][0].view(np.int64)), "a second call differs bitwise (R)"
        assert np.array_equal(berr.view(np.int64), outs[1][1].view(np.int64)), "a second call differs bitwise (berr)"
        R = _unpad(rbuf, n, nrhs, ld)
        den = abs(Aref) @ np.abs(X) + np.abs(B)
        assert (np.abs(R - (B - Aref @ X)) <= 4 * nz * EPS * den).all(), f"{perm}: R differs from B - A X"
        want = berr_of(Aref, X, B, R)
        assert np.allclose(berr, want, rtol=1e-12, atol=0), f"{perm}: berr {berr[:4]} vs {want[:4]}"
    plan.set_perm(None)


# ---- 2. exact factor ----------------------------------------------------------------------------------------
_EXACT = [(nm, k, 5) for nm in ("ex15", "mid3d", "lap30") for k in (1, 8, 64)] + \
         [("parabolic_fem", 1, 2), ("parabolic_fem", 64, 2)]


@pytest.mark.parametrize("name,nrhs,max_steps", _EXACT)
def test_exact_factor(api, name, nrhs, max_steps):
    import torch
    A, sym, plan, lv, Afull = _case(api, name)
    n = sym.n
    plan.set_perm(sym.Perm)
    B = np.random.default_rng(7 + nrhs).standard_normal((n, nrhs))
    vals, Ld, Bd = _dev(sym.A2x), _dev(lv), _dev(B.T)
    Xd = torch.zeros_like(Bd)
    steps0, berr0 = plan.solve_spd_device(vals.data_ptr(), Ld.data_ptr(), Bd.data_ptr(), n, Xd.data_ptr(), n, nrhs, 0)
    torch.cuda.synchronize()
    X0 = Xd.cpu().numpy().T
    Xs, _ = plan.solve_spd(lv, B)
    assert (steps0 == 0).all()
    assert _rel(X0, Xs) <= 1e-12, "max_steps = 0 differs from Plan.solve_spd"
    steps, berr = plan.solve_spd_device(vals.data_ptr(), Ld.data_ptr(), Bd.data_ptr(), n, Xd.data_ptr(), n, nrhs,
                                        max_steps)
    torch.cuda.synchronize()
    X = Xd.cpu().numpy().T
    assert (berr <= 1e-14).all(), f"berr {berr.max():.3e}"
    assert ((steps >= 0) & (steps <= max_steps)).all()
    assert _rel(X, _reference_solve(Afull, sym, B)) <= 1e-10
    plan.set_perm(None)


# ---- 3./4. a factor of other values -------------------------------------------------------------------------
def _stale(api, name, frac, nrhs, max_steps, seed=11):
    import torch
    A, sym, plan, lv, Afull = _case(api, name)
    n = sym.n
    plan.set_perm(sym.Perm)
    Ax, delta = stale_values(A, _shift(name), frac, seed)
    vals = _dev(sym.permute_values(Ax))
    # (right-hand sides whose every column meets dporfs's halving test from the first step on, as the test file's numpy
    # restatement shows for them: with other ones a column can stop after one step, on the device as in the restatement)
    B = np.random.default_rng(20 + nrhs).standard_normal((n, nrhs))
    Ld, Bd = _dev(lv), _dev(B.T)
    Xd = torch.zeros_like(Bd)
    steps, berr = plan.solve_spd_device(vals.data_ptr(), Ld.data_ptr(), Bd.data_ptr(), n, Xd.data_ptr(), n, nrhs,
                                        max_steps)
    torch.cuda.synchronize()
    plan.set_perm(None)
    return Xd.cpu().numpy().T, steps, berr, (Afull + sp.diags(delta)).tocsr(), B, sym


@pytest.mark.parametrize("name", ["ex15", "small3d", "mid3d", "lap30"])
@pytest.mark.parametrize("nrhs", [1, 8])
def test_stale_factor_converges(api, name, nrhs):
    _, steps0, berr0, _, _, _ = _stale(api, name, 0.1, nrhs, 0)
    assert (steps0 == 0).all() and (berr0 >= 1e-6).all(), f"a plain solve is already accurate: {berr0.min():.3e}"
    X, steps, berr, Anew, B, sym = _stale(api, name, 0.1, nrhs, 30)
    assert (berr <= 1e-14).all(), f"berr {berr.max():.3e} after {steps.tolist()} steps"
    assert (steps >= 3).all() and (steps <= 30).all(), steps.tolist()
    assert _rel(X, _reference_solve(Anew, sym, B)) <= 1e-10


@pytest.mark.parametrize("name", ["ex15", "lap30"])
def test_stale_factor_too_far_stops(api, name):
    X, steps, berr, Anew, B, sym = _stale(api, name, 0.9, 8, 30)
    assert (steps <= 2).all(), steps.tolist()
    assert (berr > 1e-6).all(), berr.tolist()
    assert np.isfinite(X).all()
    assert np.allclose(berr, berr_of(Anew, X, B), rtol=1e-10, atol=0), "berr is not the backward error of the returned x"


# ---- 5. other forms, reproducibility, refusals ---------------------------------------------------------------
def _agree(x, st, be, x_ref, st_ref, be_ref, what):
    """Two refined solves of one system: the plan's solve kernels sum with FP64 atomics, so x agrees to rounding (the
    residual and the refinement's own kernels are bitwise reproducible: test_residual_matches_scipy); every column
    converged either way and took the same number of steps, give or take the last one."""
    assert _rel(x, x_ref) <= 1e-13, f"{what}: x differs by {_rel(x, x_ref):.2e}"
    assert (be <= 1e-14).all() and (be_ref <= 1e-14).all(), f"{what}: berr {be.max():.2e}, {be_ref.max():.2e}"
    assert (np.abs(st.astype(int) - st_ref) <= 1).all(), f"{what}: steps {st.tolist()} vs {st_ref.tolist()}"


def test_in_place_host_path_and_repeat(api):
    import torch
    A, sym, plan, lv, Afull = _case(api, "mid3d")
    n, nrhs, ld = sym.n, 8, sym.n + _PAD
    Ax, delta = stale_values(A, _shift("mid3d"), 0.1, 11)
    v2 = sym.permute_values(Ax)
    B = np.random.default_rng(28).standard_normal((n, nrhs))
    plan.set_perm(sym.Perm)
    vals, Ld = _dev(v2), _dev(lv)
    runs = []
    for _ in range(2):
        Bd = _dev(_padded(B, ld))
        Xd = _dev(np.full(ld * nrhs + 11, _SENTINEL))
        st, be = plan.solve_spd_device(vals.data_ptr(), Ld.data_ptr(), Bd.data_ptr(), ld, Xd.data_ptr(), ld, nrhs, 30)
        torch.cuda.synchronize()
        xbuf = Xd.cpu().numpy()
        assert _pad_intact(xbuf, n, nrhs, ld), "the padding of X was written"
        assert np.array_equal(Bd.cpu().numpy().view(np.int64), _padded(B, ld).view(np.int64)), "B was written"
        runs.append((_unpad(xbuf, n, nrhs, ld), st, be))
    X, st, be = runs[0]
    assert (st >= 3).all()
    assert _rel(X, _reference_solve((Afull + sp.diags(delta)).tocsr(), sym, B)) <= 1e-10
    _agree(*runs[1], X, st, be, "a second call")
    # d_x == d_b
    Bd = _dev(_padded(B, ld))
    st2, be2 = plan.solve_spd_device(vals.data_ptr(), Ld.data_ptr(), Bd.data_ptr(), ld, Bd.data_ptr(), ld, nrhs, 30)
    torch.cuda.synchronize()
    xbuf = Bd.cpu().numpy()
    assert _pad_intact(xbuf, n, nrhs, ld)
    _agree(_unpad(xbuf, n, nrhs, ld), st2, be2, X, st, be, "d_x == d_b")
    # host convenience (sets sym.Perm on first use)
    plan.set_perm(None)
    plan._perm_set = False
    xh, info = plan.solve_refined(v2, lv, B, max_steps=30)
    _agree(xh, info["steps"], info["berr"], X, st, be, "solve_refined")
    assert info["seconds"] > 0
    x1, info1 = plan.solve_refined(v2, lv, B[:, 0], max_steps=30)
    assert x1.shape == (n,)
    _agree(x1[:, None], info1["steps"], info1["berr"], X[:, :1], st[:1], be[:1], "one right-hand side")
    plan.set_perm(None)


def test_refusals_leave_the_plan_usable(api):
    import torch
    from parsy_bench_amd import _native as N
    A, sym, plan, lv, Afull = _case(api, "ex15")
    n = sym.n
    vals, Ld = _dev(sym.A2x), _dev(lv)
    B = np.random.default_rng(9).standard_normal((n, 2))
    Bd = _dev(B.T)
    Xd = torch.zeros_like(Bd)
    v, L, b, x = vals.data_ptr(), Ld.data_ptr(), Bd.data_ptr(), Xd.data_ptr()
    with pytest.raises(RuntimeError, match="nrhs"):
        plan.solve_spd_device(v, L, b, n, x, n, 0)
    with pytest.raises(RuntimeError, match="leading dimension"):
        plan.solve_spd_device(v, L, b, n - 1, x, n, 2)
    with pytest.raises(RuntimeError, match="leading dimension"):
        plan.residual_device(v, x, n, b, n, 2, x, n - 1)
    with pytest.raises(RuntimeError, match="null argument"):
        plan.solve_spd_device(0, L, b, n, x, n, 2)
    with pytest.raises(RuntimeError, match="null argument"):
        plan.residual_device(v, 0, n, b, n, 2)
    with pytest.raises(RuntimeError, match="not a permutation"):
        plan.set_perm(np.zeros(n, dtype=np.int32))
    plan.set_active(np.ones(sym.nsuper, dtype=np.uint8))
    try:
        with pytest.raises(RuntimeError, match="set_active"):
            plan.solve_spd_device(v, L, b, n, x, n, 2)
        with pytest.raises(RuntimeError, match="set_active"):
            plan.residual_device(v, x, n, b, n, 2)
    finally:
        plan.set_active(None)
    Lscratch = _dev(np.zeros(int(sym.xsize)))
    plan.factor_begin(v, Lscratch.data_ptr())
    try:
        with pytest.raises(RuntimeError, match="factorization is still open"):
            plan.solve_spd_device(v, L, b, n, x, n, 2)
    finally:
        for lev in range(int(plan.info["chol_levels"])):
            plan.factor_level(lev, Lscratch.data_ptr())
        plan.factor_end()
    plan.solve_levels_device(L, x, 2, n, 0, 0, 1, True, False)
    with pytest.raises(RuntimeError, match="steps of levels"):
        plan.solve_spd_device(v, L, b, n, x, n, 2)
    plan.solve_levels_device(L, x, 2, n, 0, 1, int(plan.solve_levels().max()) + 1, False, True)
    torch.cuda.synchronize()
    # the plan still solves correctly
    plan.set_perm(sym.Perm)
    steps, berr = plan.solve_spd_device(v, L, b, n, x, n, 2, 5)
    torch.cuda.synchronize()
    assert (berr <= 1e-14).all()
    assert _rel(Xd.cpu().numpy().T, _reference_solve(Afull, sym, B)) <= 1e-10
    assert N.lib().parsy_solve_status(plan._h) == 0
    plan.set_perm(None)
