"""Forward error bounds and the condition estimate on the device (parsy_rcond_*, parsy_error_bounds_device,
parsy_solve_spd_bounds_*): every estimate against the dense exact quantity under the conditions of test_cond_host
(exact / 3 <= est <= exact (1 + 1e-6); the true error <= ferr), on inputs small enough for numpy.linalg.inv.

The exact FERR is || |A^-1| w ||_inf / ||x||_inf with w formed in numpy from the x the device returned.  The |r| in w is
the residual as parsy_residual_device returns it for that x (the same kernel sums, bit for bit): at a refined x the
residual IS rounding noise, so a residual summed in another order would change w by per cent, not by 1e-6."""
import ctypes as C

import numpy as np
import pytest

from test_cond_host import ALL, check_estimate, cond_input, ferr_exact, weights
from test_refine_gpu import _SENTINEL, _agree, _case, _dev, _pad_intact, _padded, _reference_solve, _unpad
from test_refine_host import EPS

pytestmark = pytest.mark.gpu

_PAD = 29
_CASES = {}


def _cond_case(api, name):
    """Per input: (sym, plan on device 0, lValues of sym.A2x, A dense, A^-1 dense), both in the caller's ordering."""
    if name not in _CASES:
        from parsy_bench_amd import inspector as I
        A, perm = cond_input(name)
        sym = I.analyze(A, perm)
        plan = api.Plan(sym, 0)
        lv, _ = plan.factor(sym.A2x)
        assert plan.status() == 0, f"{name}: the factorization failed at column {plan.status()}"
        Ad = A.to_dense()
        _CASES[name] = (sym, plan, lv, Ad, np.linalg.inv(Ad))
    return _CASES[name]


def _nz(Ad):
    return int((Ad != 0).sum(axis=1).max()) + 1


# ---- 1. rcond ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_rcond(api, name):
    sym, plan, lv, Ad, Ainv = _cond_case(api, name)
    n = sym.n
    vals, Ld = _dev(sym.A2x), _dev(lv)
    anorm = np.abs(Ad).sum(axis=0).max()
    exact = np.abs(Ainv).sum(axis=0).max()
    bytes0 = plan.info["device_bytes"]
    rc, an = plan.rcond_device(vals.data_ptr(), Ld.data_ptr())
    info = plan.cond_info
    rc_h, an_h, sec = plan.rcond(sym.A2x, lv)
    print(f"{name}: n {n} anorm {an:.17g} (numpy {anorm:.17g}) 1/(anorm rcond) {1 / (an * rc):.17g} exact {exact:.17g} "
          f"ratio - 1 {1 / (an * rc) / exact - 1:.3e} applications {info['applications']}")
    assert abs(an - anorm) <= 4 * _nz(Ad) * EPS * anorm and an_h == an
    check_estimate(1.0 / (an * rc), exact, f"{name}: ||A^-1||_1 (device pointers)")
    check_estimate(1.0 / (an_h * rc_h), exact, f"{name}: ||A^-1||_1 (host arrays)")
    assert info["columns"] == 1 and 1 <= info["applications"] <= 11
    assert n > 1 or info["applications"] == 1, "n = 1 takes one application"
    assert info["device_bytes"] > 0 and plan.info["device_bytes"] >= bytes0
    assert sec > 0 and plan.solve_status() == 0
    # anorm alone: no solve
    from parsy_bench_amd import _native as N
    a1 = C.c_double(0)
    assert N.lib().parsy_rcond_device(plan._h, vals.data_ptr(), Ld.data_ptr(), C.byref(a1), None, None) == 0
    assert a1.value == an and plan.cond_info["applications"] == 0


# ---- 2. error bounds of a given X --------------------------------------------------------------------------------
def _columns(n, nrhs, seed):
    """x_t with the columns scaled 1, 1e6, 1e-6, ... (a mixing of columns shows) and, from 4 columns on, one zero column."""
    rng = np.random.default_rng(seed)
    Xt = rng.standard_normal((n, nrhs)) * (10.0 ** np.array([0, 6, -6]))[np.arange(nrhs) % 3]
    zero = nrhs - 2 if nrhs >= 4 else -1
    if zero >= 0:
        Xt[:, zero] = 0.0
    return Xt, zero, rng


# every lane split of the sweep (tiny2d 4, random300 8, small3d 16, dense150 32 lanes per row), and on dense150 every
# column count it is instantiated for (1 .. 4; staged: up to 8, 16, 32, 64)
_BOUNDS = [(nm, k) for nm in ("tiny2d", "small3d", "random300", "small3d*1e3") for k in (1, 4, 5, 17)] + \
          [("dense150", k) for k in (1, 2, 3, 4, 5, 12, 17, 64)]


@pytest.mark.parametrize("name,nrhs", _BOUNDS)
def test_error_bounds(api, name, nrhs):
    import torch
    sym, plan, lv, Ad, Ainv = _cond_case(api, name)
    n, ld, P = sym.n, sym.n + _PAD, sym.Perm
    vals, Ld = _dev(sym.A2x), _dev(lv)
    v, L = vals.data_ptr(), Ld.data_ptr()
    import scipy.sparse as sp
    try:
        for perm in ("identity", "perm"):
            # identity: the plan's own system P A P'; perm: the caller's A with sym.Perm
            Aref, Aref_inv = (Ad[P][:, P], Ainv[P][:, P]) if perm == "identity" else (Ad, Ainv)
            As = sp.csr_matrix(Aref)
            plan.set_perm(None if perm == "identity" else P)
            Xt, zero, rng = _columns(n, nrhs, 100 + nrhs)
            B = Aref @ Xt
            real = np.arange(nrhs) != zero
            Bd = _dev(_padded(B, ld))
            Xd = _dev(np.full(ld * nrhs + 11, _SENTINEL))
            plan.solve_spd_device(v, L, Bd.data_ptr(), ld, Xd.data_ptr(), ld, nrhs, 5)
            torch.cuda.synchronize()
            X = _unpad(Xd.cpu().numpy(), n, nrhs, ld)
            for pss in ("refined", "perturbed"):
                if pss == "perturbed":
                    X = X * (1.0 + 1e-6 * rng.standard_normal(X.shape))
                    Xd = _dev(_padded(X, ld))
                ferr, berr = plan.error_bounds_device(v, L, Xd.data_ptr(), ld, Bd.data_ptr(), ld, nrhs)
                info = plan.cond_info
                Rd = _dev(np.full(ld * nrhs + 11, _SENTINEL))
                berr_r = plan.residual_device(v, Xd.data_ptr(), ld, Bd.data_ptr(), ld, nrhs, Rd.data_ptr(), ld)
                torch.cuda.synchronize()
                what = f"{name} nrhs {nrhs} {perm} {pss}"
                assert _pad_intact(Xd.cpu().numpy(), n, nrhs, ld) and _pad_intact(Bd.cpu().numpy(), n, nrhs, ld), what
                assert np.array_equal(_unpad(Xd.cpu().numpy(), n, nrhs, ld), X), f"{what}: X was written"
                R = _unpad(Rd.cpu().numpy(), n, nrhs, ld)
                exact = ferr_exact(Aref_inv, weights(As, X, B, R), X)
                err = np.abs(X - Xt).max(axis=0) / np.where(real, np.abs(X).max(axis=0), 1.0)
                print(f"{what}: applications {info['applications']} ferr/exact - 1 "
                      f"{np.abs(ferr[real] / exact[real] - 1).max():.3e} error/ferr {(err[real] / ferr[real]).max():.3e}")
                assert np.allclose(berr, berr_r, rtol=1e-12, atol=0), f"{what}: berr {berr} vs {berr_r}"
                assert info["columns"] == nrhs and 1 <= info["applications"] <= 11, f"{what}: {info}"
                assert np.isfinite(ferr).all() and (ferr >= 0).all(), f"{what}: ferr {ferr}"
                for q in np.nonzero(real)[0]:
                    check_estimate(ferr[q], exact[q], f"{what}: ferr of column {q}")
                    assert err[q] <= ferr[q], f"{what}: column {q}: the error {err[q]:.3e} is above ferr {ferr[q]:.3e}"
                if pss == "perturbed":
                    assert (ferr[real] >= 1e-7).all(), f"{what}: ferr {ferr} does not see an error of 1e-6"
    finally:
        plan.set_perm(None)


# ---- 3. the refined solve with bounds ------------------------------------------------------------------------------
def test_solve_refined_with_bounds(api):
    import torch
    A, sym, plan, lv, Afull = _case(api, "ex15")
    n, nrhs, ld = sym.n, 3, sym.n + _PAD
    B = np.random.default_rng(31).standard_normal((n, nrhs))
    Xref = _reference_solve(Afull, sym, B)
    plan.set_perm(None)
    plan._perm_set = False
    try:
        x0, i0 = plan.solve_refined(sym.A2x, lv, B)
        x1, i1 = plan.solve_refined(sym.A2x, lv, B, bounds=True)
        assert "ferr" not in i0 and set(i1) == set(i0) | {"ferr"}
        _agree(x1, i1["steps"], i1["berr"], x0, i0["steps"], i0["berr"], "bounds=True")
        err = np.abs(x1 - Xref).max(axis=0) / np.abs(x1).max(axis=0)
        print(f"host arrays: ferr {i1['ferr']} error against the LU reference {err}")
        assert np.isfinite(i1["ferr"]).all() and (err <= i1["ferr"]).all(), f"error {err} above ferr {i1['ferr']}"
        assert 1 <= plan.cond_info["applications"] <= 11 and plan.cond_info["columns"] == nrhs
        # device pointers, in place
        vals, Ld, Bd = _dev(sym.A2x), _dev(lv), _dev(_padded(B, ld))
        st, be, fe = plan.solve_spd_bounds_device(vals.data_ptr(), Ld.data_ptr(), Bd.data_ptr(), ld, Bd.data_ptr(), ld, nrhs, 5)
        torch.cuda.synchronize()
        xbuf = Bd.cpu().numpy()
        assert _pad_intact(xbuf, n, nrhs, ld)
        x2 = _unpad(xbuf, n, nrhs, ld)
        _agree(x2, st, be, x0, i0["steps"], i0["berr"], "d_x == d_b")
        err2 = np.abs(x2 - Xref).max(axis=0) / np.abs(x2).max(axis=0)
        print(f"in place: ferr {fe} error against the LU reference {err2}")
        assert np.isfinite(fe).all() and (err2 <= fe).all(), f"error {err2} above ferr {fe}"
        assert ((fe <= 2 * i1["ferr"]) & (i1["ferr"] <= 2 * fe)).all(), f"ferr {fe} vs {i1['ferr']}"
    finally:
        plan.set_perm(None)
        plan._perm_set = False


# ---- 4. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched(api):
    import torch
    from parsy_bench_amd import _native as N
    sym, plan, lv, Ad, Ainv = _cond_case(api, "tiny2d")
    n, lib, h = sym.n, N.lib(), plan._h
    vals, Ld = _dev(sym.A2x), _dev(lv)
    B = np.random.default_rng(9).standard_normal((n, 2))
    Bd = _dev(B.T)
    Xd = torch.full_like(Bd, _SENTINEL)
    v, L, b, x = vals.data_ptr(), Ld.data_ptr(), Bd.data_ptr(), Xd.data_ptr()
    out = {k: np.full(2, _SENTINEL) for k in ("ferr", "berr", "anorm", "rcond")}
    steps = np.full(2, -77, dtype=np.int32)
    fe, be, an, rc = (N.ptr(out[k]) for k in ("ferr", "berr", "anorm", "rcond"))

    def bounds(nrhs=2, ldx=n, f=fe, bb=be):
        return lib.parsy_error_bounds_device(h, v, L, x, ldx, b, n, nrhs, f, bb, None)

    def solve(nrhs=2, ldx=n):
        return lib.parsy_solve_spd_bounds_device(h, v, L, b, n, x, ldx, nrhs, 5, N.ptr(steps), be, fe, None)

    def refused(rc_, match):
        assert rc_ != 0 and match in N.last_error(), (rc_, N.last_error())
        assert all((a.view(np.int64) == np.float64(_SENTINEL).view(np.int64)).all() for a in out.values())
        assert (steps == -77).all()
        assert (Xd.cpu().numpy().view(np.int64) == np.float64(_SENTINEL).view(np.int64)).all(), "X was written"

    refused(bounds(f=None, bb=None), "both")
    refused(lib.parsy_rcond_device(h, v, L, None, None, None), "both")
    refused(bounds(nrhs=0), "nrhs")
    refused(solve(nrhs=0), "nrhs")
    refused(bounds(nrhs=65536), "nrhs")
    refused(bounds(ldx=n - 1), "leading dimension")
    refused(solve(ldx=n - 1), "leading dimension")
    refused(lib.parsy_error_bounds_device(h, None, L, x, n, b, n, 2, fe, be, None), "null argument")
    refused(lib.parsy_rcond_device(h, v, None, an, rc, None), "null argument")
    plan.set_active(np.ones(sym.nsuper, dtype=np.uint8))
    try:
        refused(bounds(), "set_active")
        refused(solve(), "set_active")
        refused(lib.parsy_rcond_device(h, v, L, an, rc, None), "set_active")
        refused(lib.parsy_rcond_host(h, N.ptr(sym.A2x), N.ptr(lv), an, rc, None), "set_active")
    finally:
        plan.set_active(None)
    # the plan still answers
    assert solve() == 0, N.last_error()
    torch.cuda.synchronize()
    assert (out["berr"] <= 1e-14).all() and np.isfinite(out["ferr"]).all() and (steps >= 0).all()
    X = Xd.cpu().numpy().T
    Xtrue = Ainv[sym.Perm][:, sym.Perm] @ B   # (identity ordering: the plan's own system)
    assert (np.abs(X - Xtrue).max(axis=0) / np.abs(X).max(axis=0) <= np.maximum(out["ferr"], 1e-13)).all()
