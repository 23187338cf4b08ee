"""Gradients with respect to A's values on the device: the product sampled on A's pattern (parsy_pattern_outer_device,
both kernels), the entries of Z gathered to A's pattern (parsy_inverse_pattern_device) and tr(A^-1 B)
(parsy_trace_inverse_device), against numpy; bitwise reproducibility; the refusals."""
import numpy as np
import pytest

from conftest import problem
from test_selinv_gpu import DENSE, TOL, _case, _dev, _permuted_dense
from test_selinv_host import edge

pytestmark = pytest.mark.gpu

_SENTINEL = -7.25e300
_U = 2.0 ** -53
_PLANS = {}
NRHS = [1, 2, 4, 5, 8, 9, 17, 33, 64, 70]
LANES = {1: 1, 2: 1, 4: 1, 5: 8, 8: 8, 9: 16, 17: 32, 33: 64, 64: 64, 70: 64}


def _plan(api, name):
    """(sym, plan on device 0, its pattern) per name; no factorization."""
    if name not in _PLANS:
        from parsy_bench_amd import inspector as I, matrices as M
        if name == "random":
            sym = I.analyze(M.random_spd(300, density=0.03, seed=5), None)
        elif name in ("dense150", "tridiag300", "diag37"):
            sym = edge(name)[1]
        else:
            sym = problem(name)[2]
        plan = api.Plan(sym, 0)
        _PLANS[name] = (sym, plan, plan.pattern())
    return _PLANS[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _is_sentinel(a):
    return (_bits(a) == np.float64(_SENTINEL).view(np.int64)).all()


def _padded(rng, n, nrhs, ld):
    """n x nrhs column-major with leading dimension ld, the padding rows holding the sentinel: (flat, view of the rows)."""
    flat = np.full(ld * nrhs, _SENTINEL)
    V = flat.reshape(nrhs, ld)
    V[:, :n] = rng.standard_normal((nrhs, n))
    return flat, V[:, :n].T


def _reference(pat, perm, Lam, X):
    """(S, M): the sampled product and the sum of the absolute values of the products it adds up, per entry."""
    i, j = pat["row"], pat["col"]
    pi, pj = (i, j) if perm is None else (perm[i], perm[j])
    off = (i != j)[:, None]
    t1, t2 = Lam[pi] * X[pj], np.where(off, Lam[pj] * X[pi], 0.0)
    return (t1 + t2).sum(axis=1), (np.abs(t1) + np.abs(t2)).sum(axis=1)


def _outer(plan, dl, ld, dx, nrhs, g, alpha=1.0, beta=0.0):
    import torch
    plan.pattern_outer_device(dl.data_ptr(), ld, dx.data_ptr(), ld, nrhs, g.data_ptr(), alpha=alpha, beta=beta)
    torch.cuda.synchronize()
    return g.cpu().numpy()


def _check_outer(plan, sym, pat, perm, nrhs, rng, lanes):
    """One shape through every check of the sampled product.  The bound: the device adds 2 nrhs products in a fixed
    order (an fma chain, or fma chains per lane and a butterfly): at most 2 nrhs roundings of partial sums that never
    exceed M = sum |products|; numpy's reference has as many.  Hence |got - ref| <= 4 nrhs 2^-53 M."""
    import torch
    n, nnz = sym.n, int(sym.nnzA)
    ld = n + 37
    lf, Lam = _padded(rng, n, nrhs, ld)
    xf, X = _padded(rng, n, nrhs, ld)
    S, M = _reference(pat, perm, Lam, X)
    bound = 4 * nrhs * _U * M
    dl, dx = _dev(lf), _dev(xf)
    g = torch.full((nnz + 11,), _SENTINEL, dtype=torch.float64, device="cuda")
    got = _outer(plan, dl, ld, dx, nrhs, g)
    assert plan.grad_info["last_lanes"] == lanes, (nrhs, plan.grad_info)
    err = np.abs(got[:nnz] - S)
    assert (err <= bound).all(), (nrhs, float((err - bound).max()))
    assert _is_sentinel(got[nnz:])
    again = _outer(plan, dl, ld, dx, nrhs, torch.full_like(g, _SENTINEL))
    assert (_bits(again) == _bits(got)).all()
    # alpha = -1, beta = 0: g is not read (NaN in, numbers out); the scaling by -1 is exact
    neg = _outer(plan, dl, ld, dx, nrhs, torch.full((nnz,), float("nan"), dtype=torch.float64, device="cuda"), -1.0, 0.0)
    assert (_bits(neg) == _bits(-got[:nnz])).all()
    # alpha = 0.5, beta = 2: 0.5 S is exact, then one fma on the device against two roundings in numpy
    g0 = rng.standard_normal(nnz)
    mix = _outer(plan, dl, ld, dx, nrhs, _dev(g0), 0.5, 2.0)
    ref = 2.0 * g0 + 0.5 * S
    assert (np.abs(mix - ref) <= 0.5 * bound + 4 * _U * (np.abs(2.0 * g0) + 0.5 * M)).all()
    # the inputs and their padding are untouched
    assert (_bits(dl.cpu().numpy()) == _bits(lf)).all() and (_bits(dx.cpu().numpy()) == _bits(xf)).all()
    return got[:nnz], S, bound, (dl, dx, ld)


@pytest.mark.parametrize("ordering", ["identity", "perm"])
@pytest.mark.parametrize("name", ["tiny2d", "random", "dense150", "tridiag300", "diag37", "lap30"])
def test_pattern_outer_against_numpy(api, name, ordering, monkeypatch):
    monkeypatch.delenv("PARSY_GRAD_MRHS_MIN", raising=False)
    sym, plan, pat = _plan(api, name)
    perm = None if ordering == "identity" else sym.Perm
    rng = np.random.default_rng(11)
    try:
        plan.set_perm(perm)
        for nrhs in NRHS:
            _check_outer(plan, sym, pat, perm, nrhs, rng, LANES[nrhs])
    finally:
        plan.set_perm(None)
    info = plan.grad_info
    assert info["device_bytes"] >= 8 * int(sym.nnzA) + 16 * sym.n * 72   # coordinates + the staging of 70 right-hand sides


@pytest.mark.parametrize("nrhs", [1, 8])
def test_pattern_outer_strides_over_a_large_pattern(api, nrhs, monkeypatch):
    """nd24k-class: about 10^6 entries, several turns of the capped grid in both kernels."""
    import torch
    monkeypatch.delenv("PARSY_GRAD_MRHS_MIN", raising=False)
    sym, plan, pat = _plan(api, "nd24k")
    n, nnz = sym.n, int(sym.nnzA)
    assert nnz > 3 * 1024 * 256   # more than three turns of the direct kernel's 1024 workgroups of 256
    rng = np.random.default_rng(12)
    ld = n + 37
    lf, Lam = _padded(rng, n, nrhs, ld)
    xf, X = _padded(rng, n, nrhs, ld)
    S, M = _reference(pat, sym.Perm, Lam, X)
    try:
        plan.set_perm(sym.Perm)
        g = torch.full((nnz + 11,), _SENTINEL, dtype=torch.float64, device="cuda")
        got = _outer(plan, _dev(lf), ld, _dev(xf), nrhs, g)
    finally:
        plan.set_perm(None)
    assert plan.grad_info["last_lanes"] == LANES[nrhs]
    assert (np.abs(got[:nnz] - S) <= 4 * nrhs * _U * M).all()
    assert _is_sentinel(got[nnz:])


@pytest.mark.parametrize("nrhs", [4, 8])
@pytest.mark.parametrize("name", ["random", "lap30"])
def test_both_forms_forced(api, name, nrhs, monkeypatch):
    import torch
    sym, plan, pat = _plan(api, name)
    n, nnz = sym.n, int(sym.nnzA)
    rng = np.random.default_rng(13)
    ld = n + 37
    lf, Lam = _padded(rng, n, nrhs, ld)
    xf, X = _padded(rng, n, nrhs, ld)
    dl, dx = _dev(lf), _dev(xf)
    try:
        plan.set_perm(sym.Perm)
        S, M = _reference(pat, sym.Perm, Lam, X)
        out = {}
        for setting, lanes in (("1", 8), ("1000", 1)):
            monkeypatch.setenv("PARSY_GRAD_MRHS_MIN", setting)
            out[setting] = _outer(plan, dl, ld, dx, nrhs, torch.empty(nnz, dtype=torch.float64, device="cuda"))
            assert plan.grad_info["last_lanes"] == lanes
            assert (np.abs(out[setting] - S) <= 4 * nrhs * _U * M).all()
    finally:
        plan.set_perm(None)
    assert (np.abs(out["1"] - out["1000"]) <= 4 * nrhs * _U * M).all()


@pytest.mark.parametrize("name", DENSE)
def test_inverse_pattern(api, name):
    import torch
    from parsy_bench_amd import inspector as I
    A, sym, plan, lv = _case(api, name)
    pat = plan.pattern()
    row, col = pat["row"], pat["col"]
    z, _, _ = plan.selinv(lv)
    Zd = I.bcsc_to_dense(sym, z)
    assert np.array_equal(z[pat["dst"]], Zd[row, col])
    w = np.where(row != col, 2.0, 1.0)
    g = plan.inverse_pattern(z)
    plain = plan.inverse_pattern(z, plain=True)
    assert (_bits(g) == _bits(w * Zd[row, col])).all()
    assert (_bits(plain) == _bits(Zd[row, col])).all()
    # the device call, with alpha and beta
    nnz = int(sym.nnzA)
    dz = _dev(z)
    out = torch.full((nnz + 11,), float("nan"), dtype=torch.float64, device="cuda")
    out[nnz:] = _SENTINEL
    plan.inverse_pattern_device(dz.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (_bits(o[:nnz]) == _bits(g)).all() and _is_sentinel(o[nnz:])
    g0 = np.random.default_rng(14).standard_normal(nnz)
    d0 = _dev(g0)
    plan.inverse_pattern_device(dz.data_ptr(), d0.data_ptr(), alpha=-0.37, beta=2.0, plain=True)
    torch.cuda.synchronize()
    ref = 2.0 * g0 - 0.37 * plain
    assert (np.abs(d0.cpu().numpy() - ref) <= 4 * _U * (np.abs(2.0 * g0) + np.abs(0.37 * plain))).all()
    # against the dense inverse: test_selinv_gpu's bound and reasoning
    Zref = np.linalg.inv(_permuted_dense(A, sym))
    d = np.sqrt(np.diag(Zref))
    assert (np.abs(plain - Zref[row, col]) <= TOL * d[row] * d[col]).all()


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("name", ["tiny2d", "small3d", "random"])
def test_trace_inverse(api, name, nb):
    A, sym, plan, lv = _case(api, name)
    pat = plan.pattern()
    row, col = pat["row"], pat["col"]
    n, nnz = sym.n, int(sym.nnzA)
    z, _, _ = plan.selinv(lv)
    rng = np.random.default_rng(15)
    ldb = nnz + 5
    bf = np.full(ldb * nb, _SENTINEL)
    B = bf.reshape(nb, ldb)
    B[:, :nnz] = rng.standard_normal((nb, nnz))
    dz, db = _dev(z), _dev(bf)
    got = plan.trace_inverse_device(dz.data_ptr(), db.data_ptr(), ldb, nb)
    again = plan.trace_inverse_device(dz.data_ptr(), db.data_ptr(), ldb, nb)
    assert (_bits(got) == _bits(again)).all()
    Zref = np.linalg.inv(_permuted_dense(A, sym))
    d = np.sqrt(np.diag(Zref))
    w = np.where(row != col, 2.0, 1.0)
    for m in range(nb):
        Bd = np.zeros((n, n))
        Bd[row, col] = B[m, :nnz]
        Bd[col, row] = B[m, :nnz]
        ref = np.trace(Zref @ Bd)
        bound = nnz * _U * np.abs(w * z[pat["dst"]] * B[m, :nnz]).sum() + (w * TOL * d[row] * d[col] * np.abs(B[m, :nnz])).sum()
        assert abs(got[m] - ref) <= bound, (name, m, got[m], ref, bound)
    # B = A: tr(A^-1 A) = n
    da = _dev(sym.A2x)
    t = plan.trace_inverse_device(dz.data_ptr(), da.data_ptr(), nnz, 1)
    assert abs(t[0] - n) <= 1e-10 * n


def test_refusals(api):
    import torch
    sym, plan, pat = _plan(api, "tiny2d")
    n, nnz = sym.n, int(sym.nnzA)
    V = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
    Z = torch.zeros(int(sym.xsize), dtype=torch.float64, device="cuda")
    Bv = torch.zeros(nnz, dtype=torch.float64, device="cuda")
    G = torch.full((nnz,), _SENTINEL, dtype=torch.float64, device="cuda")
    v, z, b, g = V.data_ptr(), Z.data_ptr(), Bv.data_ptr(), G.data_ptr()
    for args in ((0, n, v, n, 1, g), (v, n, 0, n, 1, g), (v, n, v, n, 1, 0)):
        with pytest.raises(RuntimeError, match="parsy_pattern_outer_device: null argument"):
            plan.pattern_outer_device(*args)
    for nrhs in (0, -1):
        with pytest.raises(RuntimeError, match="parsy_pattern_outer_device: need nrhs >= 1"):
            plan.pattern_outer_device(v, n, v, n, nrhs, g)
    with pytest.raises(RuntimeError, match="leading dimensions >= n"):
        plan.pattern_outer_device(v, n - 1, v, n, 1, g)
    with pytest.raises(RuntimeError, match="leading dimensions >= n"):
        plan.pattern_outer_device(v, n, v, n - 1, 1, g)
    for args in ((0, g), (z, 0)):
        with pytest.raises(RuntimeError, match="parsy_inverse_pattern_device: null argument"):
            plan.inverse_pattern_device(*args)
    for args in ((0, b, nnz, 1), (z, 0, nnz, 1)):
        with pytest.raises(RuntimeError, match="parsy_trace_inverse_device: null argument"):
            plan.trace_inverse_device(*args)
    with pytest.raises(RuntimeError, match="parsy_trace_inverse_device: need 1 <= nb"):
        plan.trace_inverse_device(z, b, nnz, 0)
    with pytest.raises(RuntimeError, match="ldb >= nnz"):
        plan.trace_inverse_device(z, b, nnz - 1, 1)
    with pytest.raises(ValueError):
        plan.pattern_outer(np.zeros(n), np.zeros((n, 2)))
    with pytest.raises(ValueError):
        plan.inverse_pattern(np.zeros(3))
    torch.cuda.synchronize()
    assert _is_sentinel(G.cpu().numpy())
    # the plan still computes
    rng = np.random.default_rng(16)
    lam, x = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    S, M = _reference(pat, None, lam, x)
    assert (np.abs(plan.pattern_outer(lam, x) - S) <= 12 * _U * M).all()
    assert (np.abs(plan.pattern_outer(lam[:, 0], x[:, 0], alpha=-1.0) + _reference(pat, None, lam[:, :1], x[:, :1])[0])
            <= 4 * _U * _reference(pat, None, lam[:, :1], x[:, :1])[1]).all()
