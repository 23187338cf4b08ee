"""Selected inversion (parsy_selinv_device / _host), diag(A^-1) in the caller's ordering (parsy_inverse_diag_device) and
log det A (parsy_logdet_device) on the device: Z against numpy's dense inverse and scipy solves on the pattern of L,
both kernel paths, bitwise reproducibility, and the refusals.  Checked against numpy / scipy only."""
import numpy as np
import pytest
from scipy.sparse.linalg import splu

from conftest import problem
from test_selinv_host import edge

pytestmark = pytest.mark.gpu

_SENTINEL = -7.25e300
_CASES = {}
DENSE = ["tiny2d", "small3d", "ex15", "random", "dense150", "tridiag300", "diag37"]
SAMPLED = ["mid3d", "lap30", "nd24k", "parabolic_fem"]
# |Z_ij| <= sqrt(Z_ii Z_jj) (Z is SPD), so this bound is relative to the largest value the entry can take; the
# factorization and the recurrences are backward stable and these matrices are well conditioned (a 0.1 or 0.01 shift,
# or diagonal dominance), so an error above 1e-10 of that scale is a bug, not rounding.
TOL = 1e-10


def _case(api, name):
    """(A lower CSC, sym, plan on device 0, lValues of sym.A2x), per name."""
    if name not in _CASES:
        from parsy_bench_amd import inspector as I, matrices as M
        if name == "random":
            A = M.random_spd(300, density=0.03, seed=5)
            sym = I.analyze(A, None)
        elif name in ("dense150", "tridiag300", "diag37"):
            A, sym = edge(name)
        else:
            A, _, sym = problem(name)
        plan = api.Plan(sym, 0)
        lv, _ = plan.factor(sym.A2x)
        assert plan.status() == 0
        _CASES[name] = (A, sym, plan, lv)
    return _CASES[name]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _permuted_dense(A, sym):
    P = sym.Perm
    return A.to_dense()[np.ix_(P, P)]


def _diag_offsets(sym):
    """Offset in lValues of every column's diagonal entry."""
    off = np.empty(sym.n, dtype=np.int64)
    for s in range(sym.nsuper):
        for c in range(int(sym.super[s]), int(sym.super[s + 1])):
            off[c] = int(sym.p[c]) + (c - int(sym.super[s]))
    return off


@pytest.mark.parametrize("threshold", [None, "0", "1000000000"])
@pytest.mark.parametrize("name", DENSE)
def test_dense_inverse_on_the_pattern(api, name, threshold, monkeypatch):
    from parsy_bench_amd import inspector as I
    if threshold is not None:
        monkeypatch.setenv("PARSY_SELINV_TILED_MIN", threshold)
    A, sym, plan, lv = _case(api, name)
    z, diag, sec = plan.selinv(lv)
    Zref = np.linalg.inv(_permuted_dense(A, sym))
    Zd = I.bcsc_to_dense(sym, z)
    mask = np.tril(I.bcsc_to_dense(sym, np.ones(int(sym.xsize))) != 0)
    d = np.sqrt(np.diag(Zref))
    err = np.abs(Zd - np.where(mask, Zref, 0.0)) / np.outer(d, d)
    assert err.max() <= TOL, (name, threshold, float(err.max()))
    assert (Zd[np.triu_indices(sym.n, 1)] == 0).all()   # incl. the upper part of every diagonal block
    assert np.abs(diag - np.diag(Zref)).max() <= TOL * np.diag(Zref).max()
    assert sec > 0


def test_both_paths_are_taken(api, monkeypatch):
    """The thresholds the dense checks run under send ex15's block columns to both paths; 40 rows mixes them."""
    A, sym, plan, lv = _case(api, "ex15")
    seen = {}
    for t in (None, "0", "40", "1000000000"):
        if t is None:
            monkeypatch.delenv("PARSY_SELINV_TILED_MIN", raising=False)
        else:
            monkeypatch.setenv("PARSY_SELINV_TILED_MIN", t)
        plan.selinv(lv)
        info = plan.selinv_info
        seen[t] = (info["tiled_block_columns"], info["block_columns"])
    assert seen["0"][0] == seen["0"][1] and seen["1000000000"][0] == 0
    assert 0 < seen["40"][0] < seen["40"][1]
    assert seen[None][1] == seen["0"][1] and seen[None][0] > 0


def _sample_columns(sym, k=24, seed=3):
    roots = [s for s in range(sym.nsuper) if sym.sParent[s] < 0]
    has_child = np.zeros(sym.nsuper, bool)
    has_child[sym.sParent[sym.sParent >= 0]] = True
    leaf = int(np.nonzero(~has_child)[0][0])
    cols = set()
    for s in (roots[-1], leaf):
        cols.add(int(sym.super[s]))
        cols.add(int(sym.super[s + 1]) - 1)
    rng = np.random.default_rng(seed)
    while len(cols) < k:
        cols.add(int(rng.integers(sym.n)))
    return sorted(cols)


@pytest.mark.parametrize("name", SAMPLED)
def test_sampled_columns_against_scipy(api, name):
    A, sym, plan, lv = _case(api, name)
    z, diag, _ = plan.selinv(lv)
    cols = _sample_columns(sym)
    P = sym.Perm
    Ap = A.to_scipy().tocsr()[P][:, P].tocsc()
    lu = splu(Ap, permc_spec="NATURAL")
    E = np.zeros((sym.n, len(cols)))
    E[cols, np.arange(len(cols))] = 1.0
    Zc = lu.solve(E)
    for q, c in enumerate(cols):
        s = int(sym.col2Sup[c])
        c0 = int(sym.super[s])
        b, e = int(sym.i_ptr[c0]), int(sym.i_ptr[int(sym.super[s + 1])])
        rows = sym.s[b:e]
        keep = rows >= c
        got = z[int(sym.p[c]):int(sym.p[c]) + (e - b)][keep]
        ref = Zc[rows[keep], q]
        bound = TOL * np.sqrt(np.abs(diag[rows[keep]]) * diag[c])
        assert (np.abs(got - ref) <= bound).all(), (name, c, float(np.abs(got - ref).max()))
    assert np.abs(diag[cols] - Zc[cols, np.arange(len(cols))]).max() <= TOL * diag.max()


@pytest.mark.parametrize("name", ["ex15", "random", "dense150"])
def test_inverse_diag_in_the_callers_ordering(api, name):
    import torch
    A, sym, plan, lv = _case(api, name)
    n = sym.n
    Ld = _dev(lv)
    Zd = torch.empty(int(sym.xsize), dtype=torch.float64, device="cuda")
    plan.selinv_device(Ld.data_ptr(), Zd.data_ptr())
    Dd = _dev(np.full(n + 11, _SENTINEL))
    Ainv = np.linalg.inv(A.to_dense())
    try:
        plan.set_perm(sym.Perm)
        plan.inverse_diag_device(Zd.data_ptr(), Dd.data_ptr())
        torch.cuda.synchronize()
        out = Dd.cpu().numpy()
        assert np.abs(out[:n] - np.diag(Ainv)).max() <= TOL * np.diag(Ainv).max()
        assert (out[n:].view(np.int64) == np.float64(_SENTINEL).view(np.int64)).all()
        plan.set_perm(None)
        plan.inverse_diag_device(Zd.data_ptr(), Dd.data_ptr())
        torch.cuda.synchronize()
        out = Dd.cpu().numpy()
        Zp = np.linalg.inv(_permuted_dense(A, sym))
        assert np.abs(out[:n] - np.diag(Zp)).max() <= TOL * np.diag(Zp).max()
        assert (out[n:].view(np.int64) == np.float64(_SENTINEL).view(np.int64)).all()
    finally:
        plan.set_perm(None)


@pytest.mark.parametrize("name", ["tiny2d", "ex15", "random", "dense150", "tridiag300", "diag37"])
def test_logdet_dense(api, name):
    A, sym, plan, lv = _case(api, name)
    sign, ref = np.linalg.slogdet(A.to_dense())
    assert sign > 0
    got, col = plan.logdet_device(_dev(lv).data_ptr())
    assert col == 0
    assert abs(got - ref) <= 1e-11 * max(1.0, abs(ref))


@pytest.mark.parametrize("name", ["lap30", "nd24k"])
def test_logdet_against_the_factor_diagonal(api, name):
    A, sym, plan, lv = _case(api, name)
    ref = 2.0 * np.log(lv[_diag_offsets(sym)]).sum()
    got, col = plan.logdet_device(_dev(lv).data_ptr())
    assert col == 0
    assert abs(got - ref) <= 1e-12 * abs(ref)


def test_logdet_reports_a_bad_pivot(api):
    A, sym, plan, lv = _case(api, "ex15")
    off = _diag_offsets(sym)
    bad = lv.copy()
    bad[off[sym.n // 3]] = -0.5
    bad[off[sym.n // 2]] = 0.0
    got, col = plan.logdet_device(_dev(bad).data_ptr())
    assert col == sym.n // 3 + 1 and np.isnan(got)


@pytest.mark.parametrize("name", ["ex15", "lap30"])
def test_reproducible(api, name):
    import torch
    A, sym, plan, lv = _case(api, name)
    plan2 = api.Plan(sym, 0)
    Ld = _dev(lv)
    outs = []
    for p in (plan, plan, plan2):
        Zd = torch.full((int(sym.xsize),), _SENTINEL, dtype=torch.float64, device="cuda")
        Dd = torch.empty(sym.n, dtype=torch.float64, device="cuda")
        p.selinv_device(Ld.data_ptr(), Zd.data_ptr())
        p.inverse_diag_device(Zd.data_ptr(), Dd.data_ptr())
        ld, _ = p.logdet_device(Ld.data_ptr())
        torch.cuda.synchronize()
        outs.append((Zd.cpu().numpy().view(np.int64), Dd.cpu().numpy().view(np.int64), np.float64(ld).view(np.int64)))
    for o in outs[1:]:
        assert (o[0] == outs[0][0]).all() and (o[1] == outs[0][1]).all() and o[2] == outs[0][2]
    info = plan.selinv_info
    assert info["device_bytes"] > 0 and plan2.selinv_info["device_bytes"] > 0
    plan2.close()


def test_refusals_leave_the_plan_usable(api):
    import torch
    A, sym, plan, lv = _case(api, "ex15")
    n = sym.n
    Ld = _dev(lv)
    L = Ld.data_ptr()
    Zd = torch.full((int(sym.xsize),), _SENTINEL, dtype=torch.float64, device="cuda")
    Dd = torch.full((n,), _SENTINEL, dtype=torch.float64, device="cuda")
    z, dg = Zd.data_ptr(), Dd.data_ptr()
    with pytest.raises(RuntimeError, match="null argument"):
        plan.selinv_device(0, z)
    with pytest.raises(RuntimeError, match="null argument"):
        plan.selinv_device(L, 0)
    with pytest.raises(RuntimeError, match="null argument"):
        plan.inverse_diag_device(z, 0)
    with pytest.raises(RuntimeError, match="null argument"):
        plan.logdet_device(0)
    with pytest.raises(RuntimeError, match="overlaps"):
        plan.selinv_device(L, L + 8 * (int(sym.xsize) - 1))
    plan.set_active(np.ones(sym.nsuper, dtype=np.uint8))
    try:
        with pytest.raises(RuntimeError, match="set_active"):
            plan.selinv_device(L, z)
        with pytest.raises(RuntimeError, match="set_active"):
            plan.inverse_diag_device(z, dg)
        with pytest.raises(RuntimeError, match="set_active"):
            plan.logdet_device(L)
    finally:
        plan.set_active(None)
    vals = _dev(sym.A2x)
    Lscratch = _dev(np.zeros(int(sym.xsize)))
    plan.factor_begin(vals.data_ptr(), Lscratch.data_ptr())
    try:
        with pytest.raises(RuntimeError, match="factorization is still open"):
            plan.selinv_device(L, z)
        with pytest.raises(RuntimeError, match="factorization is still open"):
            plan.logdet_device(L)
    finally:
        for lev in range(int(plan.info["chol_levels"])):
            plan.factor_level(lev, Lscratch.data_ptr())
        plan.factor_end()
    X = torch.zeros((2, n), dtype=torch.float64, device="cuda")
    plan.solve_levels_device(L, X.data_ptr(), 2, n, 0, 0, 1, True, False)
    with pytest.raises(RuntimeError, match="steps of levels"):
        plan.selinv_device(L, z)
    with pytest.raises(RuntimeError, match="steps of levels"):
        plan.inverse_diag_device(z, dg)
    plan.solve_levels_device(L, X.data_ptr(), 2, n, 0, 1, int(plan.solve_levels().max()) + 1, False, True)
    torch.cuda.synchronize()
    # the outputs were left untouched
    sent = np.float64(_SENTINEL).view(np.int64)
    assert (Zd.cpu().numpy().view(np.int64) == sent).all() and (Dd.cpu().numpy().view(np.int64) == sent).all()
    # the factor still solves correctly on the same plan, and the plan still inverts
    b = np.random.default_rng(4).standard_normal(n)
    x, _ = plan.solve_spd(lv, b)
    Af = A.to_scipy()
    assert np.abs(Af @ x - b).max() <= 1e-10 * np.abs(b).max()
    z2, diag2, _ = plan.selinv(lv)
    assert np.isfinite(z2).all() and (diag2 > 0).all()
