"""Normal matrices on the plan's pattern, on the device: the values of N = F diag(w) F' + beta I + A0 at every class border
and chunk count, a column of 300 rows and the factorization of what it gives, the products by F and F', least squares
through a fresh and a stale factor, the grid generators bit for bit, and the refusals of the device calls.

The only tolerances are the derived limits of normal_ref.py (units of u = 2^-53, any summation order); every measured
value is printed (pytest -rP shows it for passing tests).

Measured on an MI355X (least squares, n = 60, m = 240, steps = 2, scaled gradient rho_g in units of u): see DESIGN.md
section 4, "Normal matrices"."""
import numpy as np
import pytest

import normal_ref as R
import shape_cases as SC
from conftest import problem
from parsy_bench_amd import inspector as I
from parsy_bench_amd.matrices import WORKLOADS

pytestmark = pytest.mark.gpu

_SENTINEL = -7.25e300
_MADE = {}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _made(api, name):
    """{F, sym, plan (device 0, under sym.Perm: a random ordering), ne, ci, cj, lens}, made once."""
    if name not in _MADE:
        F = {"borders": lambda: R.borders()[0], "tall": R.tall, "wc": R.well_conditioned}[name]()
        sym = R.analysed(F, seed=len(name) + 1)
        plan = api.Plan(sym, 0)
        plan.set_perm(np.asarray(sym.Perm))
        plan._perm_set = True
        ne = api.NormalEquations(plan, F)
        assert ne.check() == 0
        ci, cj = R.entry_coords(plan)
        lens = np.array([ne.pairs(q)[2].size for q in range(ci.size)])
        _MADE[name] = dict(F=F, sym=sym, plan=plan, ne=ne, ci=ci, cj=cj, lens=lens)
    return _MADE[name]


def _values(ne, nnz, fx, w, beta, base, in_place=False):
    """One parsy_normal_values_device call; the output has a sentinel tail, which must keep its bits."""
    import torch
    d_fx = _dev(fx)
    d_w = None if w is None else _dev(w)
    d_base = None if base is None else _dev(base)
    if in_place:
        d_out = _dev(np.concatenate([base, np.full(5, _SENTINEL)]))
        d_base = d_out
    else:
        d_out = _dev(np.full(nnz + 5, _SENTINEL))   # (every entry is written: no zero-fill)
    ne.values_device(d_fx.data_ptr(), d_out.data_ptr(), d_w=0 if d_w is None else d_w.data_ptr(), beta=beta,
                     d_base=0 if d_base is None else d_base.data_ptr())
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (_bits(out[nnz:]) == np.float64(_SENTINEL).view(np.int64)).all(), "the tail behind d_values was written"
    assert np.array_equal(_bits(d_fx.cpu().numpy()), _bits(fx))
    return out[:nnz].copy()


def test_borders(api):
    m_ = _made(api, "borders")
    F, ne, ci, cj, lens = m_["F"], m_["ne"], m_["ci"], m_["cj"], m_["lens"]
    info = ne.info
    want = {L + d for L in info["border"] for d in (-1, 0, 1)} | {511, 512, 513, 1025}
    assert want <= set(lens.tolist()), "the matrix does not reach every border"
    assert R.borders(tuple(info["border"]))[0] is F
    assert all(v > 0 for v in info["class_entries"]) and info["chunked_entries"] > 0 and info["launches"] == 5
    assert not np.array_equal(np.asarray(m_["sym"].Perm), np.arange(F.n))
    nnz = ci.size
    rng = np.random.default_rng(21)
    w = rng.uniform(-1.0, 1.0, F.m)
    w[::5] = 0.0
    base = rng.standard_normal(nnz)
    beta = 0.625
    fx = F.data
    # plain, with weights, with beta and A0
    for label, (ww, bb, aa) in {"plain": (None, 0.0, None), "w": (w, 0.0, None), "w, beta, A0": (w, beta, base)}.items():
        got = _values(ne, nnz, fx, ww, bb, aa)
        exact, limit = R.exact_values(F, fx, ww, bb, aa, ci, cj, lens)
        worst = R.within(got, exact, limit)
        print(f"borders [{label}]: error / limit = {worst:.3f}")
        assert worst <= 1.0, label
        again = _values(ne, nnz, fx, ww, bb, aa)
        assert np.array_equal(_bits(got), _bits(again)), f"{label}: two calls differ"
    # w = NULL is w = 1, bit for bit
    assert np.array_equal(_bits(_values(ne, nnz, fx, None, beta, base)), _bits(_values(ne, nnz, fx, np.ones(F.m), beta, base)))
    # in place: d_values == d_base
    full = _values(ne, nnz, fx, w, beta, base)
    assert np.array_equal(_bits(_values(ne, nnz, fx, w, beta, base, in_place=True)), _bits(full))
    # beta and A0 are honoured exactly where F produces nothing: A0_q (+ beta)
    untouched = lens == 0
    assert untouched.sum() == info["entries_untouched"] > 0
    diag = ci == cj
    assert (untouched & diag).any(), "the empty row's diagonal should be an untouched entry"
    assert np.array_equal(full[untouched], np.where(diag, beta + base, base)[untouched])
    assert np.array_equal(_values(ne, nnz, fx, w, 0.0, None)[untouched], np.zeros(int(untouched.sum())))
    assert ne.info["device_bytes"] >= 12 * info["pairs"]


def test_tall(api):
    m_ = _made(api, "tall")
    F, ne, ci, cj, lens, plan, sym = m_["F"], m_["ne"], m_["ci"], m_["cj"], m_["lens"], m_["plan"], m_["sym"]
    assert np.diff(F.indptr).max() == 300 and ne.info["pairs"] >= 45150
    rng = np.random.default_rng(23)
    w = rng.uniform(0.5, 1.5, F.m)
    beta = 1.0
    got = _values(ne, ci.size, F.data, w, beta, None)
    exact, limit = R.exact_values(F, F.data, w, beta, None, ci, cj, lens)
    worst = R.within(got, exact, limit)
    print(f"tall: error / limit = {worst:.3f}")
    assert worst <= 1.0
    # the host-buffer form gives the same bits
    assert np.array_equal(_bits(ne.values(w=w, beta=beta)[0]), _bits(got))
    # ... and the existing factorization takes them: rho_factor against the dense N, the existing measure and limit
    import torch
    d_v, d_L = _dev(got), _dev(np.zeros(int(sym.xsize)))
    plan.factor_device(d_v.data_ptr(), d_L.data_ptr())
    torch.cuda.synchronize()
    assert plan.status() == 0
    D = F.to_dense()
    Nd = np.asarray((R.ld(D) * R.ld(w)) @ R.ld(D).T + R.ld(beta) * np.eye(F.n), dtype=np.float64)
    P = np.asarray(sym.Perm)
    rho = SC.rho_factor(Nd[np.ix_(P, P)], I.bcsc_to_dense(sym, d_L.cpu().numpy()))
    print(f"tall: rho_factor = {rho:.2f} (limit {SC.limit(F.n)})")
    assert rho <= SC.limit(F.n)


def _apply(ne, op, fx, w, X, ldx, alpha, beta_y, Y0, ldy):
    """One parsy_normal_apply_device call on padded column-major operands; returns Y (rows x nrhs)."""
    import torch
    nx, nrhs = X.shape
    ny = Y0.shape[0]
    Xp = np.full((ldx, nrhs), _SENTINEL, order="F")
    Xp[:nx] = X
    Yp = np.full((ldy, nrhs), _SENTINEL, order="F")
    Yp[:ny] = Y0
    d_x, d_y, d_fx = _dev(Xp.ravel(order="F")), _dev(Yp.ravel(order="F")), _dev(fx)
    d_w = None if w is None else _dev(w)
    ne.apply_device(op, d_fx.data_ptr(), d_x.data_ptr(), ldx, nrhs, d_y.data_ptr(), ldy,
                    d_w=0 if d_w is None else d_w.data_ptr(), alpha=alpha, beta=beta_y)
    torch.cuda.synchronize()
    out = d_y.cpu().numpy().reshape((ldy, nrhs), order="F")
    assert (_bits(out[ny:]) == np.float64(_SENTINEL).view(np.int64)).all(), "rows behind Y were written"
    assert np.array_equal(_bits(d_x.cpu().numpy()), _bits(Xp.ravel(order="F"))), "X was changed"
    return out[:ny].copy()


@pytest.mark.parametrize("op", ["F", "FT"])
def test_products(api, op):
    m_ = _made(api, "borders")
    F, ne = m_["F"], m_["ne"]
    nx, ny = (F.m, F.n) if op == "F" else (F.n, F.m)
    rng = np.random.default_rng(29)
    w = rng.uniform(-1.0, 1.0, F.m)
    w[::5] = 0.0
    X17 = rng.standard_normal((nx, 17))
    Y17 = rng.standard_normal((ny, 17))
    one = {}
    for nrhs in (1, 8, 9, 17):
        for beta_y in (0.0, 0.5):
            X = X17[:, :nrhs]
            Y0 = np.full((ny, nrhs), np.nan) if beta_y == 0.0 else Y17[:, :nrhs]
            got = _apply(ne, op, F.data, w, X, nx + 3, -1.25, beta_y, Y0, ny + 5)
            exact, limit = R.product_exact(F, F.data, w, op, X, -1.25, beta_y, Y0)
            worst = R.within(got, exact, limit)
            print(f"{op} nrhs={nrhs} beta_y={beta_y}: error / limit = {worst:.3f}")
            assert worst <= 1.0
            if nrhs == 17:
                for q in range(17):
                    alone = _apply(ne, op, F.data, w, X17[:, q:q + 1], nx, -1.25, beta_y, Y0[:, q:q + 1], ny)
                    assert np.array_equal(_bits(alone[:, 0]), _bits(got[:, q])), f"column {q} depends on its neighbours"
            one[(nrhs, beta_y)] = got
    # w = NULL is w = 1 for F, and is not read for F'
    a = _apply(ne, op, F.data, None, X17[:, :3], nx, 1.0, 0.0, np.full((ny, 3), np.nan), ny)
    b = _apply(ne, op, F.data, np.ones(F.m) if op == "F" else w, X17[:, :3], nx, 1.0, 0.0, np.full((ny, 3), np.nan), ny)
    assert np.array_equal(_bits(a), _bits(b))
    # the host-buffer form: the same bits
    h, _ = ne.apply(op, X17[:, :9], w=w, alpha=-1.25, y=Y17[:, :9], beta=0.5)
    assert np.array_equal(_bits(h), _bits(one[(9, 0.5)]))


def _lsq_problem(api):
    m_ = _made(api, "wc")
    if "lv" not in m_:
        F, ne, plan = m_["F"], m_["ne"], m_["plan"]
        rng = np.random.default_rng(31)
        m_["w"] = rng.uniform(0.5, 1.5, F.m)
        m_["beta"] = 0.5
        m_["C"] = rng.standard_normal((F.m, 9))

        def factor(w):
            vals, _ = ne.values(w=w, beta=m_["beta"])
            lv, _ = plan.factor(vals)
            assert plan.status() == 0
            return lv
        m_["lv"] = factor(m_["w"])
        m_["lv_stale"] = factor(m_["w"] * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, F.m)))
    return m_


@pytest.mark.parametrize("nrhs", [1, 9])
@pytest.mark.parametrize("steps", [0, 2])
def test_least_squares(api, nrhs, steps):
    m_ = _lsq_problem(api)
    F, ne, w, beta, plan = m_["F"], m_["ne"], m_["w"], m_["beta"], m_["plan"]
    C = m_["C"][:, :nrhs]
    x, r, g = ne.lstsq(m_["lv"], C, w=w, beta=beta, steps=steps)
    assert plan.solve_status() == 0
    x, r, g = x.reshape(F.n, nrhs), r.reshape(F.m, nrhs), g.reshape(F.n, nrhs)
    # r and g are the residual and the gradient at the returned x, within the product limits
    exact, limit = R.product_exact(F, F.data, w, "FT", x, -1.0, 1.0, C)
    wr = R.within(r, exact, limit)
    exact, limit = R.product_exact(F, F.data, w, "F", r, 1.0, -beta, x)
    wg = R.within(g, exact, limit)
    print(f"nrhs={nrhs} steps={steps}: r error / limit = {wr:.3f}, g error / limit = {wg:.3f}")
    assert wr <= 1.0 and wg <= 1.0
    rho = R.rho_g(F, F.data, w, beta, C, x)
    ref = R.rho_g(F, F.data, w, beta, C, R.lstsq_float64(F, F.data, w, beta, C, steps))
    print(f"nrhs={nrhs} steps={steps}: rho_g = {rho:.2f}, float64 restatement with a dense Cholesky {ref:.2f}")
    if steps == 2:
        assert rho <= max(4.0 * ref, F.n + 1), (rho, ref)
    # the device call without r and g (the last pass is skipped) returns as good an x
    import torch
    Cf = np.asfortranarray(C)
    d_fx, d_w, d_L, d_c = _dev(F.data), _dev(w), _dev(m_["lv"]), _dev(Cf.ravel(order="F"))
    d_x = _dev(np.full(F.n * nrhs, np.nan))
    ne.lstsq_device(d_fx.data_ptr(), d_L.data_ptr(), d_c.data_ptr(), F.m, d_x.data_ptr(), F.n, nrhs, steps=steps,
                    d_w=d_w.data_ptr(), beta=beta)
    torch.cuda.synchronize()
    assert plan.solve_status() == 0
    # (the plan's solves sum with atomics: x is reproducible to rounding only, so it is held to the same measure)
    x2 = d_x.cpu().numpy().reshape((F.n, nrhs), order="F")
    assert np.isfinite(x2).all()
    rho2 = R.rho_g(F, F.data, w, beta, C, x2)
    print(f"nrhs={nrhs} steps={steps}: rho_g without r and g = {rho2:.2f}")
    if steps == 2:
        assert rho2 <= max(4.0 * ref, F.n + 1), (rho2, ref)


def test_least_squares_through_a_stale_factor(api):
    """L factored at weights perturbed by 1 %: every step of the loop shrinks the scaled gradient of the problem as
    given, one call per steps value."""
    m_ = _lsq_problem(api)
    F, ne, w, beta = m_["F"], m_["ne"], m_["w"], m_["beta"]
    C = m_["C"]
    rhos = []
    for steps in range(5):
        x, _, _ = ne.lstsq(m_["lv_stale"], C, w=w, beta=beta, steps=steps)
        rhos.append(R.rho_g(F, F.data, w, beta, C, x))
    print("stale factor, rho_g over steps 0 .. 4: " + ", ".join(f"{v:.3e}" for v in rhos))
    assert all(b < a for a, b in zip(rhos, rhos[1:])), rhos


def test_grid_generators_bitwise(api):
    """On small3d the device values of grid_edges and grid_cells (w = 1) are the host restatement of the sum, bit for bit
    (every product is exact)."""
    from parsy_bench_amd import matrices as M
    A, _, sym = problem("small3d")
    nx, ny, nz, _, shift = WORKLOADS["small3d"]
    plan = api.Plan(sym, 0)
    for F in (M.grid_edges(nx, ny, nz), M.grid_cells(nx, ny, nz)):
        ne = api.NormalEquations(plan, F)
        got, _ = ne.values(beta=shift)
        assert np.array_equal(_bits(got), _bits(R.restated_values(ne, ne.fx, None, beta=shift)))
        ne.close()


def test_refusals_leave_the_outputs_untouched(api):
    import torch
    m_ = _lsq_problem(api)
    F, ne, plan = m_["F"], m_["ne"], m_["plan"]
    nnz = int(plan.info["nnzA"])
    sent = np.float64(_SENTINEL).view(np.int64)
    d_fx, d_w, d_L = _dev(F.data), _dev(m_["w"]), _dev(m_["lv"])
    d_c = _dev(np.ones(F.m * 2))
    outs = {k: _dev(np.full(v, _SENTINEL)) for k, v in dict(v=nnz, x=F.n * 2 + 8, y=F.m * 2 + 8, r=F.m * 2, g=F.n * 2).items()}

    def refused(call, word):
        with pytest.raises(RuntimeError, match=word):
            call()
        torch.cuda.synchronize()
        for k, t in outs.items():
            assert (_bits(t.cpu().numpy()) == sent).all(), f"{word}: output {k} was written"

    p = {k: t.data_ptr() for k, t in outs.items()}
    refused(lambda: ne.values_device(0, p["v"]), "null argument")
    refused(lambda: ne.values_device(d_fx.data_ptr(), 0), "null argument")
    refused(lambda: ne.apply_device(2, d_fx.data_ptr(), d_c.data_ptr(), F.m, 1, p["x"], F.n), "op must be")
    refused(lambda: ne.apply_device("F", d_fx.data_ptr(), d_c.data_ptr(), F.m, 0, p["x"], F.n), "nrhs >= 1")
    refused(lambda: ne.apply_device("F", d_fx.data_ptr(), d_c.data_ptr(), F.m - 1, 1, p["x"], F.n), "leading dimensions")
    refused(lambda: ne.apply_device("F", d_fx.data_ptr(), d_c.data_ptr(), F.m, 1, p["x"], F.n - 1), "leading dimensions")
    refused(lambda: ne.apply_device("FT", d_fx.data_ptr(), p["x"], F.n - 1, 1, p["y"], F.m), "leading dimensions")
    refused(lambda: ne.apply_device("FT", d_fx.data_ptr(), p["x"], F.n, 1, p["x"], F.m), "same array")
    refused(lambda: ne.apply_device("FT", d_fx.data_ptr(), 0, F.n, 1, p["y"], F.m), "null argument")

    def lsq(**kw):
        a = dict(d_fx=d_fx.data_ptr(), d_lValues=d_L.data_ptr(), d_c=d_c.data_ptr(), ldc=F.m, d_x=p["x"], ldx=F.n, nrhs=2,
                 steps=1, d_w=d_w.data_ptr(), beta=0.5, d_r=p["r"], ldr=F.m, d_g=p["g"], ldg=F.n)
        a.update(kw)
        return lambda: ne.lstsq_device(**a)
    refused(lsq(steps=-1), "steps >= 0")
    refused(lsq(nrhs=0), "nrhs")
    refused(lsq(nrhs=65536), "nrhs")
    refused(lsq(ldc=F.m - 1), "leading dimensions")
    refused(lsq(ldx=F.n - 1), "leading dimensions")
    refused(lsq(ldr=F.m - 1), "leading dimensions")
    refused(lsq(ldg=F.n - 1), "leading dimensions")
    refused(lsq(d_x=d_c.data_ptr()), "same array")
    refused(lsq(d_lValues=0), "null argument")
    refused(lsq(d_c=0), "null argument")
    # what parsy_residual_device refuses: a plan restricted by set_active
    plan.set_active(np.ones(m_["sym"].nsuper, dtype=np.uint8))
    try:
        refused(lsq(), "restricted by parsy_plan_set_active")
    finally:
        plan.set_active(None)
    # ... and the same call, not refused, writes all three outputs
    lsq()()
    torch.cuda.synchronize()
    assert plan.solve_status() == 0
    for k in ("x", "r", "g"):
        assert not (_bits(outs[k].cpu().numpy())[:F.n] == sent).any()
