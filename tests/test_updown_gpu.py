"""Update and downdate of the factor on the device (parsy_factor_updown_device / _host, Plan.updown): parity with numpy's
dense Cholesky of P A P' + W W', engineered supernode shapes, the componentwise error against the dense restatement of
the algorithm (updown_ref.py), what must not move, round trips, failed downdates, the factor in use afterwards,
reproducibility, homogeneity under scaling and the info counters.

Every measured value is printed (pytest -rP shows it for passing tests) and stands in the assertion messages.
"""
import numpy as np
import pytest

import shape_cases as SC
import updown_ref as R
from conftest import problem
from parsy_bench_amd import inspector as I
from test_factor_shapes_gpu import FACTOR_TOL
from test_gpu_parity import RESID_TOL
from test_selinv_host import edge

pytestmark = pytest.mark.gpu

_SENTINEL = -7.25e300
_TAIL = 11
PATTERNS = ["tiny2d", "small3d", "lap30", "random", "dense150", "tridiag300", "diag37"]
KS = [1, 3, 8, 9, 17]
# Engineered shapes (shape_cases.arrow, analysed with ZRELAX): supernode widths 1, 16, 63, 64, 65, 129, 130, 200 over
# 0 (a root), 1, 63, 64, 65 and 257 rows below the diagonal block -- one over a 256-row workgroup, one over a tile -- and a
# chain of blocks (a deep tree with ragged row lists).
SHAPES = {
    "edges": dict(blocks=((1, 1), (16, 63), (63, 64), (64, 65), (65, 1), (129, 257)), border=260, seed=31, chain=False),
    "wide": dict(blocks=((200, 65), (130, 257), (64, 0)), border=300, seed=32, chain=False),
    "chain": dict(blocks=((17, 20), (33, 30), (65, 25), (129, 40), (64, 30)), border=100, seed=33, chain=True),
}
_NAMED, _SHAPED, _ENTRIES = {}, {}, {}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _named(api, name):
    """{sym, plan (under sym.Perm), lv: the factor of sym.A2x, Sp: P A P' dense (None for lap30)}, made once."""
    if name not in _NAMED:
        from parsy_bench_amd import matrices as M
        if name == "random":
            A = M.random_spd(300, density=0.03, seed=5)
            sym = I.analyze(A, None)
        elif name in ("dense150", "tridiag300", "diag37"):
            A, sym = edge(name)
        else:
            A, _, sym = problem(name)
        _NAMED[name] = _made(api, A, sym, A.to_dense() if sym.n <= 1000 else None)
    return _NAMED[name]


def _shaped(api, shape):
    if shape not in _SHAPED:
        spec = SHAPES[shape]
        A, S = SC.arrow(spec["blocks"], spec["border"], spec["seed"], spec["chain"])
        sym = I.analyze(A, None, zrelax=SC.ZRELAX)
        want = SC.arrow_layout(spec["blocks"], spec["border"], spec["seed"], spec["chain"])[1]
        assert sorted(SC.supernodes_of(sym)) == sorted(want), (shape, SC.supernodes_of(sym), want)
        _SHAPED[shape] = _made(api, A, sym, S)
    return _SHAPED[shape]


def _made(api, A, sym, dense):
    plan = api.Plan(sym, 0)
    plan.set_perm(np.asarray(sym.Perm))
    lv, _ = plan.factor(sym.A2x)
    assert plan.status() == 0
    P = np.asarray(sym.Perm)
    return {"A": A, "sym": sym, "plan": plan, "lv": lv, "Sp": None if dense is None else dense[np.ix_(P, P)]}


def _entries(sym):
    if id(sym) not in _ENTRIES:
        _ENTRIES[id(sym)] = (sym, R.entries(sym))
    return _ENTRIES[id(sym)][1]


def _leaf_columns(sym):
    has_child = np.zeros(sym.nsuper, dtype=bool)
    par = np.asarray(sym.sParent)
    has_child[par[(par >= 0) & (par < sym.nsuper) & (par != np.arange(sym.nsuper))]] = True
    return [int(sym.super[s]) for s in np.flatnonzero(~has_child)]


def _starts(sym, k, seed):
    """k start columns spread from the leaves to the root: a leaf, column n - 1, and columns in between."""
    rng = np.random.default_rng(seed)
    leaves = _leaf_columns(sym)
    out = [leaves[int(rng.integers(len(leaves)))]]
    if k >= 2:
        out.append(sym.n - 1)
    spread = np.linspace(0, sym.n - 1, max(k, 2)).astype(int)
    while len(out) < k:
        out.append(int(spread[len(out)] if rng.random() < 0.5 else leaves[int(rng.integers(len(leaves)))]))
    return out[:k]


def _run(plan, sym, lv, Wp, sign):
    """One parsy_factor_updown_device call on a copy of lv with a sentinel tail, W given in the factor's ordering.
    Returns the new lValues; asserts that the tail and W's values kept their bits."""
    import torch
    wp, wi, wx = plan._w_csc(R.to_caller(sym, Wp), sym.n)
    d_wx = _dev(wx if wx.size else np.zeros(1))
    dL = _dev(np.concatenate([lv, np.full(_TAIL, _SENTINEL)]))
    plan.updown_device(dL.data_ptr(), wp, wi, d_wx.data_ptr(), sign=sign)
    torch.cuda.synchronize()
    out = dL.cpu().numpy()
    assert (_bits(out[lv.size:]) == np.float64(_SENTINEL).view(np.int64)).all(), "the tail behind lValues was written"
    if wx.size:
        assert np.array_equal(_bits(d_wx.cpu().numpy()), _bits(wx)), "the values of W were changed"
    return out[:lv.size].copy()


def _path_columns(sym, sn, fc):
    return np.concatenate([np.arange(int(f), int(sym.super[int(s) + 1])) for s, f in zip(sn, fc)])


def _assert_rest_kept(sym, lv0, lv1, Wp, what):
    """Item 4: everything off the path and every column before the entry column keeps its bits, the strict upper
    triangles of the diagonal blocks too (zero after a factorization)."""
    starts = [int(np.flatnonzero(Wp[:, t])[0]) for t in range(Wp.shape[1]) if Wp[:, t].any()]
    sn, fc = R.path_of(sym, starts)
    row, col, off, esn, upper = _entries(sym)
    on_path = np.zeros(sym.n, dtype=bool)
    if sn.size:
        on_path[_path_columns(sym, sn, fc)] = True
    keep = np.ones(lv0.size, dtype=bool)
    keep[off[on_path[col]]] = False
    moved = np.flatnonzero(_bits(lv0)[keep] != _bits(lv1)[keep])
    assert moved.size == 0, f"{what}: {moved.size} entries off the path (or before the entry column) changed"
    assert np.array_equal(_bits(lv0[upper]), _bits(lv1[upper])), f"{what}: a strict upper triangle was written"
    return sn, fc


def _check_against_cholesky(case, lv0, lv1, Wp, coef, what):
    """lv1 against numpy.linalg.cholesky(P A P' + coef W W') on the stored entries, limit FACTOR_TOL max|L|.  Patterns too
    large for a dense factor (lap30): with C the path's columns, L_new[C, C] is the Cholesky factor of
    L[C, C] L[C, C]' + coef W[C] W[C]' (the other columns of L keep their values, and so does what they contribute to
    A[C, C]), so the dense factor is formed for those columns alone; everything else is compared bit for bit."""
    sym = case["sym"]
    row, col, off, _, _ = _entries(sym)
    sn, fc = _assert_rest_kept(sym, lv0, lv1, Wp, what)
    if case["Sp"] is not None:
        want = np.linalg.cholesky(case["Sp"] + coef * (Wp @ Wp.T))
        err = np.abs(lv1[off] - want[row, col]).max() / np.abs(want).max()
    else:
        C = _path_columns(sym, sn, fc)
        sel = np.isin(col, C)
        r, c, o = np.searchsorted(C, row[sel]), np.searchsorted(C, col[sel]), off[sel]
        assert np.array_equal(C[r], row[sel]), "a row of a path panel is a column of the path"
        L0 = np.zeros((C.size, C.size))
        L0[r, c] = lv0[o]
        want = np.linalg.cholesky(L0 @ L0.T + coef * (Wp[C] @ Wp[C].T))
        err = np.abs(lv1[o] - want[r, c]).max() / np.abs(want).max()
    print(f"UPDOWN_PARITY {what}: n={sym.n} path_supernodes={sn.size} err={err:.3e}")
    assert err <= FACTOR_TOL, f"{what}: max|L - cholesky| / max|L| = {err:.3e}"
    return sn, fc


# ---- 1. parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", PATTERNS)
def test_update_matches_dense_cholesky(api, name, k):
    case = _named(api, name)
    sym, plan = case["sym"], case["plan"]
    Wp = R.admissible_w(sym, _starts(sym, k, 100 * k + len(name)), seed=k)
    lv1 = _run(plan, sym, case["lv"], Wp, +1)
    assert plan.updown_status() == 0
    _check_against_cholesky(case, case["lv"], lv1, Wp, 1.0, f"{name} k={k}")


# ---- 2. engineered shapes -------------------------------------------------------------------------------------------
def _scenarios(sym):
    """Named lists of start columns (factor's ordering) for an engineered shape."""
    sup = np.asarray(sym.super)
    widths = np.diff(sup)
    out = {
        "first_columns": [int(c) for c in sup[:-1]],
        "last_columns": [int(c) - 1 for c in sup[1:]],
        "last_column_of_all": [sym.n - 1],
        "two_branches": [int(sup[0]), int(sup[1] - 1) if sym.nsuper > 2 else 0, int(sup[min(2, sym.nsuper - 1)])],
    }
    for s in np.flatnonzero(widths >= 129):
        out[f"second_block_column_of_{int(widths[s])}"] = [int(sup[s]) + 70]
    return out


@pytest.mark.parametrize("shape", list(SHAPES))
def test_update_on_engineered_shapes(api, shape):
    """Starts at the first and the last column of every supernode, at column 70 of the wide ones (the second block column,
    offset 6), at column n - 1 and on branches that merge at the border; whole structures (full=True) and random subsets."""
    case = _shaped(api, shape)
    sym, plan = case["sym"], case["plan"]
    for label, starts in _scenarios(sym).items():
        for full in (True, False):
            Wp = R.admissible_w(sym, starts, seed=len(label), full=full)
            lv1 = _run(plan, sym, case["lv"], Wp, +1)
            assert plan.updown_status() == 0
            sn, fc = _check_against_cholesky(case, case["lv"], lv1, Wp, 1.0, f"{shape} {label} full={full}")
            info = plan.updown_info
            assert info["path_supernodes"] == sn.size and info["block_columns"] == R.block_columns(sym, sn, fc)
            if label.startswith("second_block_column"):
                assert fc[0] - int(sym.super[sn[0]]) == 70


# ---- 3. componentwise error -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_componentwise_error_against_the_restatement(api, shape):
    """rho_factor (shape_cases.py, units of u) of the device's result against 4 x the same measure of the dense numpy
    restatement on the same input; the margin is for another, equivalent order (blocks of 8 columns of W), the stored
    reciprocal and fused multiply-adds.  Measured on an MI355X: DESIGN.md, section 4."""
    case = _shaped(api, shape)
    sym, plan, Sp = case["sym"], case["plan"], case["Sp"]
    sc = _scenarios(sym)
    starts = (sc["first_columns"] + sc["last_columns"])[:9]
    Wp = R.admissible_w(sym, starts, seed=7)
    L0 = I.bcsc_to_dense(sym, case["lv"])
    # the downdate must leave a positive definite matrix: W is scaled to take half of the smallest eigenvalue at most
    small = np.sqrt(0.5 * np.linalg.eigvalsh(Sp)[0] / np.linalg.norm(Wp, 2) ** 2)
    for sign, W in ((+1, Wp), (-1, small * Wp)):
        target = Sp + sign * (W @ W.T)
        lv1 = _run(plan, sym, case["lv"], W, sign)
        assert plan.updown_status() == 0
        ref, bad = R.updown_dense(L0, W, sign)
        assert bad is None
        rho_ref = SC.rho_factor(target, ref)
        rho = SC.rho_factor(target, I.bcsc_to_dense(sym, lv1))
        print(f"UPDOWN_RHO shape={shape} sign={sign:+d} n={sym.n} k={len(starts)} rho={rho:.2f} restatement={rho_ref:.2f}")
        assert rho <= 4.0 * rho_ref, f"{shape} sign={sign}: rho_factor = {rho:.4g} > 4 x {rho_ref:.4g} (the restatement's)"


# ---- 4. what must not move, on values that are no factor ----------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_random_values_off_the_path_keep_their_bits(api, shape):
    """lValues full of random numbers, the strict upper triangles of the diagonal blocks included (never read, never
    written): everything off the path, every column before the entry column, the tail and W's values keep their bits."""
    case = _shaped(api, shape)
    sym, plan = case["sym"], case["plan"]
    lv = np.random.default_rng(5).standard_normal(int(sym.xsize))
    for label, starts in _scenarios(sym).items():
        Wp = R.admissible_w(sym, starts, seed=11)
        lv1 = _run(plan, sym, lv, Wp, +1)
        sn, fc = _assert_rest_kept(sym, lv, lv1, Wp, f"{shape} {label}")
        assert np.isfinite(lv1).all()
        changed = np.flatnonzero(_bits(lv) != _bits(lv1))
        assert changed.size > 0, "the update changed nothing"


# ---- 5. round trip and downdate -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small3d", "random", "dense150", "edges", "chain"])
def test_round_trip_and_downdate(api, name):
    case = _shaped(api, name) if name in SHAPES else _named(api, name)
    sym, plan, lv = case["sym"], case["plan"], case["lv"]
    Wp = R.admissible_w(sym, _starts(sym, 9, 3), seed=9)
    up = _run(plan, sym, lv, Wp, +1)
    assert plan.updown_status() == 0
    back = _run(plan, sym, up, Wp, -1)
    assert plan.updown_status() == 0
    err = np.abs(back - lv).max() / np.abs(lv).max()
    print(f"UPDOWN_ROUND_TRIP {name}: err={err:.3e}")
    assert err <= FACTOR_TOL, f"{name}: update then downdate leaves max|L - L0| / max|L| = {err:.3e}"
    half = _run(plan, sym, up, 0.5 * Wp, -1)
    assert plan.updown_status() == 0
    _check_against_cholesky(case, up, half, Wp, 0.75, f"{name} downdate by W / 2")


# ---- 6. failed downdate -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["leaf", "last"])
def test_failed_downdate_reports_the_column(api, where):
    case = _named(api, "small3d")
    sym, plan, lv = case["sym"], case["plan"], case["lv"]
    j = _leaf_columns(sym)[0] if where == "leaf" else sym.n - 1
    Wp = np.zeros((sym.n, 1))
    Wp[j, 0] = 1.5 * I.bcsc_to_dense(sym, lv)[j, j]
    bad = _run(plan, sym, lv, Wp, -1)
    assert plan.updown_status() == j + 1
    assert np.isfinite(bad).all(), "a failed pivot spread NaN or Inf"
    # the same W as an update is fine, and the plan goes on: factor again, update, compare
    lv2, _ = plan.factor(sym.A2x)
    assert plan.status() == 0 and np.array_equal(lv2, lv)
    W3 = R.admissible_w(sym, _starts(sym, 3, 1), seed=3)
    lv3 = _run(plan, sym, lv2, W3, +1)
    assert plan.updown_status() == 0
    _check_against_cholesky(case, lv2, lv3, W3, 1.0, f"after a failed downdate at {where}")


# ---- 7. the factor is usable --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small3d", "random"])
def test_updated_factor_solves_and_gives_the_logdet(api, name):
    """Plan.updown (host buffers, W dense in the caller's ordering), then solve_spd against the dense A + W W' and
    logdet_device against the factor's diagonal."""
    case = _named(api, name)
    sym, plan, lv = case["sym"], case["plan"], case["lv"]
    Wc = R.to_caller(sym, R.admissible_w(sym, _starts(sym, 5, 2), seed=5))
    lv1, sec = plan.updown(lv, Wc, sign=+1)
    assert plan.updown_status() == 0 and sec >= 0.0 and not np.array_equal(lv1, lv)
    Anew = case["A"].to_dense() + Wc @ Wc.T
    B = np.random.default_rng(12).standard_normal((sym.n, 3))
    X, _ = plan.solve_spd(lv1, B)
    res = np.abs(Anew @ X - B).max()
    assert res <= RESID_TOL * (np.abs(Anew).max() * np.abs(X).max() + np.abs(B).max()), res
    want = np.linalg.solve(Anew, B)
    assert np.abs(X - want).max() <= RESID_TOL * np.linalg.cond(Anew) * np.abs(want).max()
    diag = np.diag(I.bcsc_to_dense(sym, lv1))
    ref = 2.0 * np.log(diag).sum()
    got, col = plan.logdet_device(_dev(lv1).data_ptr())
    assert col == 0 and abs(got - ref) <= 1e-12 * max(1.0, abs(ref))
    assert abs(got - np.linalg.slogdet(Anew)[1]) <= 1e-10 * max(1.0, abs(ref))
    # a single column as a vector, and as a (wp, wi, wx) triple: the same bits
    one, _ = plan.updown(lv, Wc[:, 0])
    wp, wi, wx = plan._w_csc(Wc[:, :1], sym.n)
    tri, _ = plan.updown(lv, (wp, wi, wx))
    assert np.array_equal(_bits(one), _bits(tri)) and not np.array_equal(one, lv)


# ---- 8. reproducible and homogeneous ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_reproducible_and_homogeneous_under_scaling(api, shape):
    """Two runs are bitwise equal; and with D = diag(2^k) in the caller's ordering, the factor of D S D updated by D W is
    D L_new bitwise, update and downdate: square roots, quotients and fused multiply-adds of terms that carry the same
    power of two are exact under the scaling, as test_factor_is_homogeneous_under_scaling holds for the factorization."""
    case = _shaped(api, shape)
    sym, plan, lv = case["sym"], case["plan"], case["lv"]
    seed = 200 + SHAPES[shape]["seed"]
    sc = _scenarios(sym)
    Wp = R.admissible_w(sym, (sc["first_columns"] + sc["last_columns"])[:17], seed=13)
    lvs, _ = plan.factor(sym.permute_values(SC.scaled_values(case["A"], seed)))
    assert plan.status() == 0
    d = SC.scaling(sym.n, seed)[np.asarray(sym.Perm)]
    assert np.array_equal(I.bcsc_to_dense(sym, lvs), d[:, None] * I.bcsc_to_dense(sym, lv)), "the factorization itself"
    small = np.sqrt(0.5 * np.linalg.eigvalsh(case["Sp"])[0] / np.linalg.norm(Wp, 2) ** 2)
    small = 2.0 ** np.floor(np.log2(small))
    for sign, W in ((+1, Wp), (-1, small * Wp)):
        a, b = _run(plan, sym, lv, W, sign), _run(plan, sym, lv, W, sign)
        assert plan.updown_status() == 0
        assert np.array_equal(_bits(a), _bits(b)), f"{shape} sign={sign}: two runs differ"
        got = _run(plan, sym, lvs, d[:, None] * W, sign)
        assert plan.updown_status() == 0
        want = d[:, None] * I.bcsc_to_dense(sym, a)
        diff = int((want != I.bcsc_to_dense(sym, got)).sum())
        print(f"UPDOWN_SCALING shape={shape} sign={sign:+d} entries_that_differ={diff}")
        assert diff == 0, f"{shape} sign={sign}: {diff} entries of the update of L(D S D) by D W differ from D L_new"


# ---- 9. info ------------------------------------------------------------------------------------------------------
def test_info_counters_and_no_ops(api):
    import torch
    case = _shaped(api, "wide")
    sym, lv = case["sym"], case["lv"]
    plan = api.Plan(sym, 0)
    plan.set_perm(np.asarray(sym.Perm))
    before = plan.info["device_bytes"]
    assert plan.updown_info["device_bytes"] == 0 and plan.updown_status() == 0
    # k = 0 and an all-zero W: nothing is launched, nothing is allocated, lValues keeps its bits
    for Wp in (np.zeros((sym.n, 0)), np.zeros((sym.n, 3))):
        same = _run(plan, sym, lv, Wp, +1)
        info = plan.updown_info
        assert np.array_equal(_bits(same), _bits(lv))
        assert info["last_launches"] == 0 and info["path_supernodes"] == 0 and info["block_columns"] == 0
        assert info["last_k"] == Wp.shape[1] and info["entries_touched"] == 0 and info["device_bytes"] == 0
    host, _ = plan.updown(lv, np.zeros((sym.n, 0)))
    assert np.array_equal(_bits(host), _bits(lv)) and plan.info["device_bytes"] == before
    starts = _scenarios(sym)["two_branches"] + [int(sym.super[1]) + 70]
    Wp = R.admissible_w(sym, starts * 3, seed=2)        # 12 columns: two blocks
    _run(plan, sym, lv, Wp, -1)
    sn, fc = R.path_of(sym, starts)
    got_sn, got_fc = plan.updown_path(R.to_caller(sym, Wp))
    assert np.array_equal(got_sn, sn) and np.array_equal(got_fc, fc)
    info = plan.updown_info
    assert info["path_supernodes"] == sn.size and info["block_columns"] == R.block_columns(sym, sn, fc)
    assert info["last_k"] == 12 and info["last_sign"] == -1
    # per block of 8 columns: a scatter and a clear, and one or two launches per block column
    assert 2 * 2 + 2 * info["block_columns"] <= info["last_launches"] <= 2 * 2 + 2 * 2 * info["block_columns"]
    stored = sum(sum(R.panel(sym, int(s))[4] - (j - R.panel(sym, int(s))[0]) for j in range(int(f), int(sym.super[int(s) + 1])))
                 for s, f in zip(sn, fc))
    assert info["entries_touched"] == 2 * stored
    assert info["device_bytes"] >= 8 * 8 * sym.n
    assert plan.info["device_bytes"] == before + info["device_bytes"]
    # a restricted plan refuses; the restriction lifted, it goes on
    plan.set_active(np.ones(sym.nsuper, dtype=np.uint8))
    with pytest.raises(RuntimeError, match="parsy_factor_updown_device: plan is restricted by parsy_plan_set_active"):
        _run(plan, sym, lv, Wp, +1)
    plan.set_active(None)
    _run(plan, sym, lv, Wp, +1)
    assert plan.updown_status() == 0
    torch.cuda.synchronize()
    plan.close()
