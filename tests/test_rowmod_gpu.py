"""Row delete and row add in the factor on the device (parsy_factor_rowdel_device / parsy_factor_rowadd_device and their
host forms, Plan.rowdel / Plan.rowadd): parity with numpy's dense Cholesky of the modified matrix on engineered supernode
shapes and named patterns, that an add never reads what it overwrites, round trips, the componentwise error against the
dense restatement (rowmod_ref.py), what must not move, failures, the factor in use afterwards, reproducibility and the
info counters.

lap30 (n = 27000) has no dense factor: its deletes are checked on the path's columns alone, as test_updown_gpu.py does,
and its adds against the plan's own factor of the full matrix.

Every measured value is printed (pytest -rP shows it for passing tests) and stands in the assertion messages.
"""
import numpy as np
import pytest

import rowmod_ref as RR
import shape_cases as SC
import updown_ref as R
from parsy_bench_amd import inspector as I
from test_gpu_parity import FACTOR_TOL, RESID_TOL
from test_updown_gpu import PATTERNS, SHAPES, _SENTINEL, _TAIL, _bits, _dev, _entries, _named, _shaped

pytestmark = pytest.mark.gpu

ALL = list(SHAPES) + PATTERNS
_COLS = {}


def _case(api, name):
    return _shaped(api, name) if name in SHAPES else _named(api, name)


def _sym_columns(sym):
    """(rows, cols, values) of the full symmetric P A P' from the A2 arrays (lower triangle, factor's ordering)."""
    if id(sym) not in _COLS:
        col = np.repeat(np.arange(sym.n), np.diff(np.asarray(sym.A2p)))
        _COLS[id(sym)] = (sym, np.asarray(sym.A2i, dtype=np.int64), col.astype(np.int64))
    return _COLS[id(sym)][1:]


def _column(sym, p, values=None, scale=1.0, lift=0.0):
    """(ci, cx): column p (factor's ordering) of the symmetric matrix with these A2 values, in the caller's ordering and
    ascending; off-diagonals scaled, the diagonal lifted."""
    row, col = _sym_columns(sym)
    v = np.asarray(sym.A2x if values is None else values, dtype=np.float64)
    lo, up = col == p, (row == p) & (col != p)
    other = np.concatenate([row[lo], col[up]])
    vals = np.concatenate([v[lo], v[up]])
    vals = np.where(other == p, vals + lift, scale * vals)
    ci = np.asarray(sym.Perm)[other]
    order = np.argsort(ci)
    return ci[order].astype(np.int32), np.ascontiguousarray(vals[order])


def _identity_values(sym, p):
    """The A2 values of P A P' with row and column p made the identity's."""
    row, col = _sym_columns(sym)
    v = np.array(sym.A2x, dtype=np.float64, copy=True)
    v[(row == p) | (col == p)] = 0.0
    v[(row == p) & (col == p)] = 1.0
    return v


def _rows(sym, few=False):
    """Rows (factor's ordering) to try: the first and last column of every supernode, column 70 of the wide ones, 0,
    n - 1 and the border row with the most branches of equal height below it.  few: 0, a leaf's last column, the first
    column of the middle supernode, row n / 2 and n - 1."""
    if few:
        return sorted({0, int(sym.super[1]) - 1, int(sym.super[sym.nsuper // 2]), sym.n // 2, sym.n - 1})
    rows = set(RR.rows_to_try(sym))
    best, most = None, 1
    for p in range(int(sym.super[sym.nsuper - 1]), sym.n):
        h = RR.reach_of(sym, p)[3]
        same = int(np.bincount(h).max()) if h.size else 0
        if same > most:
            best, most = p, same
    if best is not None:
        rows.add(best)
    return sorted(rows)


def _launch(plan, lv, call, values=None):
    """One device call on a copy of lv with a sentinel tail; the tail and the values of the column keep their bits."""
    import torch
    dL = _dev(np.concatenate([lv, np.full(_TAIL, _SENTINEL)]))
    d_cx = None if values is None else _dev(values)
    call(dL.data_ptr(), None if d_cx is None else d_cx.data_ptr())
    torch.cuda.synchronize()
    out = dL.cpu().numpy()
    assert (_bits(out[lv.size:]) == np.float64(_SENTINEL).view(np.int64)).all(), "the tail behind lValues was written"
    if d_cx is not None:
        assert np.array_equal(_bits(d_cx.cpu().numpy()), _bits(values)), "the values of the column were changed"
    return out[:lv.size].copy()


def _del(plan, sym, lv, p):
    k = int(sym.Perm[p])
    return _launch(plan, lv, lambda dL, _: plan.rowdel_device(dL, k))


def _add(plan, sym, lv, p, ci, cx):
    k = int(sym.Perm[p])
    return _launch(plan, lv, lambda dL, dc: plan.rowadd_device(dL, k, ci, dc), cx)


def _err(sym, lv1, want):
    row, col, off, _, _ = _entries(sym)
    return np.abs(lv1[off] - want[row, col]).max() / np.abs(want).max()


def _exact_identity(sym, lv1, p):
    row, col, off, _, _ = _entries(sym)
    at_row, at_col = (row == p) & (col < p), (col == p) & (row > p)
    zero = np.float64(0.0).view(np.int64)
    assert (_bits(lv1[off[at_row]]) == zero).all() and (_bits(lv1[off[at_col]]) == zero).all(), f"row / column {p} is not 0.0"
    assert lv1[off[(row == p) & (col == p)]][0] == 1.0, f"the diagonal of row {p} is not 1.0"


def _kept(sym, lv0, lv1, p, what):
    """Item 5: every stored entry outside may_write(p) and every strict upper triangle keeps its bits."""
    keep = ~RR.may_write(sym, p, _entries(sym))
    upper = _entries(sym)[4]
    keep[upper] = True
    moved = np.flatnonzero(_bits(lv0)[keep] != _bits(lv1)[keep])
    assert moved.size == 0, f"{what}: {moved.size} entries outside row {p}, column {p} and the path changed"


def _check_delete(case, lv0, lv1, p, what):
    sym = case["sym"]
    _exact_identity(sym, lv1, p)
    _kept(sym, lv0, lv1, p, what)
    if case["Sp"] is not None:
        err = _err(sym, lv1, np.linalg.cholesky(RR.identity_row(case["Sp"], p)))
    else:
        fb = RR.first_below(sym, p)
        if fb is None:
            return 0.0
        row, col, off, _, _ = _entries(sym)
        sn, fc = R.path_of(sym, [fb])
        C = np.concatenate([np.arange(int(f), int(sym.super[int(s) + 1])) for s, f in zip(sn, fc)])
        sel = np.isin(col, C)
        r, c, o = np.searchsorted(C, row[sel]), np.searchsorted(C, col[sel]), off[sel]
        L0 = np.zeros((C.size, C.size))
        L0[r, c] = lv0[o]
        w = np.zeros(sym.n)
        below = (col == p) & (row > p)
        w[row[below]] = lv0[off[below]]
        want = np.linalg.cholesky(L0 @ L0.T + np.outer(w[C], w[C]))
        err = np.abs(lv1[o] - want[r, c]).max() / np.abs(want).max()
    assert err <= FACTOR_TOL, f"{what}: max|L - cholesky| / max|L| = {err:.3e}"
    return err


# ---- 1. delete ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_delete_matches_dense_cholesky(api, name):
    case = _case(api, name)
    sym, plan, lv = case["sym"], case["plan"], case["lv"]
    worst = 0.0
    rows = _rows(sym, few=name not in SHAPES)
    for p in rows:
        lv1 = _del(plan, sym, lv, p)
        assert plan.rowmod_status() == 0
        worst = max(worst, _check_delete(case, lv, lv1, p, f"{name} row {p}"))
    print(f"ROWDEL_PARITY {name}: n={sym.n} rows={len(rows)} worst={worst:.3e}")


# ---- 2. add ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_add_matches_dense_cholesky_and_never_reads_what_it_overwrites(api, name):
    """From the factor of the values with row k made the identity's, and from the same buffer with random numbers over
    row p and column p: the same bits, and the factor of P A P'."""
    case = _case(api, name)
    sym, plan, lv = case["sym"], case["plan"], case["lv"]
    want = np.linalg.cholesky(case["Sp"]) if case["Sp"] is not None else None
    row, col, off, _, _ = _entries(sym)
    rng = np.random.default_rng(len(name))
    worst = 0.0
    rows = _rows(sym, few=name not in SHAPES)
    for p in rows:
        base, _ = plan.factor(_identity_values(sym, p))
        assert plan.status() == 0
        ci, cx = _column(sym, p)
        got = _add(plan, sym, base, p, ci, cx)
        assert plan.rowmod_status() == 0
        dirty = base.copy()
        mine = off[((row == p) & (col <= p)) | (col == p)]
        dirty[mine] = rng.standard_normal(mine.size)
        again = _add(plan, sym, dirty, p, ci, cx)
        assert np.array_equal(_bits(got), _bits(again)), f"{name} row {p}: the add read what stood in row / column p"
        _kept(sym, base, got, p, f"{name} row {p}")
        err = _err(sym, got, want) if want is not None else np.abs(got - lv).max() / np.abs(lv).max()
        worst = max(worst, err)
        assert err <= FACTOR_TOL, f"{name} row {p}: max|L - cholesky| / max|L| = {err:.3e}"
    print(f"ROWADD_PARITY {name}: n={sym.n} rows={len(rows)} worst={worst:.3e}")


# ---- 3. round trip --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES) + ["small3d", "random", "dense150"])
def test_round_trip_and_other_values(api, name):
    case = _case(api, name)
    sym, plan, lv, Sp = case["sym"], case["plan"], case["lv"], case["Sp"]
    worst = 0.0
    for p in _rows(sym, few=name not in SHAPES):
        gone = _del(plan, sym, lv, p)
        back = _add(plan, sym, gone, p, *_column(sym, p))
        assert plan.rowmod_status() == 0
        err = np.abs(back - lv).max() / np.abs(lv).max()
        assert err <= FACTOR_TOL, f"{name} row {p}: delete then add leaves max|L - L0| / max|L| = {err:.3e}"
        other = _add(plan, sym, gone, p, *_column(sym, p, scale=0.5, lift=1.0))
        assert plan.rowmod_status() == 0
        S2 = Sp.copy()
        S2[p, :] *= 0.5
        S2[:, p] *= 0.5
        S2[p, p] = Sp[p, p] + 1.0
        err2 = _err(sym, other, np.linalg.cholesky(S2))
        assert err2 <= FACTOR_TOL, f"{name} row {p}: other values, max|L - cholesky| / max|L| = {err2:.3e}"
        worst = max(worst, err, err2)
    print(f"ROWMOD_ROUND_TRIP {name}: worst={worst:.3e}")


# ---- 4. componentwise error, add only -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_componentwise_error_of_an_add_against_the_restatement(api, shape):
    """rho_factor (shape_cases.py, units of u) of the device's result against 4 x the same measure of rowadd_dense on the
    same input; the margin is the one updown has, for an equivalent order (partial sums per supernode) and fused
    multiply-adds.  Not for deletes: entries that a delete makes exactly zero come out as 1e-21 in the restatement itself.
    Measured on an MI355X: DESIGN.md, section 4."""
    case = _shaped(api, shape)
    sym, plan, Sp = case["sym"], case["plan"], case["Sp"]
    sup = np.asarray(sym.super)
    wide = int(np.argmax(np.diff(sup)))
    for p in sorted({int(sup[wide]) + min(70, int(sup[wide + 1] - sup[wide]) - 1), sym.n - 1}):
        base, _ = plan.factor(_identity_values(sym, p))
        got = _add(plan, sym, base, p, *_column(sym, p))
        assert plan.rowmod_status() == 0
        ref, bad = RR.rowadd_dense(I.bcsc_to_dense(sym, base), p, Sp[:, p])
        assert bad is None
        rho_ref = SC.rho_factor(Sp, ref)
        rho = SC.rho_factor(Sp, I.bcsc_to_dense(sym, got))
        print(f"ROWADD_RHO shape={shape} row={p} n={sym.n} rho={rho:.2f} restatement={rho_ref:.2f}")
        assert rho <= 4.0 * rho_ref, f"{shape} row {p}: rho_factor = {rho:.4g} > 4 x {rho_ref:.4g} (the restatement's)"


# ---- 5. what must not move, on values that are no factor ------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_random_values_outside_the_writable_set_keep_their_bits(api, shape):
    """lValues full of random numbers, the strict upper triangles of the diagonal blocks included: everything but row p
    in the panels of T(p), column p and the path's columns keeps its bits, and so do the tail and the column's values."""
    case = _shaped(api, shape)
    sym, plan = case["sym"], case["plan"]
    lv = np.random.default_rng(5).standard_normal(int(sym.xsize))
    for p in _rows(sym):
        gone = _del(plan, sym, lv, p)
        _kept(sym, lv, gone, p, f"{shape} delete {p}")
        _exact_identity(sym, gone, p)
        back = _add(plan, sym, lv, p, *_column(sym, p))
        _kept(sym, lv, back, p, f"{shape} add {p}")
        assert not np.array_equal(_bits(back), _bits(lv)), "the add changed nothing"


# ---- 6. failures ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small3d", "chain"])
def test_failed_adds_report_their_column_and_spread_nothing(api, name):
    case = _case(api, name)
    sym, plan, lv = case["sym"], case["plan"], case["lv"]
    Ld = I.bcsc_to_dense(sym, lv)
    p = next(q for q in RR.rows_to_try(sym)
             if RR.reach_of(sym, q)[0].size and RR.first_below(sym, q) is not None and np.abs(Ld[q, :q]).max() > 0.05)
    gone = _del(plan, sym, lv, p)
    ci, cx = _column(sym, p)
    at = int(np.flatnonzero(ci == int(sym.Perm[p]))[0])
    l12 = float(Ld[p, :p] @ Ld[p, :p])
    half = cx.copy()
    half[at] = 0.5 * l12                                # a22 - l12' l12 < 0: the add's own pivot
    bad = _add(plan, sym, gone, p, ci, half)
    assert plan.rowmod_status() == p + 1
    assert np.isfinite(bad).all(), "a failed pivot spread NaN or Inf"
    row, col, off, _, _ = _entries(sym)
    assert bad[off[(row == p) & (col == p)]][0] == 1.0 and not bad[off[(col == p) & (row > p)]].any()
    thin = cx.copy()
    thin[at] = l12 * (1.0 + 1e-9)                       # a tiny l22, a huge l32: the downdate behind it must fail
    bad = _add(plan, sym, gone, p, ci, thin)
    later = plan.rowmod_status()
    assert later > p + 1, f"status {later} after an add that leaves the matrix indefinite (row {p})"
    assert np.isfinite(bad).all(), "a failed downdate spread NaN or Inf"
    # the plan goes on: factor again, and a next row call is clean
    lv2, _ = plan.factor(sym.A2x)
    assert plan.status() == 0 and np.array_equal(lv2, lv)
    again = _add(plan, sym, _del(plan, sym, lv2, p), p, ci, cx)
    assert plan.rowmod_status() == 0
    assert np.abs(again - lv).max() <= FACTOR_TOL * np.abs(lv).max()


# ---- 7. the factor is usable ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small3d", "random"])
def test_modified_factor_solves_and_gives_the_logdet(api, name):
    """Plan.rowdel / Plan.rowadd (host buffers, the caller's ordering), then solve_spd against the dense modified matrix and
    logdet_device against the factor's diagonal, with the limits of test_updated_factor_solves_and_gives_the_logdet."""
    case = _named(api, name)
    sym, plan, lv = case["sym"], case["plan"], case["lv"]
    Ac = case["A"].to_dense()
    p = next(q for q in RR.rows_to_try(sym) if RR.reach_of(sym, q)[0].size and RR.first_below(sym, q) is not None)
    k = int(sym.Perm[p])
    gone, sec = plan.rowdel(lv, k)
    assert plan.rowmod_status() == 0 and sec >= 0.0 and not np.array_equal(gone, lv)
    column = Ac[:, k].copy()
    column *= 0.5
    column[k] = Ac[k, k] + 1.0
    back, sec = plan.rowadd(gone, k, column)
    assert plan.rowmod_status() == 0 and sec >= 0.0
    Anew = Ac.copy()
    Anew[k, :], Anew[:, k] = column, column
    B = np.random.default_rng(12).standard_normal((sym.n, 3))
    for lv1, M in ((gone, RR.identity_row(Ac, k)), (back, Anew)):
        X, _ = plan.solve_spd(lv1, B)
        res = np.abs(M @ X - B).max()
        assert res <= RESID_TOL * (np.abs(M).max() * np.abs(X).max() + np.abs(B).max()), res
        want = np.linalg.solve(M, B)
        assert np.abs(X - want).max() <= RESID_TOL * np.linalg.cond(M) * np.abs(want).max()
        ref = 2.0 * np.log(np.diag(I.bcsc_to_dense(sym, lv1))).sum()
        got, col = plan.logdet_device(_dev(lv1).data_ptr())
        assert col == 0 and abs(got - ref) <= 1e-12 * max(1.0, abs(ref))
        assert abs(got - np.linalg.slogdet(M)[1]) <= 1e-10 * max(1.0, abs(ref))
    # a dense vector and an (indices, values) pair: the same bits
    ci = np.flatnonzero(column).astype(np.int32)
    pair, _ = plan.rowadd(gone, k, (ci, column[ci]))
    assert np.array_equal(_bits(pair), _bits(back)) and not np.array_equal(back, gone)


# ---- 8. reproducible ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_two_runs_give_the_same_bits(api, shape):
    case = _shaped(api, shape)
    sym, plan, lv = case["sym"], case["plan"], case["lv"]
    for p in _rows(sym):
        a, b = _del(plan, sym, lv, p), _del(plan, sym, lv, p)
        assert np.array_equal(_bits(a), _bits(b)), f"{shape} row {p}: two deletes differ"
        ci, cx = _column(sym, p)
        c, d = _add(plan, sym, a, p, ci, cx), _add(plan, sym, a, p, ci, cx)
        assert plan.rowmod_status() == 0
        assert np.array_equal(_bits(c), _bits(d)), f"{shape} row {p}: two adds differ"


# ---- 9. info and no-ops ---------------------------------------------------------------------------------------------
def test_info_counters_and_no_ops(api):
    import torch
    case = _shaped(api, "chain")
    sym, lv = case["sym"], case["lv"]
    plan = api.Plan(sym, 0)
    plan.set_perm(np.asarray(sym.Perm))
    before = plan.info["device_bytes"]
    assert plan.rowmod_info["device_bytes"] == 0 and plan.rowmod_info["last_op"] == 0 and plan.rowmod_status() == 0
    updown_before = plan.updown_info
    for p in _rows(sym):
        sn, pos, ks, h = RR.reach_of(sym, p)
        got_sn, got_pos, got_h = plan.rowmod_reach(int(sym.Perm[p]))
        assert np.array_equal(got_sn, sn) and np.array_equal(got_pos, pos) and np.array_equal(got_h, h)
        heights = int(h.max()) + 1 if h.size else 0
        gone = _del(plan, sym, lv, p)
        info = plan.rowmod_info
        assert (info["last_op"], info["last_row"], info["reach_supernodes"], info["heights"]) == (1, p, sn.size, heights)
        assert info["row_launches"] == (1 if sn.size else 0) and info["column_launches"] == 1 and info["entries_read"] == 0
        fb = RR.first_below(sym, p)
        path = R.path_of(sym, [fb]) if fb is not None else (np.zeros(0), np.zeros(0))
        blocks = R.block_columns(sym, *path) if fb is not None else 0
        want_rot = (blocks + 1, 2 * blocks + 1) if fb is not None else (0, 0)
        assert want_rot[0] <= info["rotation_launches"] <= want_rot[1], (p, info, blocks)
        walked = sum(sum(R.panel(sym, int(s))[4] - (j - R.panel(sym, int(s))[0]) for j in range(int(f), int(sym.super[int(s) + 1])))
                     for s, f in zip(*path))
        assert info["entries_walked"] == walked
        _add(plan, sym, gone, p, *_column(sym, p))
        info = plan.rowmod_info
        assert (info["last_op"], info["last_row"], info["reach_supernodes"], info["heights"]) == (2, p, sn.size, heights)
        # per height a solve and at most a panel launch, and the clearing; nothing over an empty reach (row 0)
        assert (heights + 1 if sn.size else 0) <= info["row_launches"] <= (2 * heights + 1 if sn.size else 0), (p, info)
        assert info["column_launches"] == 1 and info["entries_read"] == RR.entries_read(sym, p)
        assert info["entries_walked"] == walked
        assert want_rot[0] <= info["rotation_launches"] <= want_rot[1], (p, info, blocks)
    assert RR.reach_of(sym, 0)[0].size == 0
    info = plan.rowmod_info
    assert info["device_bytes"] >= 8 * (int(sym.ssize) + sym.n) + 8 * (int(sym.ssize) + sym.n + 1)
    up = plan.updown_info
    assert {k: up[k] for k in up if k != "device_bytes"} == {k: updown_before[k] for k in up if k != "device_bytes"}
    assert up["device_bytes"] >= 8 * 8 * sym.n
    assert plan.info["device_bytes"] == before + info["device_bytes"] + up["device_bytes"]
    # a restricted plan refuses; the restriction lifted, it goes on
    p = sym.n - 1
    plan.set_active(np.ones(sym.nsuper, dtype=np.uint8))
    with pytest.raises(RuntimeError, match="parsy_factor_rowdel_device: plan is restricted by parsy_plan_set_active"):
        _del(plan, sym, lv, p)
    with pytest.raises(RuntimeError, match="parsy_factor_rowadd_device: plan is restricted by parsy_plan_set_active"):
        _add(plan, sym, lv, p, *_column(sym, p))
    plan.set_active(None)
    back = _add(plan, sym, _del(plan, sym, lv, p), p, *_column(sym, p))
    assert plan.rowmod_status() == 0 and np.abs(back - lv).max() <= FACTOR_TOL * np.abs(lv).max()
    torch.cuda.synchronize()
    plan.close()
