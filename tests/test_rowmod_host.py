"""Row delete / row add in the factor on the CPU tier: the row subtree a host-only plan finds (parsy_rowmod_reach) against
the restatement from the symbolic arrays (rowmod_ref.reach_of), the two dense restatements against numpy's Cholesky of
the modified matrix and inside the pattern of L, and every refusal by its message."""
import numpy as np
import pytest

import rowmod_ref as RR
import shape_cases as SC
import updown_ref as R
from conftest import problem
from test_updown_gpu import SHAPES

NAMES = ["tiny2d", "small3d", "edges", "wide", "chain"]
_CASES = {}


def _case(name):
    """(sym, P A P' dense, host-only plan under sym.Perm) per name."""
    if name not in _CASES:
        from parsy_bench_amd import api, inspector as I
        if name in SHAPES:
            spec = SHAPES[name]
            A, S = SC.arrow(spec["blocks"], spec["border"], spec["seed"], spec["chain"])
            sym = I.analyze(A, None, zrelax=SC.ZRELAX)
        else:
            A, _, sym = problem(name)
            S = A.to_dense()
        P = np.asarray(sym.Perm)
        plan = api.Plan(sym, -1)
        plan.set_perm(P)
        _CASES[name] = (sym, S[np.ix_(P, P)], plan)
    return _CASES[name]


@pytest.mark.parametrize("name", NAMES)
def test_reach_is_the_restated_one_on_every_row(name):
    sym, _, plan = _case(name)
    P = np.asarray(sym.Perm)
    tallest = 0
    for p in range(sym.n):
        sn, pos, h = plan.rowmod_reach(int(P[p]))
        want_sn, want_pos, want_ks, want_h = RR.reach_of(sym, p)
        assert sn.dtype == np.int32 and np.array_equal(sn, want_sn), (p, sn, want_sn)
        assert np.array_equal(pos, want_pos) and np.array_equal(h, want_h), (p, pos, want_pos, h, want_h)
        assert (np.diff(sn) > 0).all()
        own = int(sym.col2Sup[p])
        assert (own in sn.tolist()) == (p > int(sym.super[own])), "p's own supernode takes part unless p is its first column"
        # a subtree with p's own supernode on top: every other member's parent is a member, or is p's own supernode
        members = set(sn.tolist()) | {own}
        assert all(int(sym.sParent[int(s)]) in members for s in sn if int(s) != own), p
        for s, height in zip(sn, h):
            kids = [int(hh) for t, hh in zip(sn, h) if int(sym.sParent[int(t)]) == int(s) and int(t) != int(s)]
            assert int(height) == (1 + max(kids) if kids else 0), (p, int(s))
        tallest = max(tallest, int(h.max()) + 1 if h.size else 0)
    assert plan.rowmod_reach(int(P[0]))[0].size == 0, "row 0 of the factor's ordering has an empty reach"
    assert tallest >= (2 if name in ("small3d", "chain") else 1)


def test_reach_follows_the_plan_s_ordering():
    sym, _, plan = _case("small3d")
    p = sym.n - 1
    want = RR.reach_of(sym, p)[0]
    try:
        plan.set_perm(None)
        assert np.array_equal(plan.rowmod_reach(p)[0], want)        # identity: the row is taken as it is
    finally:
        plan.set_perm(np.asarray(sym.Perm))
    assert np.array_equal(plan.rowmod_reach(int(sym.Perm[p]))[0], want)


@pytest.mark.parametrize("name", NAMES)
def test_dense_restatements_against_cholesky(name):
    """Delete against cholesky of the matrix with the row made the identity's, add against cholesky of the matrix itself
    -- from the deleted factor and from the same with random numbers over row p and column p (the same bits) -- and both
    inside the pattern of L."""
    sym, Sp, _ = _case(name)
    L = np.linalg.cholesky(Sp)
    row, col, _, _, _ = R.entries(sym)
    pattern = np.zeros_like(Sp, dtype=bool)
    pattern[row, col] = True
    assert not L[~pattern].any()
    rows = RR.rows_to_try(sym)
    if len(rows) > 31:
        rows = rows[:: len(rows) // 30] + [sym.n - 1]
    rng = np.random.default_rng(len(name))
    worst = 0.0
    for p in rows:
        gone, bad = RR.rowdel_dense(L, p)
        assert bad is None and not gone[~pattern].any(), p
        want = np.linalg.cholesky(RR.identity_row(Sp, p))
        worst = max(worst, np.abs(gone - want).max() / np.abs(want).max())
        assert not gone[p, :p].any() and not gone[p + 1:, p].any() and gone[p, p] == 1.0
        back, bad = RR.rowadd_dense(gone, p, Sp[:, p])
        assert bad is None and not back[~pattern].any(), p
        worst = max(worst, np.abs(back - L).max() / np.abs(L).max())
        dirty = gone.copy()
        dirty[p, :p + 1] = rng.standard_normal(p + 1)
        dirty[p + 1:, p] = rng.standard_normal(sym.n - p - 1)
        again, bad = RR.rowadd_dense(dirty, p, Sp[:, p])
        assert bad is None and np.array_equal(again, back), f"row {p}: the add read what stood in row / column p"
    print(f"ROWMOD_RESTATEMENT {name}: rows={len(rows)} worst={worst:.3e}")
    assert worst <= 1e-13
    # a diagonal of half of l12' l12 fails at p itself
    p = sym.n - 1
    a = Sp[:, p].copy()
    a[p] = 0.5 * float(L[p, :p] @ L[p, :p])
    assert RR.rowadd_dense(RR.rowdel_dense(L, p)[0], p, a) == (None, p)


def test_writable_set_covers_what_the_restatement_changes():
    """rowmod_ref.may_write holds every stored entry that a delete or an add changes in the dense restatement."""
    sym, Sp, _ = _case("chain")
    L = np.linalg.cholesky(Sp)
    row, col, off, _, _ = R.entries(sym)
    for p in RR.rows_to_try(sym):
        gone, _ = RR.rowdel_dense(L, p)
        back, _ = RR.rowadd_dense(gone, p, 1.5 * Sp[:, p])
        mask = RR.may_write(sym, p)
        for a, b in ((L, gone), (gone, back)):
            changed = a[row, col] != b[row, col]
            assert mask[off[changed]].all(), p


def test_refusals_by_their_messages():
    """On a host-only plan: every refusal comes before the question of a device.  The pointers are never followed."""
    from parsy_bench_amd import _native as N
    sym, Sp, plan = _case("small3d")
    n = sym.n
    P = np.asarray(sym.Perm)
    lib = N.lib()
    lv = np.full(int(sym.xsize), 3.5)
    p = int(sym.super[0])                        # the first column of a leaf
    k = int(P[p])
    Sc = np.zeros_like(Sp)
    Sc[np.ix_(P, P)] = Sp
    ci, cx = RR.column_of(Sc, k)
    L, I_, X = lv.ctypes.data, ci.ctypes.data, cx.ctypes.data

    def both(stem, args, message):
        for name in (f"parsy_factor_{stem}_device", f"parsy_factor_{stem}_host"):
            assert getattr(lib, name)(plan._h, *args, None) == -1, (name, message)
            assert N.last_error() == f"{name}: {message}", N.last_error()

    both("rowdel", (None, k), "null argument")
    both("rowadd", (None, k, ci.size, I_, X), "null argument")
    both("rowadd", (L, k, ci.size, None, X), "null argument")
    both("rowadd", (L, k, ci.size, I_, None), "null argument")
    for bad in (-1, n):
        both("rowdel", (L, bad), f"row {bad} is out of range (n = {n})")
        both("rowadd", (L, bad, ci.size, I_, X), f"row {bad} is out of range (n = {n})")
        assert lib.parsy_rowmod_reach(plan._h, bad, None, None, None) == -1
        assert N.last_error() == f"parsy_rowmod_reach: row {bad} is out of range (n = {n})"
    both("rowadd", (L, k, -1, I_, X), "need nz >= 0")
    for bad in (-1, n):
        rows = np.array([bad], dtype=np.int32)
        both("rowadd", (L, k, 1, rows.ctypes.data, X), f"row index {bad} of the column is out of range (n = {n})")
    for pair in ([3, 3], [4, 3]):
        rows = np.array(pair, dtype=np.int32)
        both("rowadd", (L, k, 2, rows.ctypes.data, X), f"row indices of the column are unsorted or repeated (row {pair[1]})")
    off = ci[ci != k]
    both("rowadd", (L, k, off.size, off.ctypes.data, X), f"the column has no diagonal entry (row {k})")
    both("rowadd", (L, k, 0, I_, X), f"the column has no diagonal entry (row {k})")
    # the pattern rule, below and above the diagonal: the message names the row in both orderings
    inside = set(R.structure(sym, p).tolist())
    below = next(i for i in range(n - 1, p, -1) if i not in inside)
    q = n - 1
    above = next(i for i in range(q) if q not in set(R.structure(sym, i).tolist()))
    for at, outside in ((p, below), (q, above)):
        rows = np.array(sorted({int(P[at]), int(P[outside])}), dtype=np.int32)
        both("rowadd", (L, int(P[at]), 2, rows.ctypes.data, X),
             f"the column of row {int(P[at])} (row {at} of the factor's ordering) has a non-zero at row {int(P[outside])} "
             f"(row {outside} of the factor's ordering) outside the pattern of L; the pattern of L does not change")
    # a restricted plan, then a host-only plan
    plan.set_active(np.ones(sym.nsuper, dtype=np.uint8))
    try:
        for stem, args in (("rowdel", (L, k)), ("rowadd", (L, k, ci.size, I_, X))):
            name = f"parsy_factor_{stem}_device"
            assert getattr(lib, name)(plan._h, *args, None) == -1
            assert N.last_error() == f"{name}: plan is restricted by parsy_plan_set_active / _set_active_pieces"
    finally:
        plan.set_active(None)
    both("rowdel", (L, k), "plan was built without a device (device < 0)")
    both("rowadd", (L, k, ci.size, I_, X), "plan was built without a device (device < 0)")
    with pytest.raises(RuntimeError, match="parsy_factor_rowdel_host: plan was built without a device"):
        plan.rowdel(lv, k)
    with pytest.raises(RuntimeError, match="parsy_factor_rowadd_host: plan was built without a device"):
        plan.rowadd(lv, k, (ci, cx))
    with pytest.raises(RuntimeError, match="parsy_factor_rowadd_device: plan was built without a device"):
        plan.rowadd_device(lv.ctypes.data, k, ci, cx.ctypes.data)
    assert lib.parsy_rowmod_reach(None, 0, None, None, None) == -1
    assert lib.parsy_rowmod_get_info(plan._h, None) == -1
    assert (lv == 3.5).all()
    assert plan.rowmod_info == {"last_op": 0, "last_row": -1, "reach_supernodes": 0, "heights": 0, "row_launches": 0,
                                "column_launches": 0, "rotation_launches": 0, "entries_read": 0, "entries_walked": 0,
                                "device_bytes": 0}
    assert plan.info["device_bytes"] == 0
    assert plan.rowmod_status() == -1          # (as parsy_updown_status: no device, no status)
