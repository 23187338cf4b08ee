"""Update / downdate of the factor on the CPU tier: the path a host-only plan finds for a W (parsy_updown_path) against a
numpy restatement from sym.sParent / sym.col2Sup, the pattern rule, every refusal of the arguments, and the refusal of the
device and host-buffer calls on a host-only plan."""
import numpy as np
import pytest

import shape_cases as SC
import updown_ref as R
from test_selinv_host import sym_of

NAMES = ["tiny2d", "small3d", "ex15", "lap30", "dense150", "tridiag300", "diag37"]
_PLANS = {}


def _plan(name):
    """(sym, host-only plan under sym.Perm) per name."""
    if name not in _PLANS:
        from parsy_bench_amd import api
        sym = sym_of(name)
        plan = api.Plan(sym, -1)
        plan.set_perm(np.asarray(sym.Perm))
        _PLANS[name] = (sym, plan)
    return _PLANS[name]


def _leaf_columns(sym):
    """The first column of every supernode without children, ascending."""
    has_child = np.zeros(sym.nsuper, dtype=bool)
    par = np.asarray(sym.sParent)
    has_child[par[(par >= 0) & (par < sym.nsuper) & (par != np.arange(sym.nsuper))]] = True
    return [int(sym.super[s]) for s in np.flatnonzero(~has_child)]


def _check_path(sym, plan, starts, Wp=None, seed=0):
    """The plan's path of an admissible W with these start columns (factor's ordering) is the restated one."""
    Wp = R.admissible_w(sym, starts, seed) if Wp is None else Wp
    sn, fc = plan.updown_path(R.to_caller(sym, Wp))
    want_sn, want_fc = R.path_of(sym, [j for t, j in enumerate(starts) if Wp[:, t].any()])
    assert sn.dtype == np.int32 and np.array_equal(sn, want_sn), (starts, sn, want_sn)
    assert np.array_equal(fc, want_fc), (starts, fc, want_fc)
    return sn, fc


@pytest.mark.parametrize("name", NAMES)
def test_path_is_the_restated_one(name):
    sym, plan = _plan(name)
    n = sym.n
    leaves = _leaf_columns(sym)
    rng = np.random.default_rng(len(name))
    # a start at column 0 and at column n - 1 (a root: the path is that supernode alone, entered at its last column)
    sn, fc = _check_path(sym, plan, [0])
    assert sn[0] == sym.col2Sup[0] and fc[0] == 0
    sn, fc = _check_path(sym, plan, [n - 1])
    assert sn.tolist() == [sym.nsuper - 1] and fc.tolist() == [n - 1]
    # every leaf by itself (up to 8 of them), and random columns
    for j in leaves[:8] + rng.integers(0, n, 6).tolist():
        sn, fc = _check_path(sym, plan, [int(j)], seed=int(j))
        assert (np.diff(sn) > 0).all() and sn[0] == sym.col2Sup[int(j)] and fc[0] == j
    # two columns whose paths merge (two leaves, where there are two), two with the same start, and 17 columns
    if len(leaves) >= 2:
        a, b = leaves[0], leaves[-1]
        sn, _ = _check_path(sym, plan, [a, b])
        assert set(sn) == set(R.path_of(sym, [a])[0]) | set(R.path_of(sym, [b])[0])
    _check_path(sym, plan, [leaves[0], leaves[0]])
    _check_path(sym, plan, sorted(rng.integers(0, n, 17).tolist(), reverse=True), seed=17)
    # an empty column among the others adds nothing; k = 0 and an all-zero W have no path
    Wp = R.admissible_w(sym, [leaves[0], 0, n - 1], 3)
    Wp[:, 1] = 0.0
    _check_path(sym, plan, [leaves[0], 0, n - 1], Wp=Wp)
    for W in (np.zeros((n, 0)), np.zeros((n, 3)), (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))):
        sn, fc = plan.updown_path(W)
        assert sn.size == 0 and fc.size == 0


def test_path_under_the_identity_and_after_the_ordering_changes():
    """Rows of W go through the plan's ordering as it is set: the same W means other columns of L under another one."""
    sym, plan = _plan("small3d")
    Wp = R.admissible_w(sym, [5], 1)
    try:
        plan.set_perm(None)
        sn, fc = plan.updown_path(Wp)                      # identity: W is taken as it is
        want = R.path_of(sym, [5])
        assert np.array_equal(sn, want[0]) and np.array_equal(fc, want[1])
    finally:
        plan.set_perm(np.asarray(sym.Perm))
    sn, fc = plan.updown_path(R.to_caller(sym, Wp))
    assert np.array_equal(sn, want[0]) and np.array_equal(fc, want[1])


def test_entry_column_of_a_wide_supernode():
    """An arrow matrix: a 130-wide block entered at its column 70 starts in its second block column; the border is entered
    at the first of the block's rows below."""
    A, S = SC.arrow(((130, 40), (16, 9)), 60, seed=21)
    from parsy_bench_amd import api, inspector as I
    sym = I.analyze(A, None, zrelax=SC.ZRELAX)
    assert SC.supernodes_of(sym) == [(130, 170), (16, 25), (60, 60)]
    plan = api.Plan(sym, -1)
    sn, fc = plan.updown_path(R.admissible_w(sym, [70], 2))
    first_below = int(sym.s[int(sym.i_ptr[0]) + 130])
    assert sn.tolist() == [0, 2] and fc.tolist() == [70, first_below] and first_below >= 146
    assert R.block_columns(sym, sn, fc) == 2 + 1      # columns 64 .. 129 of the block, and the border
    sn, fc = plan.updown_path(R.admissible_w(sym, [3, 140], 2))     # two branches that merge at the border
    assert sn.tolist() == [0, 1, 2] and fc[:2].tolist() == [3, 140]
    assert fc[2] == min(first_below, int(sym.s[int(sym.i_ptr[130]) + 16]))


def test_pattern_rule_names_the_column_and_the_row():
    sym, plan = _plan("small3d")
    leaf = _leaf_columns(sym)[0]
    inside = set(R.structure(sym, leaf).tolist())
    outside = next(i for i in range(sym.n - 1, leaf, -1) if i not in inside)
    Wp = R.admissible_w(sym, [sym.n - 1, leaf], 4)
    Wp[outside, 1] = 0.5
    Wc = R.to_caller(sym, Wp)
    row = int(np.asarray(sym.Perm)[outside])
    msg = (rf"parsy_updown_path: column 1 of W has a non-zero at row {row} \(row {outside} of the factor's ordering\) "
           rf"outside the structure of column {leaf} of L")
    with pytest.raises(RuntimeError, match=msg):
        plan.updown_path(Wc)
    # ... and a row ABOVE nothing: the smallest row is the start column by definition, so a W of one entry always passes
    one = np.zeros(sym.n)
    one[row] = 1.0
    assert plan.updown_path(one)[1][0] == outside
    # the device and host-buffer calls refuse it with the same words before they ask for a device
    lv = np.zeros(int(sym.xsize))
    with pytest.raises(RuntimeError, match=msg.replace("parsy_updown_path", "parsy_factor_updown_host")):
        plan.updown(lv, Wc)
    wp, wi, wx = plan._w_csc(Wc, sym.n)
    with pytest.raises(RuntimeError, match=msg.replace("parsy_updown_path", "parsy_factor_updown_device")):
        plan.updown_device(lv.ctypes.data, wp, wi, wx.ctypes.data)


def test_argument_refusals():
    """Each by its message, on a host-only plan: they come before the question of a device.  The pointers are never
    followed (host arrays stand in for the device ones)."""
    from parsy_bench_amd import _native as N
    sym, plan = _plan("tiny2d")
    n = sym.n
    lib = N.lib()
    lv = np.zeros(int(sym.xsize))
    wp = np.array([0, 1], dtype=np.int32)
    wi = np.array([int(np.asarray(sym.Perm)[n - 1])], dtype=np.int32)
    wx = np.ones(1)
    L, P, I_, X = lv.ctypes.data, wp.ctypes.data, wi.ctypes.data, wx.ctypes.data

    def both(args, message):
        for name in ("parsy_factor_updown_device", "parsy_factor_updown_host"):
            assert getattr(lib, name)(plan._h, *args, None) == -1, (name, message)
            assert N.last_error() == f"{name}: {message}", N.last_error()

    both((None, 1, 1, P, I_, X), "null argument")
    both((L, 1, 1, None, I_, X), "null argument")
    both((L, 1, 1, P, None, X), "null argument")
    both((L, 1, 1, P, I_, None), "null argument")
    both((L, 0, 1, P, I_, X), "sign must be +1 (update) or -1 (downdate)")
    both((L, 2, 1, P, I_, X), "sign must be +1 (update) or -1 (downdate)")
    both((L, 1, -1, P, I_, X), "need k >= 0")
    for bad in (-1, n):
        rows = np.array([bad], dtype=np.int32)
        both((L, 1, 1, P, rows.ctypes.data, X), f"row index {bad} of column 0 of W is out of range (n = {n})")
    wp2, two = np.array([0, 0, 2], dtype=np.int32), np.ones(2)
    for pair in ([3, 3], [4, 3]):
        rows = np.array(pair, dtype=np.int32)
        both((L, -1, 2, wp2.ctypes.data, rows.ctypes.data, two.ctypes.data),
             f"row indices of column 1 of W are unsorted or repeated (row {pair[1]})")
    down = np.array([1, 0], dtype=np.int32)
    both((L, 1, 1, down.ctypes.data, I_, X), "column pointers of W must start at 0 or above and not decrease")
    rows = np.array([n], dtype=np.int32)
    assert lib.parsy_updown_path(plan._h, 1, P, rows.ctypes.data, None, None) == -1
    assert N.last_error() == f"parsy_updown_path: row index {n} of column 0 of W is out of range (n = {n})"
    assert lib.parsy_updown_path(None, 0, None, None, None, None) == -1
    assert lib.parsy_updown_get_info(plan._h, None) == -1
    assert not lv.any() and wx[0] == 1.0


def test_host_only_plan_refuses_the_device_and_host_calls():
    from parsy_bench_amd import _native as N
    sym, plan = _plan("tiny2d")
    n = sym.n
    lv = np.full(int(sym.xsize), 3.5)
    W = R.to_caller(sym, R.admissible_w(sym, [0, n - 1], 5))
    with pytest.raises(RuntimeError, match=r"parsy_factor_updown_host: plan was built without a device"):
        plan.updown(lv, W)
    wp, wi, wx = plan._w_csc(W, n)
    for sign in (+1, -1):
        with pytest.raises(RuntimeError, match=r"parsy_factor_updown_device: plan was built without a device"):
            plan.updown_device(lv.ctypes.data, wp, wi, wx.ctypes.data, sign=sign)
    # k = 0 is a no-op everywhere else; here the plan still has no device to do nothing on
    with pytest.raises(RuntimeError, match="without a device"):
        plan.updown(lv, np.zeros((n, 0)))
    assert "without a device" in N.last_error()
    assert (lv == 3.5).all()
    info = plan.updown_info
    assert info == {"path_supernodes": 0, "last_launches": 0, "last_k": 0, "last_sign": 0, "block_columns": 0,
                    "entries_touched": 0, "device_bytes": 0}
    assert plan.info["device_bytes"] == 0
    assert plan.updown_status() == -1          # (as parsy_factor_status: no device, no status)


def test_dense_restatement_on_arrow_matrices():
    """The reference itself: on arrow matrices an admissible W never takes the rotations outside the pattern of L, the
    result is the Cholesky factor of S + W W' / S - W W' to rounding, and a downdate that leaves the matrix indefinite
    names its column."""
    for blocks, border, chain, seed in ((((17, 9), (33, 30), (5, 1)), 40, False, 1), (((17, 20), (33, 30), (20, 25)), 50, True, 2)):
        A, S = SC.arrow(blocks, border, seed, chain)
        from parsy_bench_amd import inspector as I
        sym = I.analyze(A, None, zrelax=SC.ZRELAX)
        P = np.asarray(sym.Perm)
        S = S[np.ix_(P, P)]
        L = np.linalg.cholesky(S)
        pattern = np.zeros_like(S, dtype=bool)
        row, col, _, _, _ = R.entries(sym)
        pattern[row, col] = True
        assert not L[~pattern].any()
        starts = [0, 16, 20, int(sym.super[-2]) - 1, sym.n - 1, 3, 40, 17, 2]
        W = R.admissible_w(sym, starts, seed)
        up, bad = R.updown_dense(L, W, +1)
        assert bad is None and not up[~pattern].any()
        want = np.linalg.cholesky(S + W @ W.T)
        assert np.abs(up - want).max() <= 1e-13 * np.abs(want).max()
        down, bad = R.updown_dense(up, 0.5 * W, -1)
        assert bad is None and not down[~pattern].any()
        want = np.linalg.cholesky(S + 0.75 * W @ W.T)
        assert np.abs(down - want).max() <= 1e-13 * np.abs(want).max()
        e = np.zeros((sym.n, 1))
        e[7, 0] = 1.5 * L[7, 7]
        assert R.updown_dense(L, e, -1) == (None, 7)
