"""The factor as an operator, host side: the transpose of the row lists (parsy_factor_apply_row_index) against a numpy
restatement, parsy_factor_apply_get_info, and the refusal of the device and host-buffer calls on a host-only plan."""
import numpy as np
import pytest

from test_selinv_host import sym_of

NAMES = ["tiny2d", "small3d", "ex15", "lap30", "dense150", "tridiag300", "diag37"]
_PLANS = {}


def _plan(name):
    if name not in _PLANS:
        from parsy_bench_amd import api
        sym = sym_of(name)
        _PLANS[name] = (sym, api.Plan(sym, -1))
    return _PLANS[name]


def _restated_index(sym):
    """For each row the indices k with sym.s[k] == row, ascending: (ptr, pos)."""
    s = np.asarray(sym.s[:int(sym.ssize)], dtype=np.int64)
    pos = np.argsort(s, kind="stable").astype(np.int64)   # (stable: ascending k within a row)
    counts = np.bincount(s, minlength=sym.n).astype(np.int64)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), pos


@pytest.mark.parametrize("name", NAMES)
def test_row_index_is_the_transpose_of_the_row_lists(name):
    sym, plan = _plan(name)
    ptr, pos = plan.apply_row_index()
    want_ptr, want_pos = _restated_index(sym)
    assert ptr.dtype == np.int64 and pos.dtype == np.int64
    assert np.array_equal(ptr, want_ptr)
    assert np.array_equal(pos, want_pos)
    # ... which is what the definition says, row by row
    s = np.asarray(sym.s[:int(sym.ssize)])
    for row in (0, sym.n // 2, sym.n - 1):
        assert np.array_equal(pos[ptr[row]:ptr[row + 1]], np.flatnonzero(s == row))


@pytest.mark.parametrize("name", NAMES)
def test_apply_info_of_a_host_only_plan(name):
    sym, plan = _plan(name)
    info = plan.apply_info
    ptr, _ = _restated_index(sym)
    assert info["rows"] == sym.n
    assert info["occurrences"] == int(sym.ssize)
    assert info["max_occurrences"] == int(np.diff(ptr).max())
    assert info["block_columns"] >= 1
    assert info["workspace_bytes"] >= 8 * int(sym.ssize)   # one column of T has a row per entry of the row lists
    assert info["device_bytes"] == 0
    assert info["last_op"] == -1 and info["last_launches"] == 0


def test_max_occurrences_of_the_named_patterns():
    """Computed here from the symbolic arrays: a row of tiny2d appears in at most 5 panels, one of lap30 in 20."""
    for name, want in (("tiny2d", 5), ("lap30", 20)):
        sym, plan = _plan(name)
        assert int(np.bincount(np.asarray(sym.s[:int(sym.ssize)]), minlength=sym.n).max()) == want
        assert plan.apply_info["max_occurrences"] == want


@pytest.mark.parametrize("op", [0, 1, 2, 3])
def test_host_only_plan_refuses_the_device_and_host_calls(op):
    from parsy_bench_amd import _native as N
    sym, plan = _plan("tiny2d")
    n = sym.n
    lv = np.zeros(int(sym.xsize))
    x = np.ones((n, 2), order="F")
    y = np.full((n, 2), 3.5, order="F")
    with pytest.raises(RuntimeError, match=r"parsy_factor_apply_host: plan was built without a device"):
        plan.factor_apply(lv, x, op, y=y, beta=1.0)
    # the device call: the pointers are never followed (host arrays stand in for them)
    with pytest.raises(RuntimeError, match=r"parsy_factor_apply_device: plan was built without a device"):
        plan.factor_apply_device(lv.ctypes.data, op, x.ctypes.data, n, 2, y.ctypes.data, n)
    assert (y == 3.5).all() and (x == 1.0).all()
    assert plan.apply_info["device_bytes"] == 0
    with pytest.raises(RuntimeError, match="without a device"):
        plan.sample(lv, np.ones(n))
    assert "without a device" in N.last_error()
