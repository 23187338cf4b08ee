"""Gradients with respect to A's values on the CPU tier: the pattern of A as a host-only plan reports it
(parsy_plan_pattern) against the inspector's A2 arrays and a numpy restatement of the scatter offsets, the entry counts
of parsy_grad_get_info, and the refusal of every device call on a host-only plan."""
import numpy as np
import pytest

from test_selinv_host import EDGES, sym_of

NAMES = ["tiny2d", "small3d", "mid3d", "ex15", "lap30"] + EDGES


@pytest.fixture(scope="module")
def plans():
    from parsy_bench_amd import api
    cache = {}

    def get(name):
        if name not in cache:
            sym = sym_of(name)
            cache[name] = (api.Plan(sym, -1), sym)
        return cache[name]
    return get


def scatter_offsets(sym):
    """Where the factorization puts every A2 entry: p[c] + the position of its row in the supernode's row list."""
    n = sym.n
    col = np.repeat(np.arange(n), np.diff(sym.A2p))
    dst = np.empty(int(sym.nnzA), dtype=np.int64)
    for s in range(sym.nsuper):
        c0, c1 = int(sym.super[s]), int(sym.super[s + 1])
        rows = sym.s[int(sym.i_ptr[c0]):int(sym.i_ptr[c1])]
        q0, q1 = int(sym.A2p[c0]), int(sym.A2p[c1])
        pos = np.searchsorted(rows, sym.A2i[q0:q1])
        assert (rows[pos] == sym.A2i[q0:q1]).all()
        dst[q0:q1] = sym.p[col[q0:q1]].astype(np.int64) + pos
    return col, dst


@pytest.mark.parametrize("name", NAMES)
def test_pattern_matches_the_inspector(plans, name):
    plan, sym = plans(name)
    pat = plan.pattern()
    col, dst = scatter_offsets(sym)
    assert pat["row"].dtype == np.int32 and pat["col"].dtype == np.int32 and pat["dst"].dtype == np.int64
    assert np.array_equal(pat["row"], sym.A2i)
    assert np.array_equal(pat["col"], col)
    assert np.array_equal(pat["dst"], dst)
    assert (pat["row"] >= pat["col"]).all()


@pytest.mark.parametrize("name", NAMES)
def test_entry_counts(plans, name):
    from parsy_bench_amd import _native as N
    plan, sym = plans(name)
    info = plan.grad_info
    assert info["entries"] == int(sym.nnzA)
    assert info["offdiag_entries"] == int(sym.nnzA) - sym.n   # every diagonal entry of an SPD matrix is stored
    assert info["device_bytes"] == 0 and info["last_lanes"] == 0
    # any output may be left out; the count comes back alone
    assert int(N.lib().parsy_plan_pattern(plan._h, None, None, None)) == int(sym.nnzA)
    row = np.zeros(int(sym.nnzA), dtype=np.int32)
    assert int(N.lib().parsy_plan_pattern(plan._h, N.ptr(row), None, None)) == int(sym.nnzA)
    assert np.array_equal(row, sym.A2i)


def test_diag37_has_no_offdiagonal_entry(plans):
    plan, sym = plans("diag37")
    assert plan.grad_info["offdiag_entries"] == 0 and plan.grad_info["entries"] == 37


@pytest.mark.parametrize("name", ["tiny2d", "ex15"])
def test_a2src_addresses_the_callers_entry(name):
    """Entry q of A2 at permuted (i, j) is the caller's entry A2src[q] at (max, min) of (Perm[i], Perm[j]): what the
    PyTorch layer's index_select / index_copy_ with A2src rely on."""
    from conftest import problem
    A, _, sym = problem(name)
    assert int(sym.nnzA) == len(A.Ax)
    assert np.array_equal(np.sort(sym.A2src), np.arange(len(A.Ax)))
    ccol = np.repeat(np.arange(A.n), np.diff(A.Ap))
    i, j = sym.Perm[sym.A2i], sym.Perm[np.repeat(np.arange(sym.n), np.diff(sym.A2p))]
    assert np.array_equal(A.Ai[sym.A2src], np.maximum(i, j))
    assert np.array_equal(ccol[sym.A2src], np.minimum(i, j))


def test_host_only_plan_refuses_device_calls(plans):
    plan, sym = plans("ex15")
    n, nnz = sym.n, int(sym.nnzA)
    with pytest.raises(RuntimeError, match="parsy_pattern_outer_device.*without a device"):
        plan.pattern_outer_device(8, n, 8, n, 1, 8)
    with pytest.raises(RuntimeError, match="parsy_inverse_pattern_device.*without a device"):
        plan.inverse_pattern_device(8, 8)
    with pytest.raises(RuntimeError, match="parsy_trace_inverse_device.*without a device"):
        plan.trace_inverse_device(8, 8, nnz, 1)
    with pytest.raises(RuntimeError, match="parsy_pattern_outer_host.*without a device"):
        plan.pattern_outer(np.zeros(n), np.zeros(n))
    with pytest.raises(RuntimeError, match="parsy_inverse_pattern_host.*without a device"):
        plan.inverse_pattern(np.zeros(int(sym.xsize)))
    info = plan.grad_info
    assert info["device_bytes"] == 0 and info["last_lanes"] == 0
