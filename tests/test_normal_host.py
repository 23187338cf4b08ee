"""Normal matrices on the plan's pattern, CPU tier (host-only plans): parsy_normal_pattern against numpy, the pair lists of
a handle (counts, order, check), the sum restated from the lists against the dense F W F' within the derived limit
(normal_ref.py), every refusal with its message, and the grid generators restating the workloads' own matrices exactly."""
import ctypes as C

import numpy as np
import pytest

import normal_ref as R
from conftest import problem
from parsy_bench_amd import _native as N
from parsy_bench_amd.matrices import WORKLOADS, ColumnsCSC

_MADE = {}


def _small():
    """A ragged F (40 x 70): an empty column, an empty row, a single-entry column, columns of 1 .. 6 rows."""
    rng = np.random.default_rng(5)
    D = np.zeros((40, 70))
    for k in range(68):
        rows = rng.choice(39, size=int(rng.integers(1, 7)), replace=False)
        D[rows, k] = rng.uniform(0.25, 1.0, rows.size) * rng.choice([-1.0, 1.0], rows.size)
    D[7, 69] = -0.5
    return R.from_dense(D)


def _made(name):
    """(F, sym, host-only plan under sym.Perm, handle), made once."""
    if name not in _MADE:
        from parsy_bench_amd import api
        F = {"small": _small, "borders": lambda: R.borders()[0], "tall": R.tall, "wc": R.well_conditioned}[name]()
        sym = R.analysed(F, seed=len(name))
        plan = api.Plan(sym, -1)
        plan.set_perm(np.asarray(sym.Perm))
        plan._perm_set = True
        _MADE[name] = (F, sym, plan, api.NormalEquations(plan, F))
    return _MADE[name]


@pytest.mark.parametrize("name", ["small", "borders", "tall", "wc"])
def test_pattern_is_numpys(name):
    from parsy_bench_amd import api
    F = _made(name)[0]
    Ap, Ai = api.NormalEquations.pattern(F.n, F)
    want = R.pattern_lower(F.n, F)
    assert np.array_equal(Ap, want.Ap) and np.array_equal(Ai, want.Ai)
    # Ai == NULL: the count alone
    Ap2 = np.zeros(F.n + 1, dtype=np.int32)
    assert N.lib().parsy_normal_pattern(F.n, F.m, N.ptr(F.indptr), N.ptr(F.indices), N.ptr(Ap2), None) == Ai.size
    assert np.array_equal(Ap2, Ap)


@pytest.mark.parametrize("name", ["small", "borders", "tall", "wc"])
def test_info_and_check(name):
    F, sym, plan, ne = _made(name)
    info = ne.info
    c = np.diff(F.indptr).astype(np.int64)
    assert info["n"] == F.n and info["m"] == F.m and info["nnzF"] == F.indices.size
    assert info["pairs"] == int((c * (c + 1) // 2).sum())
    assert ne.check() == 0
    nnz = int(plan.info["nnzA"])
    lens = np.zeros(nnz, dtype=np.int64)
    col = R.column_of(F)
    inv = np.empty(F.n, dtype=np.int64)
    inv[np.asarray(sym.Perm)] = np.arange(F.n)
    pat = plan.pattern()
    for q in range(nnz):
        a, b, k = ne.pairs(q)
        lens[q] = k.size
        assert (np.diff(k) > 0).all(), f"list {q} is not ascending in k"
        assert (col[a] == k).all() and (col[b] == k).all()
        # orientation: a sits on the entry's row, b on its column, in the factor's ordering
        assert (inv[F.indices[a]] == pat["row"][q]).all() and (inv[F.indices[b]] == pat["col"][q]).all()
    assert lens.sum() == info["pairs"] and lens.max() == info["longest_list"]
    assert info["entries_untouched"] == int((lens == 0).sum())
    b = info["border"]
    assert b == [8, 64, 512]
    assert info["class_entries"] == [int((lens <= b[0]).sum()), int(((lens > b[0]) & (lens <= b[1])).sum()),
                                     int(((lens > b[1]) & (lens <= b[2])).sum())]
    assert info["chunked_entries"] == int((lens > 512).sum())
    assert info["chunks"] == int((-(-lens[lens > 512] // 512)).sum())
    assert info["launches"] == sum(1 for v in info["class_entries"] if v) + (2 if info["chunks"] else 0)
    assert info["device_bytes"] == 0
    if name == "borders":
        assert info["chunked_entries"] >= 3 and {7, 8, 9, 63, 64, 65, 511, 512, 513, 1025} <= set(lens.tolist())
    if name == "tall":
        assert info["pairs"] >= 45150


@pytest.mark.parametrize("name", ["small", "borders"])
def test_restated_sum_is_the_dense_matrix(name):
    """Under a random ordering (sym.Perm is one) the sum over pairs(q) is entry q of F W F' + beta I + A0: both
    orientations of an entry occur, and every one lands on the right A2 entry."""
    F, sym, plan, ne = _made(name)
    assert not np.array_equal(np.asarray(sym.Perm), np.arange(F.n))
    rng = np.random.default_rng(11)
    w = rng.uniform(-1.0, 1.0, F.m)
    w[::7] = 0.0
    nnz = int(plan.info["nnzA"])
    base = rng.standard_normal(nnz)
    got = R.restated_values(ne, F.data, w, beta=0.75, base=base)
    ci, cj = R.entry_coords(plan)
    assert (ci < cj).any() and (ci > cj).any(), "both orientations of an entry should occur in the caller's ordering"
    lens = np.array([ne.pairs(q)[2].size for q in range(nnz)])
    exact, limit = R.exact_values(F, F.data, w, 0.75, base, ci, cj, lens)
    worst = R.within(got, exact, limit)
    print(f"{name}: restated sum / limit = {worst:.3f}")
    assert worst <= 1.0


def _create(plan, m, Fp, Fi):
    h = N.lib().parsy_normal_create(plan._h if plan is not None else None, m, N.ptr(Fp), N.ptr(Fi))
    if h:
        N.lib().parsy_normal_destroy(h)
    return bool(h), N.last_error()


def test_refusals_of_create():
    F, sym, plan, _ = _made("small")
    Fp, Fi = F.indptr.copy(), F.indices.copy()
    ok, _ = _create(plan, F.m, Fp, Fi)
    assert ok
    for args, word in [((None, F.m, Fp, Fi), "null argument"), ((plan, F.m, None, Fi), "null argument"),
                       ((plan, F.m, Fp, None), "null argument"), ((plan, -1, Fp, Fi), "m >= 0")]:
        ok, msg = _create(*args)
        assert not ok and "parsy_normal_create" in msg and word in msg, msg
    bad = Fi.copy()
    bad[3] = F.n
    ok, msg = _create(plan, F.m, Fp, bad)
    assert not ok and f"row index {F.n}" in msg and "out of range" in msg, msg
    bad[3] = -1
    ok, msg = _create(plan, F.m, Fp, bad)
    assert not ok and "row index -1" in msg, msg
    k = int(np.flatnonzero(np.diff(Fp) >= 2)[0])
    swapped = Fi.copy()
    swapped[Fp[k]], swapped[Fp[k] + 1] = Fi[Fp[k] + 1], Fi[Fp[k]]
    ok, msg = _create(plan, F.m, Fp, swapped)
    assert not ok and f"column {k} of F are unsorted or repeated" in msg, msg
    rep = Fi.copy()
    rep[Fp[k] + 1] = rep[Fp[k]]
    ok, msg = _create(plan, F.m, Fp, rep)
    assert not ok and "unsorted or repeated" in msg, msg
    dec = Fp.copy()
    dec[5] = dec[6] + 1
    ok, msg = _create(plan, F.m, dec, Fi)
    assert not ok and "not decrease" in msg, msg
    # (nnzF beyond int32 cannot be stated through Fp's type; more than 2^31 - 1 chunks needs 2^40 triples)
    # m == 0 is a handle whose values are beta I + A0
    ok, msg = _create(plan, 0, np.zeros(1, np.int32), np.zeros(1, np.int32))
    assert ok, msg


def test_pattern_rule():
    """An F with a pair of rows that A's pattern does not hold is refused with the column and the rows in both orderings;
    the same F on a plan analysed from parsy_normal_pattern is accepted."""
    from parsy_bench_amd import api
    A, _, sym = problem("tiny2d")          # 5-point: (0, 13) (a diagonal neighbour) is no entry
    plan = api.Plan(sym, -1)
    P = np.asarray(sym.Perm)
    plan.set_perm(P)
    plan._perm_set = True
    inv = np.empty(sym.n, dtype=np.int64)
    inv[P] = np.arange(sym.n)
    Fp = np.array([0, 2, 4], np.int32)
    Fi = np.array([0, 1, 0, 13], np.int32)
    ok, msg = _create(plan, 2, Fp, Fi)
    assert not ok and "column 1 of F holds rows" in msg, msg
    assert " 0" in msg and " 13" in msg and f"{inv[0]}" in msg and f"{inv[13]}" in msg, msg
    assert "pattern of A does not change" in msg
    with pytest.raises(RuntimeError, match="column 1 of F"):
        api.NormalEquations(plan, (Fp, Fi, np.ones(4)))
    F = ColumnsCSC(sym.n, 2, Fp, Fi, np.ones(4))
    sym2 = R.analysed(F, seed=3)
    ne = api.NormalEquations(api.Plan(sym2, -1), F)
    assert ne.check() == 0 and ne.info["pairs"] == 6
    # a row of F whose diagonal is missing cannot happen on a plan of this library (A's diagonal is full); a later
    # set_perm does not move a handle
    before = [ne.pairs(q) for q in range(int(ne.plan.info["nnzA"]))]
    ne.plan.set_perm(None)
    after = [ne.pairs(q) for q in range(int(ne.plan.info["nnzA"]))]
    assert all(np.array_equal(x, y) for b4, af in zip(before, after) for x, y in zip(b4, af)) and ne.check() == 0


def test_device_calls_refuse_a_host_only_plan():
    F, sym, plan, ne = _made("small")
    with pytest.raises(RuntimeError, match="without a device"):
        ne.values()
    with pytest.raises(RuntimeError, match="without a device"):
        ne.apply("F", np.ones(F.m))
    with pytest.raises(RuntimeError, match="without a device"):
        ne.lstsq(np.zeros(int(sym.xsize)), np.ones(F.m))
    assert ne.info["device_bytes"] == 0
    assert N.lib().parsy_normal_pairs(ne._h, -1, None, None, None) == -1
    assert N.lib().parsy_normal_pairs(ne._h, int(plan.info["nnzA"]), None, None, None) == -1
    assert N.lib().parsy_normal_check(None) == -1
    assert N.lib().parsy_normal_get_info(ne._h, None) == -1


@pytest.mark.parametrize("name", ["tiny2d", "small3d"])
def test_grid_edges_restate_the_grid_matrix_exactly(name):
    """grid_edges with w = 1 and beta = shift is the 5- / 7-point matrix of the grid, bit for bit: on tiny2d the
    workload's own A2x; on small3d (a 27-point workload) the 7-point matrix of the same grid on the workload's
    pattern, zero where the 27-point pattern has entries the 7-point one lacks."""
    from parsy_bench_amd import api, matrices as M
    A, _, sym = problem(name)
    nx, ny, nz, stencil, shift = WORKLOADS[name]
    plan = api.Plan(sym, -1)
    ne = api.NormalEquations(plan, M.grid_edges(nx, ny, nz))
    assert ne.check() == 0
    got = R.restated_values(ne, ne.fx, None, beta=shift)
    if stencil == 5:
        assert ne.info["entries_untouched"] == 0
        assert np.array_equal(got, np.asarray(sym.A2x))
    else:
        G = M.grid_spd(nx, ny, nz, 7, shift).to_dense()
        ci, cj = R.entry_coords(plan)
        assert np.array_equal(got, G[ci, cj])
        assert ne.info["entries_untouched"] == int((G[ci, cj] == 0).sum()) > 0
    # w = 1 given explicitly: the same bits
    assert np.array_equal(R.restated_values(ne, ne.fx, np.ones(ne.m), beta=shift), got)


def test_grid_cells_have_the_27_point_pattern():
    from parsy_bench_amd import api, matrices as M
    A, _, sym = problem("small3d")
    nx, ny, nz, stencil, shift = WORKLOADS["small3d"]
    assert stencil == 27
    F = M.grid_cells(nx, ny, nz)
    assert F.m == (nx - 1) * (ny - 1) * (nz - 1) and (np.diff(F.indptr) == 8).all() and (F.data == 1.0).all()
    Ap, Ai = api.NormalEquations.pattern(F.n, F)
    assert np.array_equal(Ap, A.Ap) and np.array_equal(Ai, A.Ai)
    ne = api.NormalEquations(api.Plan(sym, -1), F)
    assert ne.info["entries_untouched"] == 0 and ne.check() == 0
    # 2-D: four ones per column, the 9-point pattern
    F2 = M.grid_cells(7, 5)
    A9 = M.grid_spd(7, 5, 1, 9, 0.1)
    Ap, Ai = api.NormalEquations.pattern(F2.n, F2)
    assert (np.diff(F2.indptr) == 4).all() and np.array_equal(Ap, A9.Ap) and np.array_equal(Ai, A9.Ai)
