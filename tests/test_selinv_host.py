"""Selected inversion and log-determinant on the CPU tier: the schedule a host-only plan builds (block-column tree,
levels, gather map, path split) against the test suite's own numpy restatement from the symbolic arrays, and the
refusal of the device calls on a host-only plan."""
import numpy as np
import pytest

from conftest import problem

NAMED = ["tiny2d", "small3d", "mid3d", "ex15", "lap30", "nd24k"]
EDGES = ["dense150", "tridiag300", "diag37"]
_EDGE = {}


def lower_csc(D):
    """LowerCSC of the lower triangle of the dense symmetric D."""
    from parsy_bench_amd import matrices as M
    n = D.shape[0]
    Ap, Ai, Ax = [0], [], []
    for j in range(n):
        rows = np.nonzero(D[j:, j])[0] + j
        Ai.extend(rows.tolist())
        Ax.extend(D[rows, j].tolist())
        Ap.append(len(Ai))
    return M.LowerCSC(n, np.array(Ap, np.int32), np.array(Ai, np.int32), np.array(Ax, np.float64))


def edge(name):
    """(A, sym) of an edge pattern in natural order: a dense 150 x 150 SPD matrix (one supernode of three block columns,
    the last 22 wide), a tridiagonal matrix of order 300 (its etree is a chain), a diagonal matrix of order 37."""
    if name not in _EDGE:
        from parsy_bench_amd import inspector as I
        rng = np.random.default_rng(7)
        if name == "dense150":
            B = rng.standard_normal((150, 150))
            D = B @ B.T / 150 + np.eye(150)
        elif name == "tridiag300":
            n = 300
            D = np.diag(np.full(n, 2.5)) + np.diag(np.full(n - 1, -1.0), 1) + np.diag(np.full(n - 1, -1.0), -1)
        else:
            D = np.diag(rng.uniform(0.5, 3.0, 37))
        A = lower_csc(D)
        _EDGE[name] = (A, I.analyze(A, np.arange(A.n, dtype=np.int32)))
    return _EDGE[name]


def sym_of(name):
    return edge(name)[1] if name in EDGES else problem(name)[2]


def block_columns(sym):
    """(supernode, first column in it, width, |R_b|) of every block column, in supernode order."""
    out = []
    for s in range(sym.nsuper):
        c0, c1 = int(sym.super[s]), int(sym.super[s + 1])
        w, r = c1 - c0, int(sym.i_ptr[c1] - sym.i_ptr[c0])
        for j0 in range(0, w, 64):
            wb = min(64, w - j0)
            out.append((s, j0, wb, r - j0 - wb))
    return out


def nominal_flops(sym):
    return sum(2.0 * m * m * wb + 4.0 * m * wb * wb for _, _, wb, m in block_columns(sym))


def tree_levels(sym):
    """Depth of the block-column tree (levels from the root): the parent of a block column is the next one of its
    supernode, or the first one of the supernode's etree parent."""
    nb = [-(-(int(sym.super[s + 1]) - int(sym.super[s])) // 64) for s in range(sym.nsuper)]
    dlast = {}

    def last_depth(s):
        chain = []
        while s >= 0 and s not in dlast:
            chain.append(s)
            s = int(sym.sParent[s])
        for u in reversed(chain):
            p = int(sym.sParent[u])
            dlast[u] = 0 if p < 0 else dlast[p] + nb[p]
        return dlast[chain[0]] if chain else dlast[s]

    return max(last_depth(s) + nb[s] - 1 for s in range(sym.nsuper)) + 1


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


@pytest.mark.parametrize("name", NAMED + EDGES)
def test_schedule_checks_and_counts(plans, name):
    from parsy_bench_amd import _native as N
    plan, sym = plans(name)
    assert plan.selinv_check() == 0, N.last_error()
    info = plan.selinv_info
    bcs = block_columns(sym)
    assert info["block_columns"] == len(bcs)
    assert info["flops"] == pytest.approx(nominal_flops(sym), rel=1e-12)
    assert info["levels"] == tree_levels(sym)
    assert info["device_bytes"] == 0
    assert 0 <= info["tiled_block_columns"] <= info["block_columns"]
    assert info["launches"] >= info["levels"]


def test_edge_pattern_shapes():
    _, sym = edge("dense150")
    assert sym.nsuper == 1
    assert [wb for _, _, wb, _ in block_columns(sym)] == [64, 64, 22]
    _, sym = edge("tridiag300")
    # a chain: every supernode but the last has exactly one child, its predecessor
    parents = sym.sParent.astype(int)
    assert (parents[:-1] == np.arange(1, sym.nsuper)).all() and parents[-1] == -1
    _, sym = edge("diag37")
    assert all(m == 0 for _, _, _, m in block_columns(sym))


@pytest.mark.parametrize("name", ["ex15", "dense150"])
def test_threshold_moves_block_columns_between_paths(plans, name, monkeypatch):
    plan, sym = plans(name)
    bcs = block_columns(sym)
    monkeypatch.setenv("PARSY_SELINV_TILED_MIN", "0")
    assert plan.selinv_info["tiled_block_columns"] == len(bcs)
    monkeypatch.setenv("PARSY_SELINV_TILED_MIN", "1000000000")
    assert plan.selinv_info["tiled_block_columns"] == 0
    monkeypatch.setenv("PARSY_SELINV_TILED_MIN", "40")
    assert plan.selinv_info["tiled_block_columns"] == sum(1 for *_, m in bcs if m >= 40)
    assert plan.selinv_check() == 0


def test_host_only_plan_refuses_device_calls(plans):
    plan, sym = plans("ex15")
    with pytest.raises(RuntimeError, match="without a device"):
        plan.selinv_device(1, 1 << 20)
    with pytest.raises(RuntimeError, match="without a device"):
        plan.inverse_diag_device(1, 1 << 20)
    with pytest.raises(RuntimeError, match="without a device"):
        plan.logdet_device(1)
    with pytest.raises(RuntimeError, match="without a device"):
        plan.selinv(np.zeros(int(sym.xsize)))
    assert plan.selinv_info["device_bytes"] == 0
