"""Selected inversion on the engineered block-column shapes of selinv_ref.py, CPU tier: every shape has exactly the
supernodes and the (wb, m) block-column classes it was made for; the split between the two kernel paths follows the
threshold and puts both on one level; and the reference the GPU tier (test_selinv_shapes_gpu.py) measures against is
itself within a fixed cap of the extended-precision inverse, equally so under the bad scaling.

Every measured value is printed (pytest -rP shows it for passing tests)."""
import numpy as np
import pytest

import selinv_ref as R
import shape_cases as SC
from test_selinv_host import block_columns

NAMES = list(R.SHAPES)
THRESHOLDS = [None, "33", "64", "65", "1000000000"]
_PLANS = {}


def _host_plan(name):
    if name not in _PLANS:
        from parsy_bench_amd import api
        sym = R.build(name)[2]
        _PLANS[name] = (sym, api.Plan(sym, -1))
    return _PLANS[name]


def _set_threshold(monkeypatch, threshold):
    if threshold is None:
        monkeypatch.delenv("PARSY_SELINV_TILED_MIN", raising=False)
    else:
        monkeypatch.setenv("PARSY_SELINV_TILED_MIN", threshold)


def block_column_levels(sym):
    """Level (depth from the root) of every block column, in block_columns' order: the parent of a block column is the
    next one of its supernode, or the first one of the supernode's etree parent."""
    nb = [-(-(int(sym.super[s + 1]) - int(sym.super[s])) // 64) for s in range(sym.nsuper)]
    dlast = [0] * sym.nsuper
    for s in range(sym.nsuper - 1, -1, -1):   # (a parent has a higher number than its children)
        p = int(sym.sParent[s])
        assert p < 0 or p > s
        dlast[s] = 0 if p < 0 else dlast[p] + nb[p]
    return [dlast[s] + nb[s] - 1 - j0 // 64 for s, j0, _, _ in block_columns(sym)]


@pytest.mark.parametrize("name", NAMES)
def test_shape_has_its_supernodes_and_block_columns(name, monkeypatch):
    from parsy_bench_amd import _native as N
    monkeypatch.delenv("PARSY_SELINV_TILED_MIN", raising=False)
    blocks, border, seed, chain = R.spec(name)
    sym, plan = _host_plan(name)
    want = SC.arrow_layout(blocks, border, seed, chain)[1]
    assert SC.supernodes_of(sym) == want, f"{name}: supernodes {SC.supernodes_of(sym)}, engineered {want}"
    assert sym.n <= 500
    got = [(wb, m) for _, _, wb, m in block_columns(sym)]
    print(f"BLOCK_COLUMNS shape={name} n={sym.n} {got}")
    missing = [c for c in R.classes(name) if c not in got]
    assert not missing, f"{name}: block-column classes {missing} are not among {got}"
    if name == "chain":
        # several runs of the gather map per supernode: the rows below a block belong to more than one ancestor
        owners = []
        for s in range(sym.nsuper - 1):
            c0, c1 = int(sym.super[s]), int(sym.super[s + 1])
            rows = np.asarray(sym.s[int(sym.i_ptr[c0]) + (c1 - c0): int(sym.i_ptr[c1])])
            owners.append(len(set(np.asarray(sym.col2Sup)[rows].tolist())))
        assert max(owners) >= 2, owners
    assert plan.selinv_check() == 0, N.last_error()
    assert plan.selinv_info["block_columns"] == len(got)


def test_the_tables_block_columns_exactly():
    """The whole (wb, m) lists of the two made-to-order shapes, in column order."""
    got = {k: [(wb, m) for _, _, wb, m in block_columns(_host_plan(k)[0])] for k in ("edges", "tall")}
    assert got["edges"] == [(1, 31), (16, 32), (63, 33), (64, 63), (64, 65), (1, 64), (17, 65), (64, 66), (64, 2), (1, 1),
                            (64, 66), (64, 2), (2, 0)]
    assert got["tall"] == [(8, 127), (64, 128), (33, 129), (2, 191), (64, 128), (64, 64), (64, 0)]


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("name", NAMES)
def test_threshold_counts(name, threshold, monkeypatch):
    sym, plan = _host_plan(name)
    _set_threshold(monkeypatch, threshold)
    t = 0 if threshold is None else int(threshold)
    ms = [m for *_, m in block_columns(sym)]
    info = plan.selinv_info
    assert info["tiled_block_columns"] == sum(1 for m in ms if m >= t), (name, threshold, info)
    assert plan.selinv_check() == 0


@pytest.mark.parametrize("threshold", [33, 64, 65])
def test_edges_has_a_level_with_both_paths(threshold):
    """From the block-column tree: under each of these thresholds some level of `edges` holds block columns on both sides
    of it, so the slot accounting of the split (T, Y and partial slots counted over the tiled ones only) matters."""
    sym, _ = _host_plan("edges")
    by_level = {}
    for lvl, (_, _, _, m) in zip(block_column_levels(sym), block_columns(sym)):
        by_level.setdefault(lvl, []).append(m)
    mixed = {lvl: sorted(ms) for lvl, ms in by_level.items() if min(ms) < threshold <= max(ms)}
    print(f"MIXED_LEVELS threshold={threshold} {mixed}")
    assert mixed, by_level
    # ... and the level of the blocks' last block columns holds m right below and at the threshold
    assert any(threshold - 1 in ms and threshold in ms for ms in mixed.values()), mixed


@pytest.mark.parametrize("name", NAMES)
def test_reference_is_sound(name):
    """The restatement against the extended-precision inverse, plain and under the scaling: within the cap (a condition,
    not a measurement: it keeps a broken reference from widening the device's allowance), the same figure for both value
    sets, and bitwise homogeneous."""
    ref = R.reference(name)
    d, mask = ref["d"], ref["mask"]
    (plain, at), (scaled, at_s) = ref["rho"][False], ref["rho"][True]
    print(f"RHO_SELINV_REF shape={name} n={ref['sym'].n} plain={plain:.3f} scaled={scaled:.3f} at={at}")
    assert 0 < plain <= R.REF_CAP and 0 < scaled <= R.REF_CAP
    assert plain == scaled and at == at_s
    assert np.array_equal(ref["Zt"][True], ref["Zt"][False] / (d[:, None] * d[None, :]))
    # the reference of the scaled values is the exact scaling of the plain one, and the measure sees a planted error
    assert R.measure(ref["Zx"][False], ref["Zx"][False], mask)[0] == 0.0
    Zbad = ref["Zt"][False].copy()
    i = ref["sym"].n // 2
    Zbad[i, i] *= 1.0 + 2.0 ** -48   # 32 u on a diagonal entry
    assert R.measure(Zbad, ref["Zx"][False], mask)[0] > R.MARGIN * plain
