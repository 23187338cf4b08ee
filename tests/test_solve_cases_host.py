"""The solve catalogue (solve_cases.py) without a GPU: its names and variables are real, its cells cover the witness
table, every shape has the supernodes it was engineered to have, every cell takes the path it exists for on a host-only
plan (the launch tables and counters of the plan through solve_cases.predict), and the limit the GPU tier holds the
kernels to is attainable at exactly these inputs: a plain float64 substitution passes it."""
import numpy as np
import pytest

import shape_cases as SC
import solve_cases as V
from parsy_bench_amd import api
from test_kernel_witness import SOLVE_ENTRIES

NAMES = [c.name for c in V.CELLS]
_PLANS = {}


def _host_plan(monkeypatch, cell):
    """(sym, info, launch tables) of the cell's plan, host-only; made once per (shape, plan_env)."""
    if cell.plan_key not in _PLANS:
        V.set_env(monkeypatch, cell.plan_env)
        A, S, sym = V.build(V.SHAPES[cell.shape])
        plan = api.Plan(sym, -1)
        assert plan.check() == 0
        _PLANS[cell.plan_key] = (sym, plan.info, V.launch_tables(plan))
    return _PLANS[cell.plan_key]


def test_names_and_variables_are_real():
    table = api.kernel_launches()
    for c in V.CELLS:
        assert c.kernels and set(c.kernels) | set(c.absent) <= set(table), c.name
        assert not set(c.kernels) & set(c.absent), f"{c.name}: an entry both required and absent"
        assert set(c.plan_env) <= set(V.PLAN_VARIABLES) and set(c.solve_env) <= set(V.SOLVE_VARIABLES), c.name
        assert c.shape in V.SHAPES and c.direction in ("forward", "backward") and c.nrhs >= 1 and c.intent, c.name
        assert c.plan_env.get("PARSY_SOLVE_ONE") in ("0", "2"), f"{c.name}: the ONE-launch mode is part of every cell"
    assert set(V.PLAN_VARIABLES) | set(V.SOLVE_VARIABLES) | set(SC.VARIABLES) == set(V.VARIABLES)


def test_prediction_reads_the_headers_right():
    """What solve_cases.predict mirrors of the headers, read from them: the fields of parsy::Launch in declaration order
    (schedule.hpp: a row of the launch table) and the defaults of SolveGates (solve_route.hpp)."""
    import re
    from test_kernel_witness import CSRC, source_text
    body = re.search(r"struct Launch \{(.*?)\};", source_text(CSRC / "schedule.hpp"), flags=re.S).group(1)
    fields = [m for decl in re.findall(r"int32_t ([^;]*);", body) for m in re.findall(r"(\w+)(?:\s*=\s*[^,]+)?(?:,|$)", decl.strip())]
    assert tuple(fields) == V.LAUNCH_FIELDS, fields
    assert re.search(r"constexpr int kLaunchFields = (\d+);", source_text(CSRC / "schedule.hpp")).group(1) == str(len(V.LAUNCH_FIELDS))
    kinds = dict(re.findall(r"(kLaunch\w+) = (\d+)", source_text(CSRC / "schedule.hpp")))
    assert [int(kinds[k]) for k in ("kLaunchBackBelow", "kLaunchSolveSmall", "kLaunchSolvePanel", "kLaunchSolveFixup", "kLaunchBackBlock")] == \
        [V.BACK_BELOW, V.SOLVE_SMALL, V.SOLVE_PANEL, V.SOLVE_FIXUP, V.BACK_BLOCK]
    forms = dict(re.findall(r"(kForm\w+) = (\d+)", source_text(CSRC / "schedule.hpp")))
    assert [int(forms[k]) for k in ("kFormEach", "kFormChain", "kFormSubtrees")] == [V.EACH, V.CHAIN, V.SUBTREES]
    gates = re.search(r"struct SolveGates \{(.*?)\};", source_text(CSRC / "solve_route.hpp"), flags=re.S).group(1)
    defaults = {k: int(v) for k, v in re.findall(r"int (\w+) = (\d+);", gates)}
    assert {k: defaults.get(k) for k in V.GATE_DEFAULTS} == V.GATE_DEFAULTS, defaults
    assert set(defaults) - set(V.GATE_DEFAULTS) <= {"wait_bias", "sub_abl"}, "a gate of SolveGates that the prediction does not know"
    assert re.search(r"bool bmrhs_wide_only = true;", gates) and re.search(r"bool xt_min_set = false;", gates)


def test_cells_cover_the_witness_table():
    union = {k for c in V.CELLS for k in c.kernels}
    assert union == set(SOLVE_ENTRIES) - {"k_copy_segments"}, (sorted(set(SOLVE_ENTRIES) - union), sorted(union - set(SOLVE_ENTRIES)))


def test_pairs_differ_in_the_gate_only():
    pairs = [c for c in V.CELLS if c.pair]
    assert {c.shape for c in pairs} >= {"dense_65", "dense_129", "dense_257", "tiles_70", "tiles_130", "tiles_257", "cap_over", "wide_130"}
    for c in pairs:
        o = V.CELL_BY_NAME[c.pair]
        assert o.pair == c.name and (o.shape, o.plan_env, o.nrhs, o.direction) == (c.shape, c.plan_env, 1, "forward")
        assert c.plan_env == V.L0 and set(c.solve_env) == set(o.solve_env) == {"PARSY_CHAIN_FEW_CHUNKS"}
        assert {c.solve_env["PARSY_CHAIN_FEW_CHUNKS"], o.solve_env["PARSY_CHAIN_FEW_CHUNKS"]} == {"0", "1000000"}


@pytest.mark.parametrize("name", list(V.SHAPES))
def test_shape_has_its_supernodes(name):
    shape = V.SHAPES[name]
    A, S, sym = V.build(shape)
    got, want = SC.supernodes_of(sym), V.engineered(shape)
    # (the analysis postorders the etree: the blocks may come in another order, the border stays last)
    assert sorted(got) == sorted(want) and got[-1] == want[-1], f"{name}: supernodes {got}, engineered {want}"
    assert sym.n == shape.n <= 1000
    assert any(c.shape == name for c in V.CELLS), f"{name}: a shape no cell uses"


# what a cell's plan must look like beyond the kernels predicted for it: (counter or table property, value)
def _chain_counts(tables, kind, field=V.COUNT):
    return sorted(int(r[field]) for r in tables[0 if kind == V.SOLVE_PANEL else 1] if r[V.KIND] == kind and r[V.FORM] == V.CHAIN)


_PINS = {
    # 130 columns over 300 rows: two 256-row chunks; the border of 171 columns: one
    "w4_wide_130": lambda info, t: _chain_counts(t, V.SOLVE_PANEL) == [1, 2],
    # (the second chunk of dense_257 is one row)
    "w4_dense_257": lambda info, t: _chain_counts(t, V.SOLVE_PANEL) == [2],
    # block columns 2 + 2 + 2 and chunk tasks of 128 rows: 1 + 2 + 3; the border: five block columns, no rows below
    "tall_f2": lambda info, t: _chain_counts(t, V.SOLVE_PANEL, V.TASK_COUNT) == [5, 12],
    # one supernode of 513 rows below: two block columns x two chunks
    "below_b1": lambda info, t: [int(r[V.COUNT]) for r in t[1] if r[V.KIND] == V.BACK_BELOW] == [4],
    "tall_b1": lambda info, t: not any(r[V.KIND] == V.BACK_BELOW for r in t[1]),
    # levels of six and of five block columns: PARSY_BCHAIN_MIN_BLOCKS=6 sends one through each kernel
    "tall_b65": lambda info, t: _chain_counts(t, V.BACK_BLOCK) == [5, 6],
    "tiny_f1": lambda info, t: [int(r[V.WIDTH]) for r in t[0]] == [16, 40],
    "lo_f9": lambda info, t: [int(r[V.WIDTH]) for r in t[0]] == [17, 40],
    "n32_f33": lambda info, t: [int(r[V.WIDTH]) for r in t[0] if r[V.KIND] == V.SOLVE_SMALL] == [32, 64],
    "n32_b8": lambda info, t: [int(r[V.WIDTH_CLASS]) for r in t[1]] == [0, 2],
    "tiny_b1": lambda info, t: [int(r[V.WIDTH_CLASS]) for r in t[1]] == [0, 1],
    "one_chain_f2": lambda info, t: info["nlevels"] == 6,
    "subc_f1_level": lambda info, t: info["solve_subtrees"] == 23 and info["solve_subtree_supernodes"] > info["solve_subtrees"],
    "sub_f6": lambda info, t: info["solve_subtrees"] == 40 == info["solve_subtree_supernodes"],
}


@pytest.mark.parametrize("name", NAMES)
def test_cell_takes_its_path(monkeypatch, name):
    cell = V.CELL_BY_NAME[name]
    shape = V.SHAPES[cell.shape]
    sym, info, tables = _host_plan(monkeypatch, cell)
    assert info["solve_launches"] == len(tables[0]) and info["backsolve_launches"] == len(tables[1])
    blocks = sum(-(-w // 64) for w, _ in SC.supernodes_of(sym))
    if cell.plan_env["PARSY_SOLVE_ONE"] == "2":
        assert info["solve_one"] & 3 == 3 and info["solve_one_blocks"] == blocks and cell.nrhs <= 8
    else:
        assert info["solve_one"] == 0 and info["solve_one_blocks"] == 0
    if "PARSY_SUBTREES" in cell.plan_env:
        assert info["solve_subtrees"] > 0 and info["sub_mrhs_tiers"] >= 1
        if cell.plan_env["PARSY_SUB_TIER_MIN_TREES"] == "0":
            assert info["sub_mrhs_tiers"] == 1 and info["sub_mrhs_cover_level"] == -1
        else:   # (bands up to the root: every level is in a tier)
            assert info["sub_mrhs_tiers"] >= 2 and info["sub_mrhs_cover_level"] == info["nlevels"] - 1
    else:
        assert info["solve_subtrees"] == 0 and info["sub_mrhs_tiers"] == 0
    unfused = "PARSY_FORCE_UNFUSED" in cell.plan_env
    assert unfused == any(r[V.KIND] == V.SOLVE_FIXUP for r in tables[0])
    assert not (unfused and any(r[V.FORM] == V.CHAIN for t in tables for r in t))
    if name == "rhs_ones":
        assert info["max_rows"] > 256   # (more than one workgroup per panel)
        return
    pred = V.predict(info, tables, cell.plan_env, cell.solve_env, cell.nrhs, cell.forward)
    assert set(cell.kernels) <= pred, f"{name}: not on its path: {sorted(set(cell.kernels) - pred)} (predicted {sorted(pred)})"
    assert not set(cell.absent) & pred, f"{name}: {sorted(set(cell.absent) & pred)} predicted"
    if cell.pair:
        # with no variable set the launch is one of few chunks: k_solve_chain_w<2>, as before the gate
        assert "k_solve_chain_w<2>" in V.predict(info, tables, cell.plan_env, {}, 1, True)
        assert all(0 < n <= 384 for n in _chain_counts(tables, V.SOLVE_PANEL))
    if name in _PINS:
        assert _PINS[name](info, tables), f"{name}: the plan is off the border of the cell: {cell.intent}"


def test_pins_name_cells():
    assert set(_PINS) <= set(NAMES)


def test_prediction_follows_the_gates(monkeypatch):
    """The prediction itself on one plan: each gate moves the kernel it is the gate of."""
    cell = V.CELL_BY_NAME["tall_b65"]
    sym, info, tables = _host_plan(monkeypatch, cell)
    p = lambda env, nrhs, fwd: V.predict(info, tables, cell.plan_env, env, nrhs, fwd)
    assert p({}, 1, True) >= {"k_solve_chain_w<2>", "k_diag_inverse"} and "k_solve_arm_wide" not in p({}, 1, True)
    assert "k_solve_chain_w<4>" in p({"PARSY_CHAIN_FEW_CHUNKS": "3"}, 1, True) and "k_solve_chain_w<2>" in p({"PARSY_CHAIN_FEW_CHUNKS": "3"}, 1, True)
    assert "k_solve_blocks_mrhs<true>" in p({}, 16, True) and "k_solve_blocks_mrhs<false>" in p({}, 17, True)
    assert "k_solve_blocks_mrhs<true>" in p({"PARSY_MRHS_MIN": "1"}, 1, True)
    assert "k_transpose_x" in p({}, 16, True) and "k_transpose_x" not in p({}, 15, True) and "k_transpose_x" not in p(V.NO_XT, 16, True)
    assert p({}, 1, False) >= {"k_bsolve_chain_w"} and "k_bsolve_below" not in p({}, 1, False)
    assert p({}, 65, False) >= {"k_bsolve_block<4>"}
    assert "k_bsolve_block_mrhs<1>" in p({"PARSY_BMRHS_WIDE_ONLY": "0"}, 65, False)
    assert "k_bsolve_block_mrhs<4>" in p({"PARSY_BMRHS_WIDE_BLOCKS": "6"}, 65, False) and "k_bsolve_block<4>" in p({"PARSY_BMRHS_WIDE_BLOCKS": "6"}, 65, False)
    assert "k_bsolve_block_mrhs<1>" in p({"PARSY_BMRHS_WIDE_BLOCKS": "1"}, 16, False)   # (64 per pass only above 16 right-hand sides)
    assert "k_bsolve_chain_mrhs" in p({"PARSY_BCHAIN_MIN_BLOCKS": "1"}, 17, False) and "k_bsolve_chain_mrhs" not in p({"PARSY_BCHAIN_MIN_BLOCKS": "1"}, 16, False)


# ---------------------------------------------------------------------------
# the limit is attainable at these inputs
# ---------------------------------------------------------------------------
def _substitute(L, B, forward):
    """Plain float64 column-oriented substitution: L x = b, or L' x = b."""
    X = np.array(B, dtype=np.float64)
    n = L.shape[0]
    if forward:
        for j in range(n):
            X[j] /= L[j, j]
            X[j + 1:] -= np.outer(L[j + 1:, j], X[j])
    else:
        for j in range(n - 1, -1, -1):
            X[j] /= L[j, j]
            X[:j] -= np.outer(L[j, :j], X[j])
    return X


@pytest.mark.parametrize("name", list(V.SHAPES))
def test_the_limit_is_attainable(name):
    """For every (shape, values, right-hand sides, direction) of the catalogue a reference substitution on numpy's own
    Cholesky factor of the permuted matrix gives rho_solve <= n + 1: no cell asks a kernel for more than that delivers."""
    shape = V.SHAPES[name]
    A, S, sym = V.build(shape)
    n = sym.n
    wanted = sorted({(c.nrhs, c.forward) for c in V.CELLS if c.shape == name and c.name != "rhs_ones"})
    for scaled in (False, True):
        L = np.linalg.cholesky(V.dense(shape, S, sym, scaled))
        for nrhs, forward in wanted:
            B = V.rhs(shape, nrhs)
            rho = SC.rho_solve(L if forward else L.T, _substitute(L, B, forward), B)
            print(f"{name} scaled={scaled} nrhs={nrhs} {'forward' if forward else 'backward'}: reference rho_solve = {rho.max():.3f}, limit {SC.limit(n)}")
            assert rho.max() <= SC.limit(n), (name, scaled, nrhs, forward, float(rho.max()))
        if any(c.name == "rhs_ones" and c.shape == name for c in V.CELLS):
            Lt = np.tril(L)
            ref = Lt.astype(np.longdouble).sum(axis=1)
            err = np.abs(Lt.sum(axis=1).astype(np.longdouble) - ref).astype(np.float64)
            assert (err <= ((Lt != 0).sum(axis=1) + 2) * SC.U * np.abs(Lt).sum(axis=1)).all()
