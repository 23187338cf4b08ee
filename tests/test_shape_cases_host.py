"""The catalogue of engineered shapes (shape_cases.py) without a GPU: every entry has exactly the supernodes it was built
for and takes the schedule path it exists for -- on a host-only plan --, so that an entry that drifts off its path fails
here instead of passing silently in the GPU tier; and the error measures themselves: the oracle passes them, planted
errors do not."""
import numpy as np
import pytest

import shape_cases as SC
from parsy_bench_amd import api, inspector as I

NAMES = [c.name for c in SC.CASES]


def _host_plan(monkeypatch, case, **override):
    SC.set_env(monkeypatch, {**case.env, **override})
    A, S, sym = SC.build(case)
    return sym, api.Plan(sym, -1)


@pytest.mark.parametrize("name", NAMES)
def test_entry_has_its_supernodes_and_takes_its_path(monkeypatch, name):
    case = SC.CASE_BY_NAME[name]
    sym, plan = _host_plan(monkeypatch, case)
    _, want = SC.arrow_layout(case.blocks, case.border, case.seed, case.chain)
    # (the analysis postorders the etree: the blocks may come in another order, the border stays last)
    got = SC.supernodes_of(sym)
    assert sorted(got) == sorted(want) and got[-1] == want[-1], f"{name}: supernodes {got}, engineered {want}"
    assert sym.n == case.n <= 1000
    assert plan.check() == 0
    info = plan.info
    assert info["n_small"] + info["n_big"] == info["n_pieces"] >= sym.nsuper == info["nsuper"]
    bad = {k: (info[k], want) for k, want in case.expect.items() if not SC.holds(info[k], want)}
    assert not bad, f"{name}: counters off their path (got, wanted): {bad}"
    if "PARSY_BIG_MINK" in case.env:
        assert info["big_tasks"] > 0 and info["n_pieces"] > sym.nsuper
    else:
        assert info["big_tasks"] == 0 and info["dense_tasks"] == 0 and info["n_pieces"] == sym.nsuper
    mode = case.env.get("PARSY_BIG_DENSE")
    if mode == "0":
        assert info["dense_entries"] == 0 and info["dense_tasks"] == 0
    if mode == "4":
        assert info["dense_entries"] >= 0.9 * info["big_entries"] > 0
    if case.family == "g":
        # two chain launches per level: more launches than the same plan without
        _, base = _host_plan(monkeypatch, case, PARSY_CHAIN_SPLIT="0")
        assert info["chol_launches"] > base.info["chol_launches"]
        assert api.N.lib().parsy_plan_chain_check(plan._h, 64) == 0


def test_the_lds_cap_and_the_update_count_decide_small_or_tiled(monkeypatch):
    """Both sides of w * r == 6144 and of 8 / 9 updates, read from the plans."""
    at, over = (_host_plan(monkeypatch, SC.CASE_BY_NAME[k])[0] for k in ("cap_at", "cap_over"))
    assert all(w * r == 6144 for w, r in SC.supernodes_of(at)[:-1])
    assert all(6144 < w * r <= 6144 + w for w, r in SC.supernodes_of(over)[:-1])
    eight, nine = (_host_plan(monkeypatch, SC.CASE_BY_NAME[k])[1].info for k in ("narrow_hi", "narrow_nine"))
    assert (eight["n_updates"], eight["n_big"]) == (8, 0) and (nine["n_updates"], nine["n_big"]) == (9, 1)


def test_push_groups_change_the_plan(monkeypatch):
    """PARSY_PUSH_GROUP=1, 2 and 3 on a border of five pieces are three different plans for the same flops."""
    infos = [_host_plan(monkeypatch, SC.CASE_BY_NAME[k])[1].info for k in ("push_1", "push_2", "push_3")]
    assert len({(i["big_tasks"], i["big_entries"]) for i in infos}) == 3, [(i["big_tasks"], i["big_entries"]) for i in infos]
    assert len({i["update_flops"] for i in infos}) == 1 and all(i["n_pieces"] - i["nsuper"] == 4 for i in infos)


def test_split_streams_are_reported(monkeypatch):
    on, off = (_host_plan(monkeypatch, SC.CASE_BY_NAME[k])[1].info for k in ("streams_split", "streams_whole"))
    assert on["split_tiles"] > 0 and 2 * on["split_tiles"] <= on["split_parts"] <= 8 * on["split_tiles"]
    assert off["split_tiles"] == 0 and off["split_parts"] == 0
    # a plan without early streams (two levels only) has none either, whatever the variables say
    case = SC.CASE_BY_NAME["cap_over"]
    _, plan = _host_plan(monkeypatch, case, PARSY_SPLIT_CHUNKS="1", PARSY_SPLIT_TARGET="1", PARSY_SPLIT_MAX="8")
    assert plan.info["split_tiles"] == 0


def test_the_catalogue_holds_every_value_of_every_knob():
    seen = {}
    for c in SC.CASES:
        for k in ("PARSY_BIG_DENSE", "PARSY_BIG_SUPER", "PARSY_DENSE_STRIPS", "PARSY_PUSH_GROUP"):
            if "PARSY_BIG_MINK" in c.env:
                seen.setdefault(k, set()).add(c.env.get(k))
    assert {"0", "2", "4"} <= seen["PARSY_BIG_DENSE"] and {None, "2", "2x1"} <= seen["PARSY_BIG_SUPER"]
    assert {None, "0"} <= seen["PARSY_DENSE_STRIPS"] and {"1", "2", "3"} <= seen["PARSY_PUSH_GROUP"]
    assert {c.family for c in SC.CASES} == set("abcdefghi")
    assert set(k for c in SC.CASES for k in c.kernels) | {"k_scatter_a"} == set(SC.FACTOR_KERNELS)
    assert all(set(c.env) <= set(SC.VARIABLES) for c in SC.CASES)


# ---------------------------------------------------------------------------
# the measures
# ---------------------------------------------------------------------------
def _oracle_factor(oracle, sym, values):
    ok, lo, _ = oracle.cholesky_05(sym, values, I.trivial_hlevel(sym))
    assert ok
    return lo


_ORACLE = {}


def _oracle_case(oracle, name, scaled):
    """(sym, S_perm, values, lValues of the oracle, dense factor), computed once."""
    if (name, scaled) not in _ORACLE:
        case = SC.CASE_BY_NAME[name]
        A, S, sym = SC.build(case)
        values = sym.permute_values(SC.scaled_values(A, 100 + case.seed)) if scaled else sym.A2x
        Sx = SC.scaled(S, 100 + case.seed) if scaled else S
        lo = _oracle_factor(oracle, sym, values)
        _ORACLE[(name, scaled)] = (sym, Sx[np.ix_(sym.Perm, sym.Perm)], values, lo, I.bcsc_to_dense(sym, lo))
    return _ORACLE[(name, scaled)]


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("name", ["cap_at", "chain"])
def test_the_oracle_passes_the_measures(oracle, name, scaled):
    sym, Sp, values, lo, Ld = _oracle_case(oracle, name, scaled)
    n = sym.n
    rho = SC.rho_factor(Sp, Ld)
    print(f"{name} scaled={scaled}: n = {n}, oracle rho_factor = {rho:.2f}")
    assert rho <= SC.limit(n), f"{name}: rho_factor of the oracle {rho:.3g} > {SC.limit(n)}"
    B = np.random.default_rng(5).standard_normal((n, 3))
    for q in range(3):
        xf = oracle.blocked_lsolve(sym, lo, B[:, q].copy(), "serial")
        xb = oracle.blocked_ltsolve(sym, lo, B[:, q].copy())
        rf, rb = SC.rho_solve(Ld, xf, B[:, q])[0], SC.rho_solve(Ld.T, xb, B[:, q])[0]
        print(f"{name} scaled={scaled}: oracle rho_solve forward {rf:.2f} backward {rb:.2f}")
        assert rf <= SC.limit(n) and rb <= SC.limit(n), (rf, rb)


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
def test_planted_errors_fail_the_measures(oracle, scaled):
    sym, Sp, values, lo, Ld = _oracle_case(oracle, "chain", scaled)
    n = sym.n
    rng = np.random.default_rng(9)
    # one entry of L off by a relative 1e-9: the smallest below the diagonal and the largest, either is seen
    low = np.tril(np.abs(Ld), -1)
    low[low == 0] = np.inf
    for i, j in (np.unravel_index(np.argmin(low), low.shape), np.unravel_index(np.argmax(np.tril(np.abs(Ld), -1)), Ld.shape)):
        bad = Ld.copy()
        bad[i, j] *= 1.0 + 1e-9
        rho = SC.rho_factor(Sp, bad)
        assert rho > 1000 * SC.limit(n), f"a relative error of 1e-9 in L[{i}, {j}] gives rho_factor = {rho:.3g} only"
    b = rng.standard_normal(n)
    # one component of a solution off by a relative 1e-9: the largest, and one of median size
    for T, x0 in ((Ld, oracle.blocked_lsolve(sym, lo, b.copy(), "serial")), (Ld.T, oracle.blocked_ltsolve(sym, lo, b.copy()))):
        order = np.argsort(np.abs(x0))
        for k, factor in ((order[-1], 1000), (order[n // 2], 1)):
            x = x0.copy()
            x[k] *= 1.0 + 1e-9
            rho = SC.rho_solve(T, x, b)[0]
            assert rho > factor * SC.limit(n), f"a relative error of 1e-9 in x[{k}] gives rho_solve = {rho:.3g} only"


@pytest.mark.parametrize("name", ["cap_at", "chain", "narrow_hi"])
def test_the_oracles_factor_is_homogeneous_under_scaling(oracle, name):
    """factor(D A D) == D factor(A) bitwise for D = diag(2^k): every operation of the factorization is a product, a sum of
    homogeneous terms or the square root of a pivot scaled by 4^k."""
    sym, _, _, _, Ld = _oracle_case(oracle, name, False)
    _, _, _, _, Ls = _oracle_case(oracle, name, True)
    d = SC.scaling(sym.n, 100 + SC.CASE_BY_NAME[name].seed)[sym.Perm]
    assert np.array_equal(Ls, d[:, None] * Ld)


def test_scaling_is_exact_and_badly_scaled():
    case = SC.CASE_BY_NAME["narrow_lo"]
    A, S, sym = SC.build(case)
    d = SC.scaling(case.n, 3)
    Sx = SC.scaled(S, 3)
    assert np.array_equal(Sx / d[:, None] / d[None, :], S) and d.min() >= 2.0 ** -20 and d.max() <= 2.0 ** 20 and d.max() / d.min() >= 2.0 ** 20
    assert np.array_equal(SC.lower_csc(Sx).Ax, SC.scaled_values(A, 3))
    # all off-diagonal values differ
    off = S[np.tril_indices(case.n, -1)]
    off = off[off != 0]
    assert len(np.unique(off)) == len(off)
