"""The host-buffer calls of every family in turn on ONE plan: they share the plan's staging buffers (the values, the
factor, the right-hand sides) and its byte count.  Every result is compared with the same call on a fresh plan that has
done nothing else, by what the call's own tests assert: the factor (test_host_factorization_with_pipelined_download),
the selected inverse and the log-determinant (test_selinv_gpu.test_reproducible) and the gradients' kernels (fixed
summation order) bitwise; the solves, which sum with FP64 atomics, by test_gpu_parity._same and test_refine_gpu._agree."""
import numpy as np
import pytest

from conftest import problem
from test_gpu_parity import _same
from test_refine_gpu import _agree
from test_selinv_gpu import _dev

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _plan(api, sym):
    """A fresh plan in the ordering solve_refined would give it on first use (selinv's diagonal and pattern_outer work in
    the plan's ordering: the shared plan and the fresh ones must agree on it whatever ran before)."""
    plan = api.Plan(sym, 0)
    plan.set_perm(sym.Perm)
    plan._perm_set = True
    return plan


def _counts(plan):
    return plan.info["device_bytes"], plan.selinv_info["device_bytes"], plan.grad_info["device_bytes"]


@pytest.mark.parametrize("name", ["tiny2d", "small3d"])
def test_families_share_one_plan(api, monkeypatch, name):
    A, perm, sym = problem(name)
    n = sym.n
    rng = np.random.default_rng(31)
    b1, b1b = rng.standard_normal(n), rng.standard_normal(n)
    B3, B5 = rng.standard_normal((n, 3)), rng.standard_normal((n, 5))
    Lam, X2 = rng.standard_normal((n, 2)), rng.standard_normal((n, 2))
    vals2 = sym.A2x * 1.5   # (as positive definite as A)
    monkeypatch.delenv("PARSY_HOST_PIPELINE", raising=False)

    def fresh(call):
        p = _plan(api, sym)
        try:
            return call(p)
        finally:
            p.close()

    def factor2(p):
        monkeypatch.setenv("PARSY_HOST_PIPELINE", "2")
        try:
            out, _ = p.factor(vals2, out=np.full(int(sym.xsize), np.nan))
            assert p.status() == 0
            return out
        finally:
            monkeypatch.delenv("PARSY_HOST_PIPELINE")

    def logdet(p, lv):
        ld, col = p.logdet_device(_dev(lv).data_ptr())
        assert col == 0
        return ld

    plans = [_plan(api, sym)]   # (closed whatever the test finds)
    one = plans[0]
    try:
        # 1. factor
        lv, _ = one.factor(sym.A2x)
        assert one.status() == 0
        assert np.array_equal(_bits(lv), _bits(fresh(lambda p: p.factor(sym.A2x)[0]))), "1: factor"
        # 2. solve, one right-hand side
        x, _ = one.solve(lv, b1)
        _same(x, fresh(lambda p: p.solve(lv, b1)[0]), "2: solve")
        # 3. selinv with the diagonal, and the log-determinant
        z, diag, _ = one.selinv(lv)
        z0, diag0, _ = fresh(lambda p: p.selinv(lv))
        assert np.array_equal(_bits(z), _bits(z0)) and np.array_equal(_bits(diag), _bits(diag0)), "3: selinv"
        assert _bits(logdet(one, lv)) == _bits(fresh(lambda p: logdet(p, lv))), "3: logdet"
        # 4. solve_refined, 3 right-hand sides
        xr, ir = one.solve_refined(sym.A2x, lv, B3)
        xr0, ir0 = fresh(lambda p: p.solve_refined(sym.A2x, lv, B3))
        _agree(xr, ir["steps"], ir["berr"], xr0, ir0["steps"], ir0["berr"], "4: solve_refined")
        # 5. pattern_outer, 2 right-hand sides
        g = one.pattern_outer(Lam, X2)
        assert np.array_equal(_bits(g), _bits(fresh(lambda p: p.pattern_outer(Lam, X2)))), "5: pattern_outer"
        # 6. inverse_pattern of that Z
        gz = one.inverse_pattern(z)
        assert np.array_equal(_bits(gz), _bits(fresh(lambda p: p.inverse_pattern(z)))), "6: inverse_pattern"
        # 7. solve2, 5 right-hand sides: the right-hand sides' buffer grows
        x5, _ = one.solve2(lv, B5)
        _same(x5, fresh(lambda p: p.solve2(lv, B5)[0]), "7: solve2")
        # 8. factor of other values with the download behind the kernels
        lv2 = factor2(one)
        assert not np.isnan(lv2).any(), "8: a part of lValues was never downloaded"
        assert np.array_equal(_bits(lv2), _bits(fresh(factor2))), "8: pipelined factor"
        # 9. solve, one right-hand side, in the grown buffer
        x9, _ = one.solve(lv2, b1b)
        _same(x9, fresh(lambda p: p.solve(lv2, b1b)[0]), "9: solve after the buffer grew")

        # the byte counts: the same calls in family order on a fresh plan
        plans.append(_plan(api, sym))
        fam = plans[-1]
        fam.factor(sym.A2x)
        factor2(fam)
        fam.solve(lv, b1)
        fam.solve2(lv, B5)
        fam.solve(lv2, b1b)
        fam.solve_refined(sym.A2x, lv, B3)
        fam.selinv(lv)
        logdet(fam, lv)
        fam.pattern_outer(Lam, X2)
        fam.inverse_pattern(z)
        assert _counts(one) == _counts(fam)
        assert all(c > 0 for c in _counts(one))
    finally:
        for p in plans:
            p.close()


@pytest.mark.parametrize("restrict", ["set_active", "set_active_pieces"])
def test_byte_count_does_not_drift_with_set_active(api, restrict):
    """parsy_plan_set_active / _set_active_pieces make the launch arrays again; the plan's device_bytes must take the old
    ones off before it adds the new ones.  A mask that drops the last supernode (piece), then no mask, three times: after
    every pair a solve brings the count back to exactly what it was after the first factor and solve, and gives the
    same solution.  (Before device memory was owned through device_buffer.hpp this failed: every call added the launch
    arrays and the backward partial sums again and took nothing off.)

    Between the pair and the solve the count is lower by the solves' hand-off buffers, which are sized by the launch
    lists, released with them and made again by the next solve: that idle count is the same after every pair, and
    equals the first count on a plan whose solves use no such buffers."""
    A, perm, sym = problem("tiny2d")
    rng = np.random.default_rng(7)
    b1 = rng.standard_normal(sym.n)
    plan = _plan(api, sym)
    try:
        lv, _ = plan.factor(sym.A2x)
        assert plan.status() == 0
        x0, _ = plan.solve(lv, b1)
        b = plan.info["device_bytes"]
        count = sym.nsuper if restrict == "set_active" else len(plan.pieces()["supernode"])
        mask = np.ones(count, dtype=np.uint8)
        mask[-1] = 0
        idle = []
        for k in range(3):
            getattr(plan, restrict)(mask)
            getattr(plan, restrict)(None)
            idle.append(plan.info["device_bytes"])
            x, _ = plan.solve(lv, b1)
            now = plan.info["device_bytes"]
            print(f"{restrict} round {k}: before {b}, after the pair {idle[-1]}, after a solve {now}")
            assert now == b, f"round {k}: device_bytes {now} after the pair and a solve, {b} before"
            _same(x, x0, f"round {k}: solve after {restrict}")
        assert idle[0] <= b and idle == [idle[0]] * 3, (b, idle)
    finally:
        plan.close()


def test_byte_counts_follow_growth(api):
    """Workspaces that grow are made again at exactly the size asked for, and the meters follow: after solve_refined with
    1, 3 and 1 right-hand sides, factor_apply(G) with 2 and 9 and rcond, the plan's count and every feature's equal
    those of a fresh plan that makes only the widest call of each family."""
    A, perm, sym = problem("small3d")
    n = sym.n
    rng = np.random.default_rng(11)
    B = rng.standard_normal((n, 9))

    def counts(p):
        return {"plan": p.info["device_bytes"], "selinv": p.selinv_info["device_bytes"],
                "grad": p.grad_info["device_bytes"], "cond": p.cond_info["device_bytes"],
                "apply": p.apply_info["device_bytes"]}

    plans = [_plan(api, sym), _plan(api, sym)]
    grown, widest = plans
    try:
        lv, _ = grown.factor(sym.A2x)
        assert grown.status() == 0
        for k in (1, 3, 1):
            grown.solve_refined(sym.A2x, lv, B[:, :k])
        for k in (2, 9):
            grown.factor_apply(lv, B[:, :k], "G")
        grown.rcond(sym.A2x, lv)
        widest.factor(sym.A2x)
        widest.solve_refined(sym.A2x, lv, B[:, :3])
        widest.factor_apply(lv, B, "G")
        widest.rcond(sym.A2x, lv)
        print("grown", counts(grown), "widest", counts(widest))
        assert counts(grown) == counts(widest)
        assert counts(grown)["plan"] > 0 and counts(grown)["cond"] > 0 and counts(grown)["apply"] > 0
    finally:
        for p in plans:
            p.close()
