"""Every solve kernel on the engineered shapes of solve_cases.py, componentwise, by witness (the -m gpu tier).

One plan and one factorization (plain values and D A D, D = diag(2^k), |k| <= 20) per (shape, variables read when the
plan is built), made once.  Every cell of the catalogue then solves through the device entry points (plan.solve_device /
plan.backsolve_device) on X with a leading dimension of n + 37 and a tail of 53 entries, with its own variables set after
all the catalogue's variables are cleared, and is held to

* solve_status() == 0, the padding rows and the tail keep their bits;
* rho_solve <= n + 1 units of u = 2^-53 for every column (shape_cases.py: the measure and the limit);
* the kernel witness: every entry of cell.kernels launched, none of cell.absent, and the counts of all entries are
  exactly those of the library's own route of that solve (solve_cases.route: parsy_debug_solve_route);
* for the k_solve_chain_w<4> / <2> pairs: the two X agree normwise to SOLVE_TOL.

Between them the cells launch every solve entry of the witness table but k_copy_segments (the last test).
test_solve_cases_host.py pins every cell to its path without a GPU and proves the limit attainable at these inputs.

Every measured value is printed (pytest -rP shows it for passing tests) and stands in the assertion messages.
"""
from collections import Counter

import numpy as np
import pytest

import shape_cases as SC
import solve_cases as V
from parsy_bench_amd import inspector as I
from test_kernel_witness import SOLVE_ENTRIES

pytestmark = pytest.mark.gpu

SOLVE_TOL = 1e-10          # the normwise comparison of test_gpu_parity.py
_SENTINEL = 1234.5678125   # (finite: the armed pattern is a NaN) -- test_gpu_parity.test_padded_leading_dimension
_PAD, _TAIL = 37, 53
NAMES = [c.name for c in V.CELLS]
_PLANS = {}
_RESULTS = {}


def _plan(api, monkeypatch, cell):
    """The plan of the cell's (shape, plan_env) and its two factors, on the host (dense) and on the device; made once."""
    import torch
    if cell.plan_key not in _PLANS:
        shape = V.SHAPES[cell.shape]
        A, S, sym = V.build(shape)
        got, want = SC.supernodes_of(sym), V.engineered(shape)
        assert sorted(got) == sorted(want) and got[-1] == want[-1] and sym.n <= 1000, f"{cell.shape}: supernodes {got}, engineered {want}"
        V.set_env(monkeypatch, cell.plan_env)
        plan = api.Plan(sym, 0)
        run = {"plan": plan, "sym": sym, "shape": shape}
        for scaled in (False, True):
            lv, _ = plan.factor(V.values(shape, A, sym, scaled))
            assert plan.status() == 0, f"{cell.shape}: factor status {plan.status()}"
            run[scaled] = {"lv": lv, "Ld": I.bcsc_to_dense(sym, lv), "dev": torch.from_numpy(lv).to(torch.device("cuda", 0))}
        _PLANS[cell.plan_key] = run
    return _PLANS[cell.plan_key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _solve(api, run, cell, scaled, B):
    """X of one device solve of the cell (the caller has set its variables), the witness of that solve alone and the
    library's route of it (a Counter of witness names)."""
    import torch
    plan, n, nrhs = run["plan"], run["sym"].n, cell.nrhs
    ldx = n + _PAD
    buf = np.full(ldx * nrhs + _TAIL, _SENTINEL)
    buf[:ldx * nrhs].reshape(nrhs, ldx)[:, :n] = B.T
    Xd = torch.from_numpy(buf).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    api.reset_kernel_launches()
    (plan.solve_device if cell.forward else plan.backsolve_device)(run[scaled]["dev"].data_ptr(), Xd.data_ptr(), nrhs, ldx)
    torch.cuda.synchronize()
    seen = api.kernel_launches()
    what = f"{cell.name} scaled={scaled}"
    assert plan.solve_status() == 0, f"{what}: solve status {plan.solve_status()}"
    out = Xd.cpu().numpy()
    body = out[:ldx * nrhs].reshape(nrhs, ldx)
    assert np.array_equal(_bits(body[:, n:]), _bits(np.full((nrhs, _PAD), _SENTINEL))), f"{what}: the padding rows of X were written"
    assert np.array_equal(_bits(out[ldx * nrhs:]), _bits(np.full(_TAIL, _SENTINEL))), f"{what}: written past the last column"
    return np.ascontiguousarray(body[:, :n].T), seen, Counter(V.route(plan, nrhs, ldx, cell.forward))


def _check_witness(cell, seen, what):
    launched = sorted(k for k, v in seen.items() if v)
    missing = [k for k in cell.kernels if not seen[k]]
    unwanted = [k for k in cell.absent if seen[k]]
    assert not missing and not unwanted, f"{what}: launched {launched}; missing {missing}, must not launch {unwanted}"


def _rhs_ones(api, run, cell):
    """parsy_rhs_ones_device against L 1 in long double: per row a sum of its K stored entries makes at most K roundings
    of partial sums that never exceed M = sum |l|, and rounding the reference adds one: |got - ref| <= (K + 2) u M
    (test_apply_gpu._check_products).  Returns max err / bound per set of values and the witness."""
    import torch
    plan, n = run["plan"], run["sym"].n
    out = {"rho": {}, "seen": {}, "X": {}}
    for scaled in (False, True):
        Ld = np.tril(run[scaled]["Ld"])
        bd = torch.zeros(n, dtype=torch.float64, device=torch.device("cuda", 0))
        torch.cuda.synchronize()
        api.reset_kernel_launches()
        plan.rhs_ones_device(run[scaled]["dev"].data_ptr(), bd.data_ptr())
        torch.cuda.synchronize()
        out["seen"][scaled] = api.kernel_launches()
        ref = Ld.astype(np.longdouble).sum(axis=1)
        M, K = np.abs(Ld).sum(axis=1), (Ld != 0).sum(axis=1)
        err = np.abs(bd.cpu().numpy().astype(np.longdouble) - ref).astype(np.float64)
        out["rho"][scaled] = err / ((K + 2) * SC.U * M)
    return out


def _result(api, monkeypatch, name):
    """The cell's solves with both factors -- X, rho_solve of every column, the witness of each solve --, made once."""
    if name not in _RESULTS:
        cell = V.CELL_BY_NAME[name]
        run = _plan(api, monkeypatch, cell)
        V.set_env(monkeypatch, {**cell.plan_env, **cell.solve_env})
        if name == "rhs_ones":
            _RESULTS[name] = _rhs_ones(api, run, cell)
        else:
            B = V.rhs(run["shape"], cell.nrhs)
            out = {"rho": {}, "seen": {}, "X": {}, "route": {}}
            for scaled in (False, True):
                out["X"][scaled], out["seen"][scaled], out["route"][scaled] = _solve(api, run, cell, scaled, B)
                Ld = run[scaled]["Ld"]
                out["rho"][scaled] = SC.rho_solve(Ld if cell.forward else Ld.T, out["X"][scaled], B)
            _RESULTS[name] = out
    return _RESULTS[name]


@pytest.mark.parametrize("name", NAMES)
def test_solve_cell(api, monkeypatch, name):
    cell = V.CELL_BY_NAME[name]
    got = _result(api, monkeypatch, name)
    n = V.SHAPES[cell.shape].n
    limit = 1 if name == "rhs_ones" else SC.limit(n)   # (rhs_ones: in units of its own bound (K + 2) u M per row)
    worst = {s: float(got["rho"][s].max()) for s in (False, True)}
    print(f"RHO_SOLVE cell={name} kernels={','.join(cell.kernels)} {cell.direction}={max(worst.values()):.3f} "
          f"plain={worst[False]:.3f} scaled={worst[True]:.3f} limit={limit}")
    for scaled in (False, True):
        what = f"{name} ({cell.shape}, nrhs={cell.nrhs}, {cell.direction}) scaled={scaled}"
        _check_witness(cell, got["seen"][scaled], what)
        if name != "rhs_ones":
            counts = Counter({k: v for k, v in got["seen"][scaled].items() if v})
            assert counts == got["route"][scaled], f"{what}: launched {dict(counts)}, the route says {dict(got['route'][scaled])}"
        rho = got["rho"][scaled]
        assert rho.max() <= limit, f"{what}: rho = {rho.max():.4g} (column / row {int(rho.argmax())}) > {limit}; {cell.intent}"
    if cell.pair:
        other = _result(api, monkeypatch, cell.pair)
        for scaled in (False, True):
            X, Y = got["X"][scaled], other["X"][scaled]
            err = np.abs(X - Y).max() / max(1.0, np.abs(Y).max())
            print(f"PAIR {name} / {cell.pair} scaled={int(scaled)} err={err:.3e}")
            assert err <= SOLVE_TOL, f"{name} against {cell.pair} scaled={scaled}: {err:.3e}"


@pytest.mark.parametrize("nrhs", [1, 3])
@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_solve_in_steps_of_levels(api, monkeypatch, direction, nrhs):
    """tiles_257 through parsy_solve_levels_device in steps of one level: the witness counts summed over the steps are those
    of the steps' routes (solve_cases.route_levels), and X is the one-call solve's -- bitwise backward, where every sum
    has one order, and to SOLVE_TOL forward, where the chain's updates arrive by atomics."""
    import torch
    cell = V.CELL_BY_NAME["w2_tiles_257"]
    assert cell.plan_env == V.L0
    run = _plan(api, monkeypatch, cell)
    V.set_env(monkeypatch, cell.plan_env)
    plan, n, forward = run["plan"], run["sym"].n, direction == "forward"
    ldx = n + _PAD
    B = V.rhs(run["shape"], nrhs)
    buf = np.full(ldx * nrhs + _TAIL, _SENTINEL)
    buf[:ldx * nrhs].reshape(nrhs, ldx)[:, :n] = B.T
    dev = torch.device("cuda", 0)
    Ld, Xd, Yd = run[False]["dev"], torch.from_numpy(buf).to(dev), torch.from_numpy(buf).to(dev)
    (plan.solve_device if forward else plan.backsolve_device)(Ld.data_ptr(), Yd.data_ptr(), nrhs, ldx)
    torch.cuda.synchronize()
    assert plan.solve_status() == 0
    nl = int(plan.solve_levels().max()) + 1
    assert nl >= 3
    seen, routed = Counter(), Counter()
    for k, lev in enumerate(range(nl) if forward else range(nl - 1, -1, -1)):
        first, last = k == 0, k == nl - 1
        api.reset_kernel_launches()
        plan.solve_levels_device(Ld.data_ptr(), Xd.data_ptr(), nrhs, ldx, 0, lev, lev + 1, first, last, backward=not forward)
        torch.cuda.synchronize()
        step = Counter({name: v for name, v in api.kernel_launches().items() if v})
        route = Counter(V.route_levels(plan, nrhs, ldx, forward, lev, lev + 1, first, last))
        assert step == route, f"level {lev}: launched {dict(step)}, the route says {dict(route)}"
        seen += step
        routed += route
    assert plan.solve_status() == 0
    print(f"LEVELS {direction} nrhs={nrhs} levels={nl} launched={dict(seen)}")
    assert seen == routed and sum(seen.values()) > nl
    X, Y = Xd.cpu().numpy(), Yd.cpu().numpy()
    if forward:
        err = np.abs(X - Y).max() / max(1.0, np.abs(Y).max())
        print(f"LEVELS forward nrhs={nrhs} err={err:.3e}")
        assert err <= SOLVE_TOL, err
        body = X[:ldx * nrhs].reshape(nrhs, ldx)
        assert np.array_equal(_bits(body[:, n:]), _bits(np.full((nrhs, _PAD), _SENTINEL))) and np.array_equal(_bits(X[ldx * nrhs:]), _bits(np.full(_TAIL, _SENTINEL)))
    else:
        assert np.array_equal(_bits(X), _bits(Y)), "the backward solve in steps of levels differs from the one-call solve"


def test_prediction_is_the_witness(api, monkeypatch):
    """solve_cases.predict, which pins the cells to their paths without a GPU (test_solve_cases_host.py), names exactly the
    solve entries every cell's solve launched."""
    wrong = []
    for name in NAMES:
        cell = V.CELL_BY_NAME[name]
        if name == "rhs_ones":
            continue
        got = _result(api, monkeypatch, name)
        plan = _plan(api, monkeypatch, cell)["plan"]
        pred = V.predict(plan.info, V.launch_tables(plan), cell.plan_env, cell.solve_env, cell.nrhs, cell.forward)
        for scaled in (False, True):
            seen = {k for k in SOLVE_ENTRIES if got["seen"][scaled][k]}
            if seen != pred:
                wrong.append((name, scaled, "launched, not predicted:", sorted(seen - pred), "predicted, not launched:", sorted(pred - seen)))
    assert not wrong, wrong


def test_solve_coverage_reaches_every_solve_kernel(api, monkeypatch):
    """The union of the witnesses over the catalogue covers every solve entry of the witness table but k_copy_segments
    (the multi-device exchange's copy, bitwise in test_gpu_parity.py) -- k_solve_chain_w<4> included."""
    union = dict.fromkeys(SOLVE_ENTRIES, 0)
    for name in NAMES:
        for seen in _result(api, monkeypatch, name)["seen"].values():
            for k in SOLVE_ENTRIES:
                union[k] += seen[k]
    print("WITNESS " + " ".join(f"{k}={v}" for k, v in union.items()))
    missing = sorted(k for k, v in union.items() if v == 0 and k != "k_copy_segments")
    assert not missing, f"solve kernels no cell reached: {missing}"
    assert union["k_solve_chain_w<4>"] > 0
