"""The eigensolver on the CPU tier: the input conditions of tests/test_eigs_gpu.py checked with the numpy restatement
(eigs_ref.py), the small dense helpers (csrc/eigs_dense.hpp) under the host sanitizers, and what a host-only plan
answers.

Input condition: for every configuration the GPU tier runs -- input x M in {I, mass} x (k, block, max_basis), the exact
factor at tol 1e-10 and 1e-12, the factor of A under the values of A + D at 1e-10 -- the restatement converges in at most
max_iter / 2 = 100 iterations and its pairs meet the GPU tier's own bounds against numpy eigh."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

import eigs_ref as E
from conftest import problem

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "parsy_bench_amd" / "csrc"


def _converges(c, cfg, mass, tol, stale, what):
    k, block, mb = cfg
    Ad = c["Ast"] if stale else c["Ad"]
    Md = c["Md"] if mass else None
    n = Ad.shape[0]
    lam, Y, resid, info = E.eigs(Ad, Md, c["Kinv"], E.start_block(n, block), k, tol, mb)
    assert info["nconv"] == k and info["iterations"] <= E.MAX_ITER // 2, f"{what}: {info}"
    assert (resid <= tol).all() and info["basis"] <= mb
    eta, bound, orth = E.measures(Ad, Md, lam, Y)
    assert (eta <= resid + (c["max_row"] + 1) * E.U).all(), what
    lerr = np.abs(lam - E.spectrum(c, stale, mass)[:k])
    limit = bound + E.reference_error(Ad, Md, lam)
    assert (lerr <= limit).all(), f"{what}: |lambda - ref| {lerr} against {limit}"
    assert orth <= n * E.U * E.kappa_m(Md), what
    return info["iterations"], float((lerr / limit).max()), orth / (n * E.U * E.kappa_m(Md))


@pytest.mark.parametrize("name", E.INPUTS)
def test_input_conditions(name):
    c = E.dense_case(name)
    n = c["sym"].n
    assert 144 <= n <= 694 and (n % 64 != 0 or name == "grid8x8x8")
    worst = (0, 0.0, 0.0)
    for cfg, mass in E.runs():
        for tol, stale in [(t, False) for t in E.TOLS] + [(1e-10, True)]:
            got = _converges(c, cfg, mass, tol, stale, f"{name} {cfg} mass={mass} tol={tol:g} stale={stale}")
            worst = tuple(max(a, b) for a, b in zip(worst, got))
    print(f"{name}: most iterations {worst[0]}, lambda error / bound {worst[1]:.2e}, orthonormality / bound {worst[2]:.2e}")


def test_the_12x12_grid_has_double_eigenvalues():
    """Multiplicities 1, 2, 1, 2, 2, 1, 2 from the bottom: k = 5 cuts a pair, k = 6 and k = 9 end on whole clusters."""
    lam = E.spectrum(E.dense_case("grid12x12"), False, False)
    gap = np.diff(lam[:11]) > 1e-9 * lam[0]
    assert gap[5] and not gap[4] and gap[8] and not gap[1] and not gap[6]


def test_restatement_drops_and_reports():
    c = E.dense_case("grid12x12")
    n = c["sym"].n
    X0 = E.start_block(n, 4)
    X0[:, 2] = X0[:, 0]   # a dependent start column is dropped, the call still converges
    lam, Y, resid, info = E.eigs(c["Ad"], None, c["Kinv"], X0, 3, 1e-10, 24)
    assert info["dropped"] >= 1 and info["nconv"] == 3
    bad = c["Md"].copy()
    bad[n // 2, n // 2] = -1e6
    with pytest.raises(E.NotSpd, match="iteration"):
        E.eigs(c["Ad"], bad, c["Kinv"], E.start_block(n, 4), 6, 1e-10, 24)
    # max_iter = 2: the current Ritz pairs with their true eta
    lam, Y, resid, info = E.eigs(c["Ad"], c["Md"], c["Kinv"], E.start_block(n, 4), 6, 1e-12, 24, max_iter=2)
    assert info["iterations"] == 2 and info["nconv"] < 6 and info["basis"] == 12
    eta, _, orth = E.measures(c["Ad"], c["Md"], lam, Y)
    assert np.allclose(eta, resid, rtol=1e-6, atol=(c["max_row"] + 1) * E.U) and orth <= n * E.U * E.kappa_m(c["Md"])


def test_dense_helpers_under_the_sanitizers(tmp_path):
    from parsy_bench_amd.build import _hipcc
    exe = tmp_path / "eigs_dense_check"
    # (the sanitizers are for the host compilation only: -Xarch_host keeps them off any device pass of the driver)
    cmd = [_hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-g", "-O1", f"-I{CSRC}", str(ROOT / "tests" / "eigs_dense_check.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "eigs_dense: all checks passed" in ran.stdout and "m=128" in ran.stdout


def test_eigs_info_size():
    from parsy_bench_amd import _native as N
    assert ctypes.sizeof(N.EigsInfo) == 40


def test_host_only_plan_refuses_and_reports_zeros():
    from parsy_bench_amd import api
    A, perm, sym = problem("tiny2d")
    plan = api.Plan(sym, -1)
    n = sym.n
    zeros = dict(iterations=0, restarts=0, nconv=0, basis=0, dropped=0, solve_columns=0, device_bytes=0)
    assert plan.eigs_info == zeros
    lam, resid = np.full(2, 7.0), np.full(2, 7.0)
    with pytest.raises(RuntimeError, match="without a device"):
        plan.eigs_device(1, 0, 1, 2, 1, n, 2, 1, n, lam=lam, resid=resid)
    with pytest.raises(RuntimeError, match="without a device"):
        plan.eigs(sym.A2x, np.zeros(int(sym.xsize)), 2)
    with pytest.raises(RuntimeError, match="null argument"):
        plan.eigs_device(0, 0, 1, 2, 1, n, 2, 1, n, lam=lam, resid=resid)
    assert (lam == 7.0).all() and (resid == 7.0).all() and plan.eigs_info == zeros
