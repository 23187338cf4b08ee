"""Selected inversion on the engineered block-column shapes of selinv_ref.py (the -m gpu tier).

Both kernel paths and their mixes (PARSY_SELINV_TILED_MIN unset, 33, 64, 65, 10^9), each shape with its own values and
under a bad symmetric scaling D A D (D = diag(2^k), |k| <= 20), with the device's own factor:

* Z against the extended-precision inverse in the measure of selinv_ref.measure (units of u = 2^-53, relative to
  sqrt(Zx_ii Zx_jj), over the pattern of L): at most 4 times what the plain numpy restatement of the recurrence gives on
  the same values.  Both make the same products per entry and differ in the order of the sums and in fma; 4 is the margin
  test_updown_gpu / test_rowmod_gpu give their restatements.  The restatement itself is held below 64 u on the CPU tier.
* the diagonal of the inverse (from the same call, and through parsy_inverse_diag_device in both orderings): the same
  bound and the same bits as Z's diagonal.
* every entry of the xsize buffer written, nothing behind it touched.
* homogeneity: Z(D A D) == D^-1 Z(A) D^-1 bitwise, per threshold.
* log det against 2 sum log L_jj in long double from the device's own factor diagonal, relative to the sum of magnitudes.
* bitwise reproducibility across calls, plans and changes of the threshold.

Every measured value is printed on a RHO_SELINV line (pytest -rP shows it for passing tests).
"""
import numpy as np
import pytest

import selinv_ref as R
import shape_cases as SC
from parsy_bench_amd import inspector as I
from test_selinv_gpu import _dev, _diag_offsets
from test_selinv_host import block_columns

pytestmark = pytest.mark.gpu

NAMES = list(R.SHAPES)
THRESHOLDS = [None, "33", "64", "65", "1000000000"]
_SENTINEL = -7.25e300
_TAIL = 11
_RUNS = {}
_Z = {}


def _set_threshold(monkeypatch, threshold):
    if threshold is None:
        monkeypatch.delenv("PARSY_SELINV_TILED_MIN", raising=False)
    else:
        monkeypatch.setenv("PARSY_SELINV_TILED_MIN", threshold)


def _run(api, monkeypatch, name):
    """One plan per shape, both value sets factored once through it.  Made once, never changed."""
    if name not in _RUNS:
        ref = R.reference(name)
        sym = ref["sym"]
        SC.set_env(monkeypatch, {})
        plan = api.Plan(sym, 0)
        run = {"sym": sym, "plan": plan, "ref": ref}
        for scaled in (False, True):
            lv, _ = plan.factor(R.values(name, scaled))
            assert plan.status() == 0, f"{name} scaled={scaled}: factor status {plan.status()}"
            run[scaled] = lv
        _RUNS[name] = run
    return _RUNS[name]


def _selinv(api, monkeypatch, name, scaled, threshold):
    """(z, diag, Z dense, tiled block columns, block columns) of plan.selinv under a threshold: one call per
    (shape, values, threshold), shared by the tests and left unchanged."""
    key = (name, scaled, threshold)
    if key not in _Z:
        run = _run(api, monkeypatch, name)
        _set_threshold(monkeypatch, threshold)
        run["plan"].set_perm(None)
        z, diag, _ = run["plan"].selinv(run[scaled])
        info = run["plan"].selinv_info
        _Z[key] = (z, diag, I.bcsc_to_dense(run["sym"], z), info["tiled_block_columns"], info["block_columns"])
    return _Z[key]


def _is_sentinel(a):
    return np.ascontiguousarray(a).view(np.int64) == np.float64(_SENTINEL).view(np.int64)


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("name", NAMES)
def test_inverse_on_engineered_shape(api, monkeypatch, name, scaled, threshold):
    run = _run(api, monkeypatch, name)
    sym, ref = run["sym"], run["ref"]
    z, diag, Zd, ntiled, nbc = _selinv(api, monkeypatch, name, scaled, threshold)
    t = 0 if threshold is None else int(threshold)
    assert ntiled == sum(1 for *_, m in block_columns(sym) if m >= t) and nbc == len(block_columns(sym))
    rho_ref = ref["rho"][scaled][0]
    assert 0 < rho_ref <= R.REF_CAP
    rho, (i, j) = R.measure(Zd, ref["Zx"][scaled], ref["mask"])
    s, b, wb, m = R.block_column_of(sym, j)
    print(f"RHO_SELINV shape={name} scaled={int(scaled)} threshold={threshold} tiled={ntiled}/{nbc} device={rho:.3f} "
          f"reference={rho_ref:.3f} limit={R.MARGIN * rho_ref:.3f} worst=({i},{j}) supernode={s} block_column={b} wb={wb} m={m}")
    assert np.isfinite(z).all()
    assert rho <= R.MARGIN * rho_ref, (f"{name} scaled={scaled} threshold={threshold}: device {rho:.4g} u > 4 x reference "
                                       f"{rho_ref:.4g} u at ({i}, {j}): supernode {s}, block column {b}, wb={wb}, m={m}")
    assert not Zd[np.triu_indices(sym.n, 1)].any(), f"{name}: a non-zero above the diagonal"
    # the diagonal from the same call: the same bits as Z's diagonal, hence the same bound
    assert np.array_equal(diag.view(np.int64), z[_diag_offsets(sym)].view(np.int64))
    zx = np.diag(ref["Zx"][scaled])
    derr = np.abs(diag.astype(np.longdouble) - zx)
    assert (derr <= R.MARGIN * rho_ref * np.longdouble(R.U) * zx).all(), (name, scaled, threshold)


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("name", NAMES)
def test_inverse_diag_in_both_orderings(api, monkeypatch, name, scaled):
    """parsy_inverse_diag_device under set_perm(sym.Perm) and set_perm(None): a gather of Z's diagonal, bit for bit, within
    4 x (reference measure) u Zx_ii of the extended inverse's diagonal; nothing written behind the n entries."""
    import torch
    run = _run(api, monkeypatch, name)
    sym, plan, ref = run["sym"], run["plan"], run["ref"]
    n = sym.n
    z, _, _, _, _ = _selinv(api, monkeypatch, name, scaled, None)
    zx = np.diag(ref["Zx"][scaled])
    limit = R.MARGIN * ref["rho"][scaled][0] * np.longdouble(R.U) * zx
    Zdev = _dev(z)
    P = np.asarray(sym.Perm)
    try:
        for perm in (P, None):
            Dd = _dev(np.full(n + _TAIL, _SENTINEL))
            plan.set_perm(perm)
            plan.inverse_diag_device(Zdev.data_ptr(), Dd.data_ptr())
            torch.cuda.synchronize()
            out = Dd.cpu().numpy()
            got = out[:n][P] if perm is not None else out[:n]   # (out[Perm[i]] = Z_ii in the factor's ordering)
            assert np.array_equal(got.view(np.int64), z[_diag_offsets(sym)].view(np.int64))
            assert (np.abs(got.astype(np.longdouble) - zx) <= limit).all()
            assert _is_sentinel(out[n:]).all()
    finally:
        plan.set_perm(None)


@pytest.mark.parametrize("threshold", ["0", "64", "1000000000"])
@pytest.mark.parametrize("name", NAMES)
def test_every_entry_has_a_writer_and_nothing_else_is_written(api, monkeypatch, name, threshold):
    import torch
    run = _run(api, monkeypatch, name)
    sym, plan = run["sym"], run["plan"]
    xs = int(sym.xsize)
    _set_threshold(monkeypatch, threshold)
    Ld = _dev(run[False])
    Zd = torch.full((xs + _TAIL,), _SENTINEL, dtype=torch.float64, device="cuda")
    plan.selinv_device(Ld.data_ptr(), Zd.data_ptr())
    torch.cuda.synchronize()
    out = Zd.cpu().numpy()
    unwritten = np.nonzero(_is_sentinel(out[:xs]))[0]
    assert unwritten.size == 0, f"{name} threshold={threshold}: {unwritten.size} entries unwritten, first at {unwritten[0]}"
    assert _is_sentinel(out[xs:]).all(), f"{name} threshold={threshold}: a write behind the xsize entries"
    assert np.array_equal(Ld.cpu().numpy().view(np.int64), run[False].view(np.int64))
    # the same bits as the host-buffer call
    z = _selinv(api, monkeypatch, name, False, threshold if threshold != "0" else None)[0]
    assert np.array_equal(out[:xs].view(np.int64), z.view(np.int64))


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("name", NAMES)
def test_inverse_is_homogeneous_under_scaling(api, monkeypatch, name, threshold):
    """Z(D A D) == D^-1 Z(A) D^-1 bitwise, D = diag(2^k): the factor is homogeneous (test_factor_shapes_gpu.py), and every
    operation of either path is a product, a fused multiply-add of terms that carry the same power of two, or a division
    by a scaled pivot (tinv64, mm16 / mm64, write_diag_block, the small path's chains)."""
    run = _run(api, monkeypatch, name)
    d = run["ref"]["d"]
    Ld = [I.bcsc_to_dense(run["sym"], run[s]) for s in (False, True)]
    assert np.array_equal(Ld[1], d[:, None] * Ld[0]), "the factor itself is not homogeneous"
    want = _selinv(api, monkeypatch, name, False, threshold)[2] / (d[:, None] * d[None, :])
    got = _selinv(api, monkeypatch, name, True, threshold)[2]
    diff = int((want != got).sum())
    print(f"SCALING_SELINV shape={name} threshold={threshold} entries_that_differ={diff}")
    assert diff == 0, f"{name} threshold={threshold}: {diff} entries differ; first at {np.argwhere(want != got)[0]}"


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("name", NAMES)
def test_logdet_on_engineered_shape(api, monkeypatch, name, scaled):
    """Against 2 sum log L_jj in long double from the device's own factor diagonal.  One rounding per addition (n of them,
    in any order) and two for each logarithm (its own and the doubling's place in the sum): (n + 2) u sum |2 log L_jj|,
    relative to the sum of magnitudes because the logarithms of scaled pivots cancel."""
    run = _run(api, monkeypatch, name)
    sym, plan = run["sym"], run["plan"]
    lv = run[scaled]
    logs = 2 * np.log(lv[_diag_offsets(sym)].astype(np.longdouble))
    want, mag = logs.sum(), np.abs(logs).sum()
    got, col = plan.logdet_device(_dev(lv).data_ptr())
    assert col == 0
    bound = (sym.n + 2) * np.longdouble(R.U) * mag
    err = abs(np.longdouble(got) - want)
    print(f"LOGDET shape={name} scaled={int(scaled)} logdet={got:.6f} sum_of_magnitudes={float(mag):.3f} "
          f"err={float(err):.3e} bound={float(bound):.3e}")
    assert err <= bound, (name, scaled, float(err), float(bound))


def test_reproducible_across_calls_plans_and_thresholds(api, monkeypatch):
    """`edges` under threshold 64 (both paths on a level): two calls on one plan and one on a second plan; then on one
    plan 0 -> 10^9 -> 0, the third call bitwise the first (the split is made again when the threshold changes)."""
    import torch
    run = _run(api, monkeypatch, "edges")
    sym, plan = run["sym"], run["plan"]
    xs = int(sym.xsize)
    Ld = _dev(run[False])

    def call(p):
        Zd = torch.full((xs,), _SENTINEL, dtype=torch.float64, device="cuda")
        p.selinv_device(Ld.data_ptr(), Zd.data_ptr())
        torch.cuda.synchronize()
        return Zd.cpu().numpy().view(np.int64)

    _set_threshold(monkeypatch, "64")
    plan2 = api.Plan(sym, 0)
    try:
        a, b, c = call(plan), call(plan), call(plan2)
        assert np.array_equal(a, b) and np.array_equal(a, c)
        outs = []
        for t in ("0", "1000000000", "0"):
            _set_threshold(monkeypatch, t)
            outs.append(call(plan2))
            assert plan2.selinv_info["tiled_block_columns"] == (0 if t != "0" else plan2.selinv_info["block_columns"])
        assert np.array_equal(outs[0], outs[2])
        _set_threshold(monkeypatch, "64")
        assert np.array_equal(call(plan2), a)
    finally:
        plan2.close()
