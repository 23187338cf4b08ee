"""Host-side mirror of the reference's operator interface for the hot path.

Two layers, both thin ctypes shims over libparsy_amd.so (the C ABI in
include/parsy_amd.h) -- no numerics happen in Python:

* the drop-in operators, with the reference's names, argument order and return
  values (cholesky/parallel_PB_Cholesky_05.h:27, Parallel_PB_Cholesky_wavefront.h:10,
  triangularSolve/Triangular_BCSC.h:14/115/171/238), taking numpy arrays where the
  reference takes raw pointers;
* `Plan`, the pattern-resident handle API (device pointers in/out) used by
  bench.py and by multi-GPU sharding.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N

KIND_NAMES = ["SMALL", "TILES", "CHAIN", "BIG", "BACK_BELOW", "SOLVE_SMALL", "SOLVE_PANEL", "SOLVE_FIXUP", "BACK_BLOCK", "DENSE"]


def device_count() -> int:
    return int(N.lib().parsy_device_count())


def kernel_launches() -> dict:
    """Kernel witness: launches enqueued per solve kernel instantiation since the last reset (process-wide),
    name -> count, every entry of the library's table (zero included)."""
    lib = N.lib()
    return {lib.parsy_debug_kernel_name(k).decode(): int(lib.parsy_debug_kernel_launches(k))
            for k in range(lib.parsy_debug_kernel_count())}


def reset_kernel_launches() -> None:
    N.lib().parsy_debug_kernel_reset()


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _sz(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


# ---------------------------------------------------------------------------
# drop-in operators (host arrays in, host arrays out)
# ---------------------------------------------------------------------------
def cholesky_left_par_05(n, c, r, values, lC, lR, Li_ptr, lValues, blockSet, supNo, timing, aTree,
                         cT, rT, col2Sup, nLevels, levelPtr, levelSet, nPar, parPtr, partition,
                         chunk, threads, super_max, col_max, nodCost=None) -> bool:
    """lValues (zeroed by the caller) receives the factor; returns False on a
    non-positive pivot or if the HIP path could not run."""
    assert lValues.dtype == np.float64 and lValues.flags["C_CONTIGUOUS"]
    a = [_i32(c), _i32(r), _f64(values), _sz(lC), _i32(lR), _sz(Li_ptr), _i32(blockSet), _i32(aTree),
         _i32(cT), _i32(rT), _i32(col2Sup), _i32(levelPtr), _i32(parPtr), _i32(partition)]
    ls = None if levelSet is None else _i32(levelSet)
    return bool(N.lib().cholesky_left_par_05(
        n, N.ptr(a[0]), N.ptr(a[1]), N.ptr(a[2]), N.ptr(a[3]), N.ptr(a[4]), N.ptr(a[5]), N.ptr(lValues),
        N.ptr(a[6]), supNo, N.ptr(timing), N.ptr(a[7]), N.ptr(a[8]), N.ptr(a[9]), N.ptr(a[10]), nLevels,
        N.ptr(a[11]), N.ptr(ls), nPar, N.ptr(a[12]), N.ptr(a[13]), chunk, threads, super_max, col_max,
        None))


def cholesky_left_par_05_prune(n, c, r, values, lC, lR, Li_ptr, lValues, blockSet, supNo, timing, prunePtr,
                               pruneSet, nLevels, levelPtr, levelSet, nPar, parPtr, partition, chunk, threads,
                               super_max, col_max, nodCost=None) -> bool:
    """The reference's PRUNE build of cholesky_left_par_05: update lists instead of etree + upper pattern."""
    assert lValues.dtype == np.float64 and lValues.flags["C_CONTIGUOUS"]
    a = [_i32(c), _i32(r), _f64(values), _sz(lC), _i32(lR), _sz(Li_ptr), _i32(blockSet), _i32(prunePtr),
         _i32(pruneSet), _i32(levelPtr), _i32(parPtr), _i32(partition)]
    ls = None if levelSet is None else _i32(levelSet)
    return bool(N.lib().cholesky_left_par_05_prune(
        n, N.ptr(a[0]), N.ptr(a[1]), N.ptr(a[2]), N.ptr(a[3]), N.ptr(a[4]), N.ptr(a[5]), N.ptr(lValues),
        N.ptr(a[6]), supNo, N.ptr(timing), N.ptr(a[7]), N.ptr(a[8]), nLevels, N.ptr(a[9]), N.ptr(ls), nPar,
        N.ptr(a[10]), N.ptr(a[11]), chunk, threads, super_max, col_max, None))


def cholesky_left_par_waveFront(n, c, r, values, lC, lR, Li_ptr, lValues, blockSet, supNo, timing,
                                aTree, cT, rT, col2Sup, nLevels, levelPtr, levelSet, chunk, threads,
                                super_max, col_max) -> bool:
    assert lValues.dtype == np.float64 and lValues.flags["C_CONTIGUOUS"]
    a = [_i32(c), _i32(r), _f64(values), _sz(lC), _i32(lR), _sz(Li_ptr), _i32(blockSet), _i32(aTree),
         _i32(cT), _i32(rT), _i32(col2Sup), _i32(levelPtr), _i32(levelSet)]
    return bool(N.lib().cholesky_left_par_waveFront(
        n, N.ptr(a[0]), N.ptr(a[1]), N.ptr(a[2]), N.ptr(a[3]), N.ptr(a[4]), N.ptr(a[5]), N.ptr(lValues),
        N.ptr(a[6]), supNo, N.ptr(timing), N.ptr(a[7]), N.ptr(a[8]), N.ptr(a[9]), N.ptr(a[10]), nLevels,
        N.ptr(a[11]), N.ptr(a[12]), chunk, threads, super_max, col_max))


def _solve_base(n, Lp, Li, Lx, NNZ, Li_ptr, col2sup, sup2col, supNo, x):
    assert x is None or (x.dtype == np.float64 and x.flags["C_CONTIGUOUS"])
    keep = [None if Lp is None else _sz(Lp), None if Li is None else _i32(Li), _f64(Lx), _sz(Li_ptr),
            _i32(col2sup), _i32(sup2col)]
    return keep, (n, N.ptr(keep[0]), N.ptr(keep[1]), N.ptr(keep[2]), int(NNZ), N.ptr(keep[3]),
                  N.ptr(keep[4]), N.ptr(keep[5]), supNo, N.ptr(x))


def blockedLsolve(n, Lp, Li, Lx, NNZ, Li_ptr, col2sup, sup2col, supNo, x) -> int:
    keep, base = _solve_base(n, Lp, Li, Lx, NNZ, Li_ptr, col2sup, sup2col, supNo, x)
    return int(N.lib().blockedLsolve(*base))


def leveledBlockedLsolve(n, Lp, Li, Lx, NNZ, Li_ptr, col2sup, sup2col, supNo, x, levels, levelPtr,
                         levelSet, chunk) -> int:
    keep, base = _solve_base(n, Lp, Li, Lx, NNZ, Li_ptr, col2sup, sup2col, supNo, x)
    lp, ls = _i32(levelPtr), _i32(levelSet)
    return int(N.lib().leveledBlockedLsolve(*base, levels, N.ptr(lp), N.ptr(ls), chunk))


def H2LeveledBlockedLsolve(n, Lp, Li, Lx, NNZ, Li_ptr, col2sup, sup2col, supNo, x, levels, levelPtr,
                           levelSet, parts, parPtr, partition, chunk) -> int:
    keep, base = _solve_base(n, Lp, Li, Lx, NNZ, Li_ptr, col2sup, sup2col, supNo, x)
    lp, pp, pt = _i32(levelPtr), _i32(parPtr), _i32(partition)
    ls = None if levelSet is None else _i32(levelSet)
    return int(N.lib().H2LeveledBlockedLsolve(*base, levels, N.ptr(lp), N.ptr(ls), parts, N.ptr(pp),
                                              N.ptr(pt), chunk))


def H2LeveledBlockedLsolve_Peeled(n, Lp, Li, Lx, NNZ, Li_ptr, col2sup, sup2col, supNo, x, levels,
                                  levelPtr, levelSet, parts, parPtr, partition, chunk, threads) -> int:
    keep, base = _solve_base(n, Lp, Li, Lx, NNZ, Li_ptr, col2sup, sup2col, supNo, x)
    lp, pp, pt = _i32(levelPtr), _i32(parPtr), _i32(partition)
    ls = None if levelSet is None else _i32(levelSet)
    return int(N.lib().H2LeveledBlockedLsolve_Peeled(*base, levels, N.ptr(lp), N.ptr(ls), parts,
                                                     N.ptr(pp), N.ptr(pt), chunk, threads))


def blockedPrunedLSolve(n, Lp, Li, Lx, NNZ, Li_ptr, BPSet, PBSetSize, sup2col, supNo, x) -> int:
    """The reference's pruned forward solve (Triangular_BCSC.h:55): L x = b on the supernodes of BPSet alone, numbered
    1 .. supNo as the reference's loop reads sup2col; x changes only in their columns.  0 (loudly) for a list that is
    not closed towards the root."""
    assert x is None or (x.dtype == np.float64 and x.flags["C_CONTIGUOUS"])
    keep = [None if Lp is None else _sz(Lp), None if Li is None else _i32(Li), _f64(Lx), _sz(Li_ptr), _i32(BPSet),
            _i32(sup2col)]
    return int(N.lib().blockedPrunedLSolve(n, N.ptr(keep[0]), N.ptr(keep[1]), N.ptr(keep[2]), int(NNZ), N.ptr(keep[3]),
                                           N.ptr(keep[4]), int(PBSetSize), N.ptr(keep[5]), supNo, N.ptr(x)))


def dropin_reset() -> None:
    N.lib().parsy_dropin_reset()


# ---------------------------------------------------------------------------
# plan API
# ---------------------------------------------------------------------------
class Plan:
    """Pattern + launch schedule resident on one device (parsy_plan)."""

    def __init__(self, sym, device: int = 0):
        lib = N.lib()
        self.sym = sym
        self.device = device
        if getattr(sym, "_handle", None):
            h = lib.parsy_plan_from_symbolic(sym._handle, device)
        else:
            a = [_i32(sym.super), _sz(sym.p), _sz(sym.i_ptr), _i32(sym.s), _i32(sym.sParent),
                 _i32(sym.col2Sup), _i32(sym.A1p), _i32(sym.A1i), _i32(sym.A2p), _i32(sym.A2i)]
            h = lib.parsy_plan_create(sym.n, sym.nsuper, *[N.ptr(v) for v in a], device)
        if not h:
            raise RuntimeError("parsy_plan_create failed: " + N.last_error())
        self._h = h

    def close(self):
        h, self._h = self._h, None
        if h:
            N.lib().parsy_plan_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def info(self) -> dict:
        pi = N.PlanInfo()
        N.lib().parsy_plan_get_info(self._h, C.byref(pi))
        return pi.as_dict()

    def set_active(self, mask) -> None:
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        if N.lib().parsy_plan_set_active(self._h, N.ptr(m)) != 0:
            raise RuntimeError(N.last_error())

    # host-buffer conveniences -------------------------------------------------
    def factor(self, values, out=None):
        """Returns (lValues, device_seconds). Raises on a HIP failure; check `status()`.  out: a float64 array of
        xsize entries to receive lValues (every entry is written)."""
        vals = _f64(values)
        lValues = np.zeros(int(self.sym.xsize), dtype=np.float64) if out is None else out
        assert lValues.dtype == np.float64 and lValues.size == int(self.sym.xsize) and lValues.flags.c_contiguous
        sec = C.c_double(0)
        if N.lib().parsy_factor_host(self._h, N.ptr(vals), N.ptr(lValues), C.byref(sec)) != 0:
            raise RuntimeError("parsy_factor_host failed: " + N.last_error())
        return lValues, sec.value

    def status(self) -> int:
        return int(N.lib().parsy_factor_status(self._h))

    def solve_status(self) -> int:
        """0 = the last solve on this plan completed; -1 = a hand-off wait inside it timed out."""
        return int(N.lib().parsy_solve_status(self._h))

    def solve(self, lValues, b):
        """Forward solve; b is (n,) or (n, nrhs) (any layout); returns x of the same shape."""
        b = np.asarray(b, dtype=np.float64)
        one = b.ndim == 1
        X = np.asfortranarray(b.reshape(self.sym.n, -1)).copy(order="F")
        nrhs = X.shape[1]
        lv = _f64(lValues)
        sec = C.c_double(0)
        rc = N.lib().parsy_solve_host(self._h, N.ptr(lv), X.ctypes.data_as(C.c_void_p), nrhs,
                                      self.sym.n, C.byref(sec))
        if rc != 0:
            raise RuntimeError("parsy_solve_host failed: " + N.last_error())
        return (X[:, 0].copy() if one else np.ascontiguousarray(X)), sec.value

    def solve2(self, lValues, b, forward: bool = True):
        """Backward solve L' x = y (forward=False) or the full L L' x = b (forward=True) of the
        PERMUTED system; returns (x, device_seconds)."""
        b = np.asarray(b, dtype=np.float64)
        one = b.ndim == 1
        X = np.asfortranarray(b.reshape(self.sym.n, -1)).copy(order="F")
        lv = _f64(lValues)
        sec = C.c_double(0)
        rc = N.lib().parsy_solve2_host(self._h, N.ptr(lv), X.ctypes.data_as(C.c_void_p), X.shape[1],
                                       self.sym.n, 1 if forward else 0, C.byref(sec))
        if rc != 0:
            raise RuntimeError("parsy_solve2_host failed: " + N.last_error())
        return (X[:, 0].copy() if one else np.ascontiguousarray(X)), sec.value

    def solve_spd(self, lValues, b):
        """x with A x = b for the ORIGINAL matrix: x = P' L'^-1 L^-1 P b (Perm from the inspector)."""
        b = np.asarray(b, dtype=np.float64)
        pb = b[self.sym.Perm] if b.ndim == 1 else b[self.sym.Perm, :]
        z, sec = self.solve2(lValues, pb, forward=True)
        x = np.empty_like(z)
        x[self.sym.Perm] = z
        return x, sec

    # A x = b in the caller's ordering: residuals, backward errors, iterative refinement (dporfs) -----------
    def set_perm(self, perm) -> None:
        """The caller's ordering (perm[new] = old, n entries) for residual_device / solve_spd_device; None: identity."""
        p = None if perm is None else _i32(perm)
        if p is not None and p.size != self.sym.n:
            raise ValueError(f"set_perm: perm has {p.size} entries, the plan has n = {self.sym.n}")
        if N.lib().parsy_plan_set_perm(self._h, N.ptr(p)) != 0:
            raise RuntimeError(N.last_error())

    def residual_device(self, d_values: int, d_x: int, ldx: int, d_b: int, ldb: int, nrhs: int, d_r: int = 0,
                        ldr: int = 0, stream: int = 0) -> np.ndarray:
        """R = B - A X (d_r: 0 for none) and the componentwise backward error of every column (returned)."""
        berr = np.zeros(nrhs, dtype=np.float64)
        if N.lib().parsy_residual_device(self._h, d_values, d_x, ldx, d_b, ldb, d_r or None, ldr, nrhs,
                                         N.ptr(berr), stream) != 0:
            raise RuntimeError("parsy_residual_device failed: " + N.last_error())
        return berr

    def solve_spd_device(self, d_values: int, d_lValues: int, d_b: int, ldb: int, d_x: int, ldx: int, nrhs: int,
                         max_steps: int = 5, stream: int = 0):
        """X = A^-1 B with up to max_steps refinement steps; returns (steps int32[nrhs], berr float64[nrhs])."""
        steps = np.zeros(nrhs, dtype=np.int32)
        berr = np.zeros(nrhs, dtype=np.float64)
        if N.lib().parsy_solve_spd_device(self._h, d_values, d_lValues, d_b, ldb, d_x, ldx, nrhs, max_steps,
                                          N.ptr(steps), N.ptr(berr), stream) != 0:
            raise RuntimeError("parsy_solve_spd_device failed: " + N.last_error())
        return steps, berr

    def solve_refined(self, values, lValues, b, max_steps: int = 5, bounds: bool = False):
        """x with A x = b for the ORIGINAL matrix (caller's ordering, like solve_spd), refined on the device against
        `values` (A2 order; they may differ from the values lValues was factored from).  On first use the plan takes
        sym.Perm as its ordering.  Returns (x, {"steps", "berr", "seconds"}); bounds=True adds "ferr", the forward error
        bound of every column (parsy_solve_spd_bounds_host)."""
        if not getattr(self, "_perm_set", False):
            self.set_perm(self.sym.Perm)
            self._perm_set = True
        b = np.asarray(b, dtype=np.float64)
        one = b.ndim == 1
        B = np.asfortranarray(b.reshape(self.sym.n, -1))
        nrhs = B.shape[1]
        X = np.zeros((self.sym.n, nrhs), order="F")
        vals, lv = _f64(values), _f64(lValues)
        steps = np.zeros(nrhs, dtype=np.int32)
        berr = np.zeros(nrhs, dtype=np.float64)
        sec = C.c_double(0)
        if bounds:
            ferr = np.zeros(nrhs, dtype=np.float64)
            if N.lib().parsy_solve_spd_bounds_host(self._h, N.ptr(vals), N.ptr(lv), B.ctypes.data_as(C.c_void_p),
                                                   self.sym.n, X.ctypes.data_as(C.c_void_p), self.sym.n, nrhs, max_steps,
                                                   N.ptr(steps), N.ptr(berr), N.ptr(ferr), C.byref(sec)) != 0:
                raise RuntimeError("parsy_solve_spd_bounds_host failed: " + N.last_error())
            x = X[:, 0].copy() if one else np.ascontiguousarray(X)
            return x, {"steps": steps, "berr": berr, "seconds": sec.value, "ferr": ferr}
        if N.lib().parsy_solve_spd_host(self._h, N.ptr(vals), N.ptr(lv), B.ctypes.data_as(C.c_void_p), self.sym.n,
                                        X.ctypes.data_as(C.c_void_p), self.sym.n, nrhs, max_steps, N.ptr(steps),
                                        N.ptr(berr), C.byref(sec)) != 0:
            raise RuntimeError("parsy_solve_spd_host failed: " + N.last_error())
        x = X[:, 0].copy() if one else np.ascontiguousarray(X)
        return x, {"steps": steps, "berr": berr, "seconds": sec.value}

    # forward error bounds (dporfs's FERR) and the reciprocal condition number (dpocon) ---------------------------
    @property
    def cond_info(self) -> dict:
        """applications (solve pairs of the last bounds / rcond call), columns, device_bytes (0 before the first call)."""
        ci = N.CondInfo()
        if N.lib().parsy_cond_get_info(self._h, C.byref(ci)) != 0:
            raise RuntimeError("parsy_cond_get_info failed: " + N.last_error())
        return ci.as_dict()

    def error_bounds_device(self, d_values: int, d_lValues: int, d_x: int, ldx: int, d_b: int, ldb: int, nrhs: int,
                            stream: int = 0):
        """(ferr, berr) of a given X (the plan's ordering, as residual_device takes it): the forward error bound and the
        componentwise backward error of every column."""
        ferr = np.zeros(max(nrhs, 0), dtype=np.float64)
        berr = np.zeros(max(nrhs, 0), dtype=np.float64)
        if N.lib().parsy_error_bounds_device(self._h, d_values or None, d_lValues or None, d_x or None, ldx, d_b or None,
                                             ldb, nrhs, N.ptr(ferr), N.ptr(berr), stream) != 0:
            raise RuntimeError("parsy_error_bounds_device failed: " + N.last_error())
        return ferr, berr

    def solve_spd_bounds_device(self, d_values: int, d_lValues: int, d_b: int, ldb: int, d_x: int, ldx: int, nrhs: int,
                                max_steps: int = 5, stream: int = 0):
        """solve_spd_device with the forward error bound of the returned X: (steps, berr, ferr)."""
        steps = np.zeros(nrhs, dtype=np.int32)
        berr = np.zeros(nrhs, dtype=np.float64)
        ferr = np.zeros(nrhs, dtype=np.float64)
        if N.lib().parsy_solve_spd_bounds_device(self._h, d_values, d_lValues, d_b, ldb, d_x, ldx, nrhs, max_steps,
                                                 N.ptr(steps), N.ptr(berr), N.ptr(ferr), stream) != 0:
            raise RuntimeError("parsy_solve_spd_bounds_device failed: " + N.last_error())
        return steps, berr, ferr

    def rcond_device(self, d_values: int, d_lValues: int, stream: int = 0):
        """(rcond, anorm): 1 / (||A||_1 est ||(L L')^-1||_1) and ||A||_1 of the values (dpocon)."""
        an, rc = C.c_double(0), C.c_double(0)
        if N.lib().parsy_rcond_device(self._h, d_values or None, d_lValues or None, C.byref(an), C.byref(rc), stream) != 0:
            raise RuntimeError("parsy_rcond_device failed: " + N.last_error())
        return rc.value, an.value

    def rcond(self, values, lValues):
        """Host arrays in: (rcond, anorm, device_seconds)."""
        vals, lv = _f64(values), _f64(lValues)
        an, rc, sec = C.c_double(0), C.c_double(0), C.c_double(0)
        if N.lib().parsy_rcond_host(self._h, N.ptr(vals), N.ptr(lv), C.byref(an), C.byref(rc), C.byref(sec)) != 0:
            raise RuntimeError("parsy_rcond_host failed: " + N.last_error())
        return rc.value, an.value, sec.value

    # the smallest eigenpairs of A v = lambda M v through the factor -------------------------------------------------
    @property
    def eigs_info(self) -> dict:
        """Of the last eigs call: iterations, restarts, nconv, basis, dropped, solve_columns; device_bytes (0 before the
        first device call)."""
        ei = N.EigsInfo()
        if N.lib().parsy_eigs_get_info(self._h, C.byref(ei)) != 0:
            raise RuntimeError("parsy_eigs_get_info failed: " + N.last_error())
        return ei.as_dict()

    def eigs_device(self, d_values: int, d_mvalues: int, d_lValues: int, k: int, d_x0: int, ldx0: int, block: int,
                    d_y: int, ldy: int, tol: float = 1e-10, max_basis: int = 0, max_iter: int = 200, stream: int = 0,
                    lam=None, resid=None):
        """parsy_eigs_device on device pointers (d_mvalues 0: M = I).  Returns (rc, lam, resid, nconv): rc 0, or -2 when
        M is not SPD; every other failure raises.  lam / resid: float64 arrays of k entries to receive the results
        (default: new ones)."""
        lam = np.zeros(max(k, 0), dtype=np.float64) if lam is None else lam
        resid = np.zeros(max(k, 0), dtype=np.float64) if resid is None else resid
        nconv = C.c_int32(0)
        rc = N.lib().parsy_eigs_device(self._h, d_values or None, d_mvalues or None, d_lValues or None, k, d_x0 or None,
                                       ldx0, block, tol, max_basis, max_iter, N.ptr(lam), d_y or None, ldy, N.ptr(resid),
                                       C.byref(nconv), stream)
        if rc not in (0, -2):
            raise RuntimeError("parsy_eigs_device failed: " + N.last_error())
        return rc, lam, resid, nconv.value

    def eigs(self, values, lValues, k: int, M=None, x0=None, tol: float = 1e-10, max_basis: int = 0, max_iter: int = 200):
        """The k smallest eigenpairs of A v = lambda M v for the ORIGINAL matrices (caller's ordering, like
        solve_refined; on first use the plan takes sym.Perm as its ordering).  values, M: A2 order (M None: the
        identity); lValues: the factor of `values` or of values nearby.  x0: the start block (n, block), block <= 16;
        None: numpy.random.default_rng(0).standard_normal((n, min(k, 8))).  Returns (lam, Y, info): lam ascending, Y
        (n, k) M-orthonormal, info = eigs_info plus "resid", "nconv" and "seconds".  Raises when M is not SPD."""
        if not getattr(self, "_perm_set", False):
            self.set_perm(self.sym.Perm)
            self._perm_set = True
        n = self.sym.n
        if x0 is None:
            x0 = np.random.default_rng(0).standard_normal((n, min(max(k, 1), 8)))
        X0 = np.asfortranarray(np.asarray(x0, dtype=np.float64).reshape(n, -1))
        vals, lv = _f64(values), _f64(lValues)
        mv = None if M is None else _f64(M)
        lam, resid = np.zeros(max(k, 0)), np.zeros(max(k, 0))
        Y = np.zeros((n, max(k, 0)), order="F")
        nconv, sec = C.c_int32(0), C.c_double(0)
        rc = N.lib().parsy_eigs_host(self._h, N.ptr(vals), N.ptr(mv), N.ptr(lv), k, X0.ctypes.data_as(C.c_void_p), n,
                                     X0.shape[1], tol, max_basis, max_iter, N.ptr(lam), Y.ctypes.data_as(C.c_void_p), n,
                                     N.ptr(resid), C.byref(nconv), C.byref(sec))
        if rc != 0:
            raise RuntimeError("parsy_eigs_host failed: " + N.last_error())
        info = self.eigs_info
        info.update(resid=resid, nconv=nconv.value, seconds=sec.value)
        return lam, np.ascontiguousarray(Y), info

    # selected inversion: entries of A^-1 on the pattern of L, and log det A ------------------------------------
    @property
    def selinv_info(self) -> dict:
        """levels, block_columns, tiled_block_columns (under the current PARSY_SELINV_TILED_MIN), launches, flops,
        device_bytes (0 before the first device call)."""
        si = N.SelinvInfo()
        if N.lib().parsy_selinv_get_info(self._h, C.byref(si)) != 0:
            raise RuntimeError("parsy_selinv_get_info failed: " + N.last_error())
        return si.as_dict()

    def selinv_check(self) -> int:
        """Violations of the selected inversion's schedule (0: none; N.last_error() names the first)."""
        return int(N.lib().parsy_selinv_check(self._h))

    def selinv(self, lValues):
        """Z = (P A P')^-1 on the pattern of L (lValues' layout) and diag(A^-1) in the plan's ordering
        (parsy_plan_set_perm); returns (Z, diag, device_seconds)."""
        lv = _f64(lValues)
        z = np.empty(int(self.sym.xsize), dtype=np.float64)
        diag = np.empty(self.sym.n, dtype=np.float64)
        sec = C.c_double(0)
        if N.lib().parsy_selinv_host(self._h, N.ptr(lv), N.ptr(z), N.ptr(diag), C.byref(sec)) != 0:
            raise RuntimeError("parsy_selinv_host failed: " + N.last_error())
        return z, diag, sec.value

    def selinv_device(self, d_lValues: int, d_z: int, stream: int = 0) -> None:
        if N.lib().parsy_selinv_device(self._h, d_lValues, d_z, stream) != 0:
            raise RuntimeError("parsy_selinv_device failed: " + N.last_error())

    def inverse_diag_device(self, d_z: int, d_diag: int, stream: int = 0) -> None:
        if N.lib().parsy_inverse_diag_device(self._h, d_z, d_diag, stream) != 0:
            raise RuntimeError("parsy_inverse_diag_device failed: " + N.last_error())

    def logdet_device(self, d_lValues: int, stream: int = 0):
        """(log det A, column): column 0, or the first 1-based column whose pivot is not positive and finite (NaN)."""
        out = C.c_double(0)
        rc = N.lib().parsy_logdet_device(self._h, d_lValues, C.byref(out), stream)
        if rc < 0:
            raise RuntimeError("parsy_logdet_device failed: " + N.last_error())
        return out.value, int(rc)

    # gradients with respect to the values of A (A2 order; symmetric parameterisation: include/parsy_amd.h) --------
    def pattern(self) -> dict:
        """The pattern of A as the plan sees it, per A2 entry: row, col (permuted coordinates, row >= col) and dst
        (its offset in lValues / Z)."""
        n = int(self.sym.nnzA)
        out = {"row": np.zeros(n, dtype=np.int32), "col": np.zeros(n, dtype=np.int32), "dst": np.zeros(n, dtype=np.int64)}
        if N.lib().parsy_plan_pattern(self._h, N.ptr(out["row"]), N.ptr(out["col"]), N.ptr(out["dst"])) != n:
            raise RuntimeError("parsy_plan_pattern failed: " + N.last_error())
        return out

    @property
    def grad_info(self) -> dict:
        """entries, offdiag_entries, device_bytes (0 before the first device call), last_lanes (lanes per entry of the
        last pattern_outer call: 0 none yet, 1 the direct kernel, 8 / 16 / 32 / 64)."""
        gi = N.GradInfo()
        if N.lib().parsy_grad_get_info(self._h, C.byref(gi)) != 0:
            raise RuntimeError("parsy_grad_get_info failed: " + N.last_error())
        return gi.as_dict()

    def pattern_outer_device(self, d_lam: int, ldl: int, d_x: int, ldx: int, nrhs: int, d_g: int, alpha: float = 1.0,
                             beta: float = 0.0, stream: int = 0) -> None:
        """g[q] = beta g[q] + alpha sum_k (lam[i,k] x[j,k] + lam[j,k] x[i,k]) (one term on the diagonal), vectors in the
        plan's ordering (set_perm)."""
        if N.lib().parsy_pattern_outer_device(self._h, d_lam or None, ldl, d_x or None, ldx, nrhs, alpha, beta,
                                              d_g or None, stream) != 0:
            raise RuntimeError("parsy_pattern_outer_device failed: " + N.last_error())

    def pattern_outer(self, lam, x, alpha: float = 1.0) -> np.ndarray:
        """Host arrays (n,) or (n, nrhs) in, the sampled product (nnzA, A2 order) out."""
        Lm = np.asfortranarray(np.asarray(lam, dtype=np.float64).reshape(self.sym.n, -1))
        X = np.asfortranarray(np.asarray(x, dtype=np.float64).reshape(self.sym.n, -1))
        if Lm.shape != X.shape:
            raise ValueError(f"pattern_outer: lam is {Lm.shape}, x is {X.shape}")
        g = np.empty(int(self.sym.nnzA), dtype=np.float64)
        if N.lib().parsy_pattern_outer_host(self._h, Lm.ctypes.data_as(C.c_void_p), self.sym.n,
                                            X.ctypes.data_as(C.c_void_p), self.sym.n, X.shape[1], alpha, 0.0, N.ptr(g),
                                            None) != 0:
            raise RuntimeError("parsy_pattern_outer_host failed: " + N.last_error())
        return g

    def inverse_pattern_device(self, d_z: int, d_g: int, alpha: float = 1.0, beta: float = 0.0, plain: bool = False,
                               stream: int = 0) -> None:
        """g[q] = beta g[q] + alpha w_q Z[dst[q]] (w_q = 2 off the diagonal unless plain)."""
        if N.lib().parsy_inverse_pattern_device(self._h, d_z or None, alpha, beta, 1 if plain else 0, d_g or None,
                                                stream) != 0:
            raise RuntimeError("parsy_inverse_pattern_device failed: " + N.last_error())

    def inverse_pattern(self, z, plain: bool = False) -> np.ndarray:
        """z as selinv() returns it; d log det A / d values (plain: the entries of (P A P')^-1) in A2 order."""
        zz = _f64(z)
        if zz.size != int(self.sym.xsize):
            raise ValueError(f"inverse_pattern: z has {zz.size} entries, xsize = {int(self.sym.xsize)}")
        g = np.empty(int(self.sym.nnzA), dtype=np.float64)
        if N.lib().parsy_inverse_pattern_host(self._h, N.ptr(zz), 1.0, 0.0, 1 if plain else 0, N.ptr(g), None) != 0:
            raise RuntimeError("parsy_inverse_pattern_host failed: " + N.last_error())
        return g

    def trace_inverse_device(self, d_z: int, d_bvalues: int, ldb: int, nb: int, stream: int = 0) -> np.ndarray:
        """tr(A^-1 B_m), m < nb, for the columns of d_bvalues (A2-ordered values on A's pattern); synchronises."""
        out = np.zeros(max(nb, 1), dtype=np.float64)
        if N.lib().parsy_trace_inverse_device(self._h, d_z or None, d_bvalues or None, ldb, nb, N.ptr(out), stream) != 0:
            raise RuntimeError("parsy_trace_inverse_device failed: " + N.last_error())
        return out[:nb]

    # the factor as an operator: G = P' L with G G' = A (include/parsy_amd.h) ------------------------------------------
    OPS = {"G": 0, "GT": 1, "GINV": 2, "GINVT": 3}

    @staticmethod
    def _op(op) -> int:
        return Plan.OPS[op] if isinstance(op, str) else int(op)

    @property
    def apply_info(self) -> dict:
        """rows, occurrences (ssize), max_occurrences (most panels a row appears in), block_columns (right-hand sides per
        pass over lValues), workspace_bytes (of the products, known on the host), device_bytes (0 before the first device
        call), last_op (-1: none yet), last_launches."""
        ai = N.ApplyInfo()
        if N.lib().parsy_factor_apply_get_info(self._h, C.byref(ai)) != 0:
            raise RuntimeError("parsy_factor_apply_get_info failed: " + N.last_error())
        return ai.as_dict()

    def apply_row_index(self):
        """(ptr int64[n + 1], pos int64[ssize]): the positions k of the row lists with s[k] == row are
        pos[ptr[row]:ptr[row + 1]], ascending."""
        ptr = np.zeros(self.sym.n + 1, dtype=np.int64)
        pos = np.zeros(int(self.sym.ssize), dtype=np.int64)
        if N.lib().parsy_factor_apply_row_index(self._h, N.ptr(ptr), N.ptr(pos)) != 0:
            raise RuntimeError("parsy_factor_apply_row_index failed: " + N.last_error())
        return ptr, pos

    def factor_apply_device(self, d_lValues: int, op, d_x: int, ldx: int, nrhs: int, d_y: int, ldy: int,
                            alpha: float = 1.0, beta: float = 0.0, stream: int = 0) -> None:
        """Y = beta Y + alpha op(X), op in "G" (P' L), "GT" (L' P), "GINV" (L^-1 P), "GINVT" (P' L^-T) or 0 .. 3, under the
        plan's ordering (set_perm); X and Y column-major device arrays, not the same one."""
        if N.lib().parsy_factor_apply_device(self._h, d_lValues or None, self._op(op), d_x or None, ldx, nrhs, alpha, beta,
                                             d_y or None, ldy, stream) != 0:
            raise RuntimeError("parsy_factor_apply_device failed: " + N.last_error())

    def factor_apply(self, lValues, x, op, alpha: float = 1.0, y=None, beta: float = 0.0):
        """Host arrays (n,) or (n, nrhs) in: (beta y + alpha op(x), device_seconds), shaped like x; y is not changed."""
        x = np.asarray(x, dtype=np.float64)
        one = x.ndim == 1
        n = self.sym.n
        X = np.asfortranarray(x.reshape(n, -1))
        nrhs = X.shape[1]
        if y is None:
            if beta != 0.0:
                raise ValueError("factor_apply: beta != 0 needs y")
            Y = np.zeros((n, nrhs), order="F")
        else:
            Y = np.array(np.asarray(y, dtype=np.float64).reshape(n, -1), order="F", copy=True)
            if Y.shape != X.shape:
                raise ValueError(f"factor_apply: x is {X.shape}, y is {Y.shape}")
        lv = _f64(lValues)
        sec = C.c_double(0)
        if N.lib().parsy_factor_apply_host(self._h, N.ptr(lv), self._op(op), X.ctypes.data_as(C.c_void_p), max(n, 1), nrhs,
                                           alpha, beta, Y.ctypes.data_as(C.c_void_p), max(n, 1), C.byref(sec)) != 0:
            raise RuntimeError("parsy_factor_apply_host failed: " + N.last_error())
        return (Y[:, 0].copy() if one else np.ascontiguousarray(Y)), sec.value

    def sample(self, lValues, z, mean=None, kind: str = "precision"):
        """x = mean + G^-T z, a draw from N(mean, A^-1) for standard normal z (kind="precision": A is a precision
        matrix), or x = mean + G z from N(mean, A) (kind="covariance"); one call with alpha = beta = 1.  z and mean are
        (n,) or (n, nrhs) in the caller's ordering; on first use the plan takes sym.Perm as its ordering, as
        solve_refined does.  The library draws nothing itself: the same z gives the same x."""
        if kind not in ("precision", "covariance"):
            raise ValueError('sample: kind must be "precision" or "covariance"')
        if not getattr(self, "_perm_set", False):
            self.set_perm(self.sym.Perm)
            self._perm_set = True
        op = "GINVT" if kind == "precision" else "G"
        if mean is None:
            return self.factor_apply(lValues, z, op)[0]
        m = np.asarray(mean, dtype=np.float64)
        zz = np.asarray(z, dtype=np.float64)
        if m.shape != zz.shape:
            m = np.broadcast_to(m.reshape(self.sym.n, -1), zz.reshape(self.sym.n, -1).shape).reshape(zz.shape)
        return self.factor_apply(lValues, zz, op, alpha=1.0, y=m, beta=1.0)[0]

    # update / downdate of the factor: A + W W' and A - W W' in place (include/parsy_amd.h) ---------------------------
    @staticmethod
    def _w_csc(W, n):
        """(wp, wi, wx) of W: a (wp, wi, wx) triple as it is, or a dense (n,) / (n, k) array whose non-zeros are the
        pattern."""
        if isinstance(W, tuple):
            wp, wi, wx = W
            return _i32(wp), _i32(wi), _f64(wx)
        D = np.asarray(W, dtype=np.float64)
        if D.ndim == 1:
            D = D.reshape(n, 1)
        if D.ndim != 2 or D.shape[0] != n:
            raise ValueError(f"W is {D.shape}, the plan has n = {n}")
        cols = [np.flatnonzero(D[:, t]) for t in range(D.shape[1])]
        wp = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int32)
        wi = (np.concatenate(cols) if cols else np.zeros(0)).astype(np.int32)
        wx = np.concatenate([D[c, t] for t, c in enumerate(cols)]).astype(np.float64) if cols else np.zeros(0)
        return wp, wi, np.ascontiguousarray(wx)

    def updown_device(self, d_lValues: int, wp, wi, d_wx: int, sign: int = +1, stream: int = 0) -> None:
        """d_lValues, the factor of A, becomes the factor of A + sign W W' (W: host pattern wp / wi in the caller's
        ordering, values on the device) under the plan's ordering (set_perm).  The pattern of L does not change: a W
        that would change it is refused.  Check updown_status() afterwards."""
        wp = _i32(wp)
        wi = _i32(wi)
        if N.lib().parsy_factor_updown_device(self._h, d_lValues or None, int(sign), wp.size - 1, N.ptr(wp), N.ptr(wi),
                                              d_wx or None, stream) != 0:
            raise RuntimeError("parsy_factor_updown_device failed: " + N.last_error())

    def updown(self, lValues, W, sign: int = +1):
        """Host arrays: (the factor of A + sign W W', device_seconds); lValues is not changed.  W: dense (n,) or (n, k) in
        the caller's ordering (its non-zeros are the pattern) or a (wp, wi, wx) triple.  On first use the plan takes
        sym.Perm as its ordering, as solve_refined does.  After a failed downdate (updown_status() != 0) the result is
        not a factor."""
        if not getattr(self, "_perm_set", False):
            self.set_perm(self.sym.Perm)
            self._perm_set = True
        wp, wi, wx = self._w_csc(W, self.sym.n)
        lv = np.array(lValues, dtype=np.float64, copy=True).reshape(-1)
        sec = C.c_double(0)
        if N.lib().parsy_factor_updown_host(self._h, N.ptr(lv), int(sign), wp.size - 1, N.ptr(wp), N.ptr(wi), N.ptr(wx),
                                            C.byref(sec)) != 0:
            raise RuntimeError("parsy_factor_updown_host failed: " + N.last_error())
        return lv, sec.value

    def updown_status(self) -> int:
        """0, or the first column (1-based, factor's ordering) whose pivot failed in the last update / downdate."""
        return int(N.lib().parsy_updown_status(self._h))

    def updown_path(self, W):
        """(supernodes, first_col) an update by W would touch, ascending, under the plan's ordering as it is set; W as
        in updown().  Host-only plans too."""
        wp, wi, _ = self._w_csc(W, self.sym.n)
        sn = np.zeros(max(self.sym.nsuper, 1), dtype=np.int32)
        fc = np.zeros(max(self.sym.nsuper, 1), dtype=np.int32)
        cnt = N.lib().parsy_updown_path(self._h, wp.size - 1, N.ptr(wp), N.ptr(wi), N.ptr(sn), N.ptr(fc))
        if cnt < 0:
            raise RuntimeError("parsy_updown_path failed: " + N.last_error())
        return sn[:cnt].copy(), fc[:cnt].copy()

    @property
    def updown_info(self) -> dict:
        """Of the last updown_device / updown call: path_supernodes, block_columns, last_launches, last_k, last_sign,
        entries_touched; device_bytes (0 before the first device call)."""
        ui = N.UpdownInfo()
        if N.lib().parsy_updown_get_info(self._h, C.byref(ui)) != 0:
            raise RuntimeError("parsy_updown_get_info failed: " + N.last_error())
        return ui.as_dict()

    # row delete / row add in the factor (include/parsy_amd.h) --------------------------------------------------------
    @staticmethod
    def _column(column, n):
        """(ci, cx) of a column: an (indices, values) pair sorted by index, or a dense (n,) vector whose non-zeros are the
        pattern."""
        if isinstance(column, tuple):
            ci, cx = _i32(column[0]), _f64(column[1])
            if ci.size != cx.size:
                raise ValueError(f"the column has {ci.size} indices and {cx.size} values")
            return ci, cx
        d = np.asarray(column, dtype=np.float64)
        if d.shape != (n,):
            raise ValueError(f"the column is {d.shape}, the plan has n = {n}")
        ci = np.flatnonzero(d).astype(np.int32)
        return ci, np.ascontiguousarray(d[ci])

    def rowdel_device(self, d_lValues: int, row: int, stream: int = 0) -> None:
        """d_lValues, the factor of A, becomes the factor of A with row and column `row` (the plan's ordering: set_perm)
        made the identity's.  The pattern of L does not change.  Check rowmod_status() afterwards."""
        if N.lib().parsy_factor_rowdel_device(self._h, d_lValues or None, int(row), stream) != 0:
            raise RuntimeError("parsy_factor_rowdel_device failed: " + N.last_error())

    def rowadd_device(self, d_lValues: int, row: int, ci, d_cx: int, stream: int = 0) -> None:
        """Puts row and column `row` back: ci the ascending row indices (host) of the full symmetric column, the diagonal
        among them, d_cx its values on the device.  What stood in that row and column of the factor is not read; a
        column outside the pattern of L is refused.  Check rowmod_status() afterwards."""
        ci = _i32(ci)
        if N.lib().parsy_factor_rowadd_device(self._h, d_lValues or None, int(row), ci.size, N.ptr(ci), d_cx or None,
                                              stream) != 0:
            raise RuntimeError("parsy_factor_rowadd_device failed: " + N.last_error())

    def _take_perm(self):
        if not getattr(self, "_perm_set", False):
            self.set_perm(self.sym.Perm)
            self._perm_set = True

    def rowdel(self, lValues, row: int):
        """Host arrays: (the factor with row / column `row` of A made the identity's, device_seconds); lValues is not
        changed.  On first use the plan takes sym.Perm as its ordering, as updown does."""
        self._take_perm()
        lv = np.array(lValues, dtype=np.float64, copy=True).reshape(-1)
        sec = C.c_double(0)
        if N.lib().parsy_factor_rowdel_host(self._h, N.ptr(lv), int(row), C.byref(sec)) != 0:
            raise RuntimeError("parsy_factor_rowdel_host failed: " + N.last_error())
        return lv, sec.value

    def rowadd(self, lValues, row: int, column):
        """Host arrays: (the factor with row / column `row` put back, device_seconds); lValues is not changed.  column:
        the full symmetric column in the caller's ordering, a dense (n,) vector (its non-zeros are the pattern) or an
        (indices, values) pair, the diagonal entry present.  After a failure (rowmod_status() != 0) the result is not a
        factor."""
        self._take_perm()
        ci, cx = self._column(column, self.sym.n)
        lv = np.array(lValues, dtype=np.float64, copy=True).reshape(-1)
        sec = C.c_double(0)
        if N.lib().parsy_factor_rowadd_host(self._h, N.ptr(lv), int(row), ci.size, N.ptr(ci), N.ptr(cx), C.byref(sec)) != 0:
            raise RuntimeError("parsy_factor_rowadd_host failed: " + N.last_error())
        return lv, sec.value

    def rowmod_status(self) -> int:
        """0; p + 1 (p: the row in the factor's ordering) when the add's own pivot failed; a larger column (1-based) when
        the downdate behind it left the matrix indefinite."""
        return int(N.lib().parsy_rowmod_status(self._h))

    def rowmod_reach(self, row: int):
        """(supernodes, position, height) of the row subtree of `row` under the plan's ordering as it is set, ascending.
        Host-only plans too."""
        m = max(self.sym.nsuper, 1)
        sn, pos, h = (np.zeros(m, dtype=np.int32) for _ in range(3))
        cnt = N.lib().parsy_rowmod_reach(self._h, int(row), N.ptr(sn), N.ptr(pos), N.ptr(h))
        if cnt < 0:
            raise RuntimeError("parsy_rowmod_reach failed: " + N.last_error())
        return sn[:cnt].copy(), pos[:cnt].copy(), h[:cnt].copy()

    @property
    def rowmod_info(self) -> dict:
        """Of the last rowdel_device / rowadd_device call: last_op (1 delete, 2 add), last_row, reach_supernodes, heights,
        row_launches, column_launches, rotation_launches, entries_read, entries_walked; device_bytes (0 before the first
        device call)."""
        ri = N.RowmodInfo()
        if N.lib().parsy_rowmod_get_info(self._h, C.byref(ri)) != 0:
            raise RuntimeError("parsy_rowmod_get_info failed: " + N.last_error())
        return ri.as_dict()

    def inverse_entries(self, lValues, rows, cols) -> np.ndarray:
        """The dense len(rows) x len(cols) block A^-1[rows, cols] (caller's ordering) from the factor, through a sparse
        solve whose right-hand sides are the unit vectors of `cols` and whose selected rows are `rows` (SparseSolve): only
        the panels those reach are read.  On first use the plan takes sym.Perm as its ordering, as rowdel does."""
        self._take_perm()
        cols = _i32(cols).reshape(-1)
        S = SparseSolve(self, (np.arange(cols.size + 1, dtype=np.int32), cols), rows)
        try:
            return S.solve(lValues, np.ones(cols.size), op="A")[0]
        finally:
            S.close()

    def backsolve_device(self, d_lValues: int, d_x: int, nrhs: int, ldx: int, stream: int = 0) -> None:
        if N.lib().parsy_backsolve_device(self._h, d_lValues, d_x, nrhs, ldx, stream) != 0:
            raise RuntimeError("parsy_backsolve_device failed: " + N.last_error())

    def rhs_ones_device(self, d_lValues: int, d_b: int, stream: int = 0) -> None:
        """d_b = L * 1 on the stored structure (the reference's rhsInitBlocked, common/Util.h:277)."""
        if N.lib().parsy_rhs_ones_device(self._h, d_lValues, d_b, stream) != 0:
            raise RuntimeError("parsy_rhs_ones_device failed: " + N.last_error())

    # device-pointer API ---------------------------------------------------------
    def factor_device(self, d_values: int, d_lValues: int, stream: int = 0, init: bool = True) -> None:
        if N.lib().parsy_factor_device_ex(self._h, d_values, d_lValues, stream, 0 if init else 1) != 0:
            raise RuntimeError("parsy_factor_device failed: " + N.last_error())

    def solve_device(self, d_lValues: int, d_x: int, nrhs: int, ldx: int, stream: int = 0) -> None:
        if N.lib().parsy_solve_device(self._h, d_lValues, d_x, nrhs, ldx, stream) != 0:
            raise RuntimeError("parsy_solve_device failed: " + N.last_error())

    def solve_levels(self) -> np.ndarray:
        """The etree level of every supernode, as the launches of the solves go by it (parsy_plan_solve_levels)."""
        out = np.zeros(self.sym.nsuper, dtype=np.int32)
        N.lib().parsy_plan_solve_levels(self._h, N.ptr(out))
        return out

    def solve_levels_device(self, d_lValues: int, d_x: int, nrhs: int, ldx: int, stream: int, level_begin: int, level_end: int,
                            first: bool, last: bool, backward: bool = False) -> None:
        """One step of a solve that goes level by level (parsy_solve_levels_device): the active supernodes of the etree
        levels [level_begin, level_end)."""
        flags = (1 if first else 0) | (2 if last else 0) | (4 if backward else 0)
        if N.lib().parsy_solve_levels_device(self._h, d_lValues, d_x, nrhs, ldx, stream, level_begin, level_end, flags) != 0:
            raise RuntimeError("parsy_solve_levels_device failed: " + N.last_error())

    # level by level (the steps of a multi-device run; parsy_factor_device is exactly this sequence) ----
    def factor_begin(self, d_values: int, d_lValues: int, stream: int = 0, init: bool = True) -> None:
        if N.lib().parsy_factor_begin(self._h, d_values, d_lValues, stream, 0 if init else 1) != 0:
            raise RuntimeError("parsy_factor_begin failed: " + N.last_error())

    def factor_level(self, level: int, d_lValues: int, stream: int = 0) -> None:
        if N.lib().parsy_factor_level(self._h, level, d_lValues, stream) != 0:
            raise RuntimeError("parsy_factor_level failed: " + N.last_error())

    def factor_end(self, stream: int = 0) -> None:
        if N.lib().parsy_factor_end(self._h, stream) != 0:
            raise RuntimeError("parsy_factor_end failed: " + N.last_error())

    def pieces(self) -> dict:
        """The pieces of the Cholesky view: supernode, level, col0, width, rows, value_begin, value_end."""
        n = int(N.lib().parsy_plan_pieces(self._h, *([None] * 7)))
        out = {k: np.zeros(n, dtype=np.int32) for k in ("supernode", "level", "col0", "width", "rows")}
        out.update({k: np.zeros(n, dtype=np.int64) for k in ("value_begin", "value_end")})
        N.lib().parsy_plan_pieces(self._h, *[N.ptr(out[k]) for k in (
            "supernode", "level", "col0", "width", "rows", "value_begin", "value_end")])
        return out

    def set_active_pieces(self, mask) -> None:
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        if N.lib().parsy_plan_set_active_pieces(self._h, N.ptr(m)) != 0:
            raise RuntimeError(N.last_error())

    def check(self) -> int:
        return int(N.lib().parsy_plan_check(self._h))

    def last_factor_ms(self) -> float:
        return float(N.lib().parsy_last_factor_ms(self._h))

    def last_solve_ms(self) -> float:
        return float(N.lib().parsy_last_solve_ms(self._h))

    def profile(self, mode: int) -> None:
        N.lib().parsy_plan_profile(self._h, mode)

    def profile_collect(self) -> None:
        if N.lib().parsy_plan_profile_collect(self._h) != 0:
            raise RuntimeError("profile_collect: no profiled run to collect")

    def profile_get(self) -> dict:
        ms = np.zeros(10, dtype=np.float64)
        cnt = np.zeros(10, dtype=np.int32)
        runs = C.c_int(0)
        N.lib().parsy_plan_profile_get(self._h, N.ptr(ms), N.ptr(cnt), C.byref(runs))
        return {"runs": runs.value, "ms": dict(zip(KIND_NAMES, ms.tolist())),
                "launches": dict(zip(KIND_NAMES, cnt.tolist()))}


# ---------------------------------------------------------------------------
# solves with sparse right-hand sides for selected rows of the result
# ---------------------------------------------------------------------------
class SparseSolve:
    """One plan, one pattern of B and one list of selected rows (parsy_reach).  B_pattern: a (bp, bi) pair or anything
    with .indptr / .indices in compressed columns (n x nrhs, rows strictly ascending within a column); rows: distinct rows
    of the result in any order, None for all.  Both in the plan's ordering as it is set (Plan.set_perm; the handle keeps
    a copy).  A call reads only the panels of the supernodes B reaches (forward) and the rows need (backward); it never
    falls back to the plan's full solve: info["fwd_entries"] / ["bwd_entries"] against ["xsize"] let a caller choose.
    Host-only plans (device < 0) too: info, reach, check."""

    OPS = {"A": 0, "GINV": 1, "GINVT": 2}

    def __init__(self, plan: "Plan", B_pattern, rows=None):
        if isinstance(B_pattern, tuple):
            bp, bi = B_pattern
        else:
            bp, bi = B_pattern.indptr, B_pattern.indices
        self.bp, self.bi = _i32(bp).reshape(-1), _i32(bi).reshape(-1)
        self.rows = None if rows is None else _i32(rows).reshape(-1)
        self.plan = plan
        self.n = int(plan.sym.n)
        self.nrhs = int(self.bp.size) - 1
        self.nx = self.n if self.rows is None else int(self.rows.size)
        self._h = N.lib().parsy_reach_create(plan._h, self.nrhs, N.ptr(self.bp), N.ptr(self.bi), self.nx, N.ptr(self.rows))
        if not self._h:
            raise RuntimeError("parsy_reach_create failed: " + N.last_error())

    def close(self):
        h, self._h = self._h, None
        if h:
            N.lib().parsy_reach_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        """nrhs, nx; fwd_ / bwd_supernodes, _pieces, _steps, _entries; xsize; last_op and last_kernels of the last device
        call (-1, 0: none yet); device_bytes (0 before the first device call)."""
        ri = N.ReachInfo()
        if N.lib().parsy_reach_get_info(self._h, C.byref(ri)) != 0:
            raise RuntimeError("parsy_reach_get_info failed: " + N.last_error())
        return ri.as_dict()

    def reach(self):
        """(F, K): the supernodes of the forward and of the backward reach, ascending."""
        i = self.info()
        fwd = np.zeros(max(i["fwd_supernodes"], 1), dtype=np.int32)
        bwd = np.zeros(max(i["bwd_supernodes"], 1), dtype=np.int32)
        if N.lib().parsy_reach_get(self._h, N.ptr(fwd), N.ptr(bwd)) != 0:
            raise RuntimeError("parsy_reach_get failed: " + N.last_error())
        return fwd[:i["fwd_supernodes"]].copy(), bwd[:i["bwd_supernodes"]].copy()

    def check(self) -> int:
        return int(N.lib().parsy_reach_check(self._h))

    def solve_device(self, d_lValues: int, d_bx: int, d_x: int, ldx: int, op="A", stream: int = 0) -> None:
        """d_x (nx x nrhs column-major, ldx >= nx) = the selected rows of A^-1 B ("A"), L^-1 P B ("GINV") or
        P' L^-T P B ("GINVT"); d_bx: B's values in the order of bi.  Only enqueues (after the handle's first call)."""
        op = self.OPS[op] if isinstance(op, str) else int(op)
        if N.lib().parsy_solve_sparse_device(self._h, d_lValues or None, d_bx or None, op, d_x or None, ldx, stream) != 0:
            raise RuntimeError("parsy_solve_sparse_device failed: " + N.last_error())

    def solve(self, lValues, bx, op="A"):
        """Host arrays: (X of shape (nx, nrhs), device_seconds); bx holds B's values in the order of bi."""
        op = self.OPS[op] if isinstance(op, str) else int(op)
        bx = _f64(bx).reshape(-1)
        if bx.size != self.bi.size:
            raise ValueError(f"bx must hold {self.bi.size} values, one per entry of the pattern of B")
        lv = _f64(lValues)
        X = np.zeros((self.nx, self.nrhs), order="F")
        sec = C.c_double(0)
        if N.lib().parsy_solve_sparse_host(self._h, N.ptr(lv), N.ptr(bx), op, X.ctypes.data_as(C.c_void_p), max(self.nx, 1),
                                           C.byref(sec)) != 0:
            raise RuntimeError("parsy_solve_sparse_host failed: " + N.last_error())
        return np.ascontiguousarray(X), sec.value


# ---------------------------------------------------------------------------
# normal matrices on the plan's pattern: N = F diag(w) F' + beta I + A0, least squares through its factor
# ---------------------------------------------------------------------------
class NormalEquations:
    """One plan and one pattern of F (parsy_normal).  F: a (Fp, Fi, Fx) triple or anything with .indptr / .indices /
    .data in compressed columns (n x m, rows ascending within a column, in the caller's ordering).  The handle keeps
    the plan's ordering as it stands; a plan whose ordering was never set takes sym.Perm first, as solve_refined
    does.  Every pair of rows that share a column of F must be a stored entry of the plan's pattern of A: an F that
    breaks the rule is refused here (RuntimeError).  Host-only plans (device < 0) too: info, pairs, check."""

    OPS = {"F": 0, "FT": 1}

    def __init__(self, plan: "Plan", F):
        Fp, Fi, Fx = self._csc(F)
        if not getattr(plan, "_perm_set", False):
            plan.set_perm(plan.sym.Perm)
            plan._perm_set = True
        self.plan = plan
        self.n = int(plan.sym.n)
        self.m = int(Fp.size) - 1
        self.Fp, self.Fi = Fp, Fi
        self.fx = Fx
        self._h = N.lib().parsy_normal_create(plan._h, self.m, N.ptr(Fp), N.ptr(Fi))
        if not self._h:
            raise RuntimeError("parsy_normal_create failed: " + N.last_error())

    @staticmethod
    def _csc(F):
        if isinstance(F, tuple):
            Fp, Fi, Fx = F
        else:
            Fp, Fi, Fx = F.indptr, F.indices, F.data
        return _i32(Fp), _i32(Fi), (None if Fx is None else _f64(Fx))

    @staticmethod
    def pattern(n: int, F):
        """(Ap, Ai): the lower triangle of the pattern of F F' with a full diagonal, sorted CSC -- what to order and
        analyse (with any values) for a plan that satisfies the pattern rule."""
        Fp, Fi, _ = NormalEquations._csc(F)
        Ap = np.zeros(n + 1, dtype=np.int32)
        nnz = N.lib().parsy_normal_pattern(n, Fp.size - 1, N.ptr(Fp), N.ptr(Fi), N.ptr(Ap), None)
        if nnz < 0:
            raise RuntimeError("parsy_normal_pattern failed: " + N.last_error())
        Ai = np.zeros(max(int(nnz), 1), dtype=np.int32)
        N.lib().parsy_normal_pattern(n, Fp.size - 1, N.ptr(Fp), N.ptr(Fi), N.ptr(Ap), N.ptr(Ai))
        return Ap, Ai[:nnz]

    def close(self):
        h, self._h = self._h, None
        if h:
            N.lib().parsy_normal_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def info(self) -> dict:
        """n, m, nnzF, pairs, longest_list, chunked_entries, chunks, border (longest list of the 1-, 8- and 64-lane
        class), class_entries, entries_untouched, launches (per values call), device_bytes."""
        ni = N.NormalInfo()
        if N.lib().parsy_normal_get_info(self._h, C.byref(ni)) != 0:
            raise RuntimeError("parsy_normal_get_info failed: " + N.last_error())
        return ni.as_dict()

    def pairs(self, q: int):
        """(a, b, k) of A2 entry q: positions in fx of the entries on its row and its column (factor's ordering), and
        their column of F, ascending in k: the summation order."""
        cap = max(int(self.info["longest_list"]), 1)
        a, b, k = (np.zeros(cap, dtype=np.int32) for _ in range(3))
        cnt = N.lib().parsy_normal_pairs(self._h, int(q), N.ptr(a), N.ptr(b), N.ptr(k))
        if cnt < 0:
            raise RuntimeError("parsy_normal_pairs failed: " + N.last_error())
        return a[:cnt].copy(), b[:cnt].copy(), k[:cnt].copy()

    def check(self) -> int:
        return int(N.lib().parsy_normal_check(self._h))

    def _fx(self, fx):
        fx = self.fx if fx is None else _f64(fx)
        if fx is None or fx.size != self.Fi.size:
            raise ValueError(f"fx must hold nnzF = {self.Fi.size} values")
        return fx

    def _w(self, w):
        if w is None:
            return None
        w = _f64(w)
        if w.size != self.m:
            raise ValueError(f"w must hold m = {self.m} weights")
        return w

    def values_device(self, d_fx: int, d_values: int, d_w: int = 0, beta: float = 0.0, d_base: int = 0,
                      stream: int = 0) -> None:
        """d_values (nnzA doubles, A2 order) = F diag(w) F' + beta I + base on the plan's pattern; d_w / d_base: 0 for
        none; d_base may be d_values."""
        if N.lib().parsy_normal_values_device(self._h, d_fx or None, d_w or None, beta, d_base or None, d_values or None,
                                              stream) != 0:
            raise RuntimeError("parsy_normal_values_device failed: " + N.last_error())

    def values(self, fx=None, w=None, beta: float = 0.0, base=None):
        """Host arrays: (values in A2 order, device_seconds)."""
        fx, w = self._fx(fx), self._w(w)
        base = None if base is None else _f64(base)
        nnz = int(self.plan.info["nnzA"])
        if base is not None and base.size != nnz:
            raise ValueError(f"base must hold nnzA = {nnz} values")
        out = np.zeros(nnz, dtype=np.float64)
        sec = C.c_double(0)
        if N.lib().parsy_normal_values_host(self._h, N.ptr(fx), N.ptr(w), beta, N.ptr(base), N.ptr(out), C.byref(sec)) != 0:
            raise RuntimeError("parsy_normal_values_host failed: " + N.last_error())
        return out, sec.value

    def apply_device(self, op, d_fx: int, d_x: int, ldx: int, nrhs: int, d_y: int, ldy: int, d_w: int = 0,
                     alpha: float = 1.0, beta: float = 0.0, stream: int = 0) -> None:
        """Y = beta Y + alpha op(X): "F" (Y n x nrhs = F diag(w) X) or "FT" (Y m x nrhs = F' X); column-major device
        arrays, the n-side in the caller's ordering."""
        op = self.OPS[op] if isinstance(op, str) else int(op)
        if N.lib().parsy_normal_apply_device(self._h, op, d_fx or None, d_w or None, d_x or None, ldx, nrhs, alpha, beta,
                                             d_y or None, ldy, stream) != 0:
            raise RuntimeError("parsy_normal_apply_device failed: " + N.last_error())

    def apply(self, op, x, fx=None, w=None, alpha: float = 1.0, y=None, beta: float = 0.0):
        """Host arrays (rows,) or (rows, nrhs) in: (beta y + alpha op(x), device_seconds); y is not changed."""
        opi = self.OPS[op] if isinstance(op, str) else int(op)
        nx, ny = (self.m, self.n) if opi == 0 else (self.n, self.m)
        fx, w = self._fx(fx), self._w(w)
        x = np.asarray(x, dtype=np.float64)
        one = x.ndim == 1
        X = np.asfortranarray(x.reshape(nx, -1))
        nrhs = X.shape[1]
        if y is None:
            if beta != 0.0:
                raise ValueError("apply: beta != 0 needs y")
            Y = np.zeros((ny, nrhs), order="F")
        else:
            Y = np.array(np.asarray(y, dtype=np.float64).reshape(ny, -1), order="F", copy=True)
            if Y.shape[1] != nrhs:
                raise ValueError(f"apply: x has {nrhs} columns, y has {Y.shape[1]}")
        sec = C.c_double(0)
        if N.lib().parsy_normal_apply_host(self._h, opi, N.ptr(fx), N.ptr(w), X.ctypes.data_as(C.c_void_p), max(nx, 1), nrhs,
                                           alpha, beta, Y.ctypes.data_as(C.c_void_p), max(ny, 1), C.byref(sec)) != 0:
            raise RuntimeError("parsy_normal_apply_host failed: " + N.last_error())
        return (Y[:, 0].copy() if one else np.ascontiguousarray(Y)), sec.value

    def lstsq_device(self, d_fx: int, d_lValues: int, d_c: int, ldc: int, d_x: int, ldx: int, nrhs: int, steps: int = 1,
                     d_w: int = 0, beta: float = 0.0, d_r: int = 0, ldr: int = 0, d_g: int = 0, ldg: int = 0,
                     stream: int = 0) -> None:
        """x = S F W c and `steps` corrections x += S (F W (c - F' x) - beta x) through d_lValues (it may be a stale
        factor); d_r / d_g (0: none) receive the residual and the gradient at the returned x.  Nothing waits: check
        plan.solve_status() after synchronising."""
        if N.lib().parsy_lsq_solve_device(self._h, d_fx or None, d_w or None, beta, d_lValues or None, d_c or None, ldc,
                                          d_x or None, ldx, nrhs, steps, d_r or None, ldr, d_g or None, ldg, stream) != 0:
            raise RuntimeError("parsy_lsq_solve_device failed: " + N.last_error())

    def lstsq(self, lValues, c, w=None, beta: float = 0.0, steps: int = 1, fx=None):
        """Host arrays: (x, r, g) minimising sum_k w_k (f_k' x - c_k)^2 + beta ||x||^2 for c (m,) or (m, nrhs); r = c - F' x
        and g = F W r - beta x at the returned x."""
        fx, w = self._fx(fx), self._w(w)
        c = np.asarray(c, dtype=np.float64)
        one = c.ndim == 1
        Cm = np.asfortranarray(c.reshape(self.m, -1))
        nrhs = Cm.shape[1]
        X = np.zeros((self.n, nrhs), order="F")
        R = np.zeros((self.m, nrhs), order="F")
        G = np.zeros((self.n, nrhs), order="F")
        lv = _f64(lValues)
        sec = C.c_double(0)
        vp = C.c_void_p
        if N.lib().parsy_lsq_solve_host(self._h, N.ptr(fx), N.ptr(w), beta, N.ptr(lv), Cm.ctypes.data_as(vp), max(self.m, 1),
                                        X.ctypes.data_as(vp), max(self.n, 1), nrhs, steps, R.ctypes.data_as(vp),
                                        max(self.m, 1), G.ctypes.data_as(vp), max(self.n, 1), C.byref(sec)) != 0:
            raise RuntimeError("parsy_lsq_solve_host failed: " + N.last_error())
        self.last_seconds = sec.value
        if one:
            return X[:, 0].copy(), R[:, 0].copy(), G[:, 0].copy()
        return np.ascontiguousarray(X), np.ascontiguousarray(R), np.ascontiguousarray(G)


# ---------------------------------------------------------------------------
# distribution of one factorization over the devices of a node
# ---------------------------------------------------------------------------
class Dist:
    """Ownership of the pieces and the messages that follow every level (parsy_dist; host logic)."""

    def __init__(self, plan: "Plan", nranks: int, block: int = 0, _borrowed=None):
        self._own = _borrowed is None
        self._h = _borrowed or N.lib().parsy_dist_create(plan._h, nranks, block)
        if not self._h:
            raise RuntimeError("parsy_dist_create failed: " + N.last_error())
        di = N.DistInfo()
        N.lib().parsy_dist_get_info(self._h, C.byref(di))
        self.info = di.as_dict()
        self.nranks, self.nlevels = di.nranks, di.nlevels
        self.owner = np.zeros(di.n_pieces, dtype=np.int32)
        self.in_subtree = np.zeros(di.n_pieces, dtype=np.uint8)
        self.rank_cost = np.zeros(di.nranks)
        self.level_cost = np.zeros((di.nlevels, di.nranks))
        N.lib().parsy_dist_get(self._h, N.ptr(self.owner), N.ptr(self.in_subtree), N.ptr(self.rank_cost),
                               N.ptr(self.level_cost))

    def close(self):
        h, self._h = self._h, None
        if h and self._own:
            N.lib().parsy_dist_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, plan: "Plan") -> int:
        return int(N.lib().parsy_dist_check(plan._h, self._h))

    def mask(self, rank: int) -> np.ndarray:
        return (self.owner == rank).astype(np.uint8)

    def messages(self, level: int, rank: int | None = None):
        """The messages that follow `level` (those `rank` sends or receives when given):
        (src, dst, off int64[], len int32[], packed int64[], total)."""
        lib = N.lib()
        out = []
        for k in range(max(int(lib.parsy_dist_level_messages(self._h, level)), 0)):
            src, dst = C.c_int32(0), C.c_int32(0)
            nseg, total = C.c_int64(0), C.c_int64(0)
            # (who talks to whom first: the arrays of a message are copied only for the ranks that take part in it)
            if lib.parsy_dist_message(self._h, level, k, C.byref(src), C.byref(dst), C.byref(nseg), C.byref(total),
                                      None, None, None) != 0:
                raise RuntimeError(N.last_error())
            if rank is not None and rank not in (src.value, dst.value):
                continue
            off, ln, pk = N.c_i64_p(), N.c_int_p(), N.c_i64_p()
            lib.parsy_dist_message(self._h, level, k, None, None, None, None, C.byref(off), C.byref(ln), C.byref(pk))
            out.append((src.value, dst.value, N.view_array(off, nseg.value, np.int64),
                        N.view_array(ln, nseg.value, np.int32), N.view_array(pk, nseg.value, np.int64), total.value))
        return out


class MultiDevice:
    """One process driving several devices (parsy_mg): `devices` lists one HIP device per rank and may
    repeat a device (several ranks share it)."""

    def __init__(self, sym, devices, block: int = 0):
        if not getattr(sym, "_handle", None):
            raise RuntimeError("MultiDevice needs an inspector result (parsy_symbolic)")
        dv = np.ascontiguousarray(devices, dtype=np.int32)
        self.sym = sym
        self.nranks = len(dv)
        self._h = N.lib().parsy_mg_create(sym._handle, len(dv), N.ptr(dv), block)
        if not self._h:
            raise RuntimeError("parsy_mg_create failed: " + N.last_error())
        self.dist = Dist(None, len(dv), _borrowed=N.lib().parsy_mg_dist(self._h))

    def close(self):
        h, self._h = self._h, None
        if h:
            self.dist._h = None
            N.lib().parsy_mg_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_values(self, values) -> None:
        v = _f64(values)
        if N.lib().parsy_mg_set_values(self._h, N.ptr(v)) != 0:
            raise RuntimeError("parsy_mg_set_values failed: " + N.last_error())

    def factor(self):
        """One distributed factorization; returns (status, wall seconds)."""
        sec = C.c_double(0)
        st = int(N.lib().parsy_mg_factor(self._h, C.byref(sec)))
        if st < 0:
            raise RuntimeError("parsy_mg_factor failed: " + N.last_error())
        return st, sec.value

    def profile(self):
        """One factorization with the ranks taking turns (every step alone on its device) and every launch timed:
        (status, main_ms, side_ms, copy_ms), each nranks x levels."""
        shape = (self.nranks, self.dist.nlevels)
        main, side, copy = np.zeros(shape), np.zeros(shape), np.zeros(shape)
        st = int(N.lib().parsy_mg_profile(self._h, N.ptr(main), N.ptr(side), N.ptr(copy)))
        if st < 0:
            raise RuntimeError("parsy_mg_profile failed: " + N.last_error())
        return st, main, side, copy

    def rank_ms(self) -> np.ndarray:
        out = np.zeros(self.nranks)
        N.lib().parsy_mg_rank_ms(self._h, N.ptr(out))
        return out

    def gather(self) -> np.ndarray:
        lv = np.zeros(int(self.sym.xsize), dtype=np.float64)
        if N.lib().parsy_mg_gather_host(self._h, N.ptr(lv)) != 0:
            raise RuntimeError("parsy_mg_gather_host failed: " + N.last_error())
        return lv
