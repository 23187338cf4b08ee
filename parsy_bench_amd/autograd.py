"""PyTorch entry point: differentiable x = A^-1 b and log det A for a sparse SPD matrix with a fixed pattern.

torch is imported only here, and only for plumbing: allocation, index_select / index_copy_ with the inspector's A2src,
and the current stream, which is passed to every call.  All numerics go through the C ABI (include/parsy_amd.h): the
factorization, the refined solve, selected inversion, and the two gradient kernels.

Conventions.  `values` are the entries of the lower triangle of A in the caller's CSC order (LowerCSC.Ax); a stored
off-diagonal value stands for both A_ij and A_ji, so its gradient counts both occurrences.  With lambda = A^-1 gbar,
    d <gbar, A^-1 b> / d a_ij = -(lambda_i x_j + lambda_j x_i)   (-lambda_i x_i on the diagonal),   d / d b = lambda,
    d log det A / d a_ij = 2 (A^-1)_ij                            ((A^-1)_ii on the diagonal).
The backward of logdet runs one selected inversion, which costs 10-12 factorizations.
"""
from __future__ import annotations

import weakref

import torch
from torch.autograd.function import once_differentiable

from . import api, inspector


class _Factor:
    """One factorization: the A2-ordered values it was made from and L, both on the device."""

    def __init__(self, ref, version, a2, L):
        self.ref, self.version, self.a2, self.L = ref, version, a2, L


class SpdSolver:
    """Plan + factor cache for one pattern.  A_or_sym: a matrices.LowerCSC (analysed here under the library's nested
    dissection ordering) or an inspector.Symbolic.  solve() and logdet() on the same `values` tensor at the same
    version share one factorization; factor_count counts the factorizations made."""

    def __init__(self, A_or_sym, device: int = 0):
        sym = A_or_sym
        if not isinstance(sym, inspector.Symbolic):
            sym = inspector.analyze(A_or_sym, inspector.order_nd(A_or_sym))
        self.sym = sym
        self.device = torch.device("cuda", device)
        self.plan = api.Plan(sym, device)
        self.plan.set_perm(sym.Perm)
        self._a2src = torch.from_numpy(sym.A2src.astype("int64")).to(self.device)
        self._fact = None
        self.factor_count = 0

    def _stream(self) -> int:
        return int(torch.cuda.current_stream(self.device).cuda_stream)

    def _factor(self, values) -> _Factor:
        f = self._fact
        if f is not None and f.ref() is values and f.version == values._version:
            return f
        if values.dtype != torch.float64 or values.device != self.device or values.dim() != 1 or \
                values.numel() != int(self.sym.nnzA):
            raise ValueError(f"SpdSolver: values must be a float64 tensor of {int(self.sym.nnzA)} entries on {self.device}")
        a2 = values.detach().index_select(0, self._a2src)
        L = torch.empty(int(self.sym.xsize), dtype=torch.float64, device=self.device)
        self.plan.factor_device(a2.data_ptr(), L.data_ptr(), self._stream())
        torch.cuda.current_stream(self.device).synchronize()
        self.factor_count += 1
        col = self.plan.status()
        if col != 0:
            self._fact = None
            raise RuntimeError(f"SpdSolver: the matrix is not positive definite: non-positive pivot at column {col} "
                               f"(1-based, permuted ordering; column {int(self.sym.Perm[col - 1])} of A, 0-based)")
        self._fact = _Factor(weakref.ref(values), values._version, a2, L)
        return self._fact

    def _solve_raw(self, fact: _Factor, B, max_steps: int):
        """B: (nrhs, n) contiguous = n x nrhs column-major.  Returns X in the same layout."""
        n = self.sym.n
        X = torch.empty_like(B)
        self.plan.solve_spd_device(fact.a2.data_ptr(), fact.L.data_ptr(), B.data_ptr(), n, X.data_ptr(), n, B.shape[0],
                                   max_steps, self._stream())
        return X

    def _to_values(self, g2):
        """A2-ordered gradient -> the caller's CSC order."""
        return torch.zeros_like(g2).index_copy_(0, self._a2src, g2)

    def solve(self, values, b, max_steps: int = 0):
        """x = A^-1 b, shaped like b ((n,) or (n, nrhs)), with up to max_steps refinement steps; differentiable in
        values and b."""
        n = self.sym.n
        if b.dtype != torch.float64 or b.device != self.device or b.dim() not in (1, 2) or b.shape[0] != n:
            raise ValueError(f"SpdSolver.solve: b must be a float64 tensor of shape ({n},) or ({n}, nrhs) on {self.device}")
        return _Solve.apply(values, b, self, self._factor(values), int(max_steps))

    def logdet(self, values):
        """log det A as a 0-dim tensor; differentiable in values."""
        return _LogDet.apply(values, self, self._factor(values))

    def sample(self, values, n_samples: int = 1, mean=None, kind: str = "precision", z=None, generator=None):
        """Draws from N(mean, A^-1) (kind="precision": x = mean + G^-T z) or N(mean, A) (kind="covariance":
        x = mean + G z) with the cached factor of `values`, G G' = A; shaped (n,) for n_samples == 1 and (n, n_samples)
        otherwise.  z (standard normal, shaped like the result) is drawn here with torch.randn(..., generator=generator)
        on the device when it is not given: the library itself holds no random number generator, and the same z gives the
        same bits.  NOT differentiable in `values` (differentiating through the factor is out of scope): a gradient flows
        to `mean` only."""
        n = self.sym.n
        if kind not in ("precision", "covariance"):
            raise ValueError('SpdSolver.sample: kind must be "precision" or "covariance"')
        if n_samples < 1:
            raise ValueError("SpdSolver.sample: n_samples must be >= 1")
        shape = (n,) if n_samples == 1 else (n, n_samples)
        if z is None:
            z = torch.randn(shape, dtype=torch.float64, device=self.device, generator=generator)
        elif z.dtype != torch.float64 or z.device != self.device or tuple(z.shape) != shape:
            raise ValueError(f"SpdSolver.sample: z must be a float64 tensor of shape {shape} on {self.device}")
        fact = self._factor(values)
        Z = _as_columns(z, n)
        X = torch.empty_like(Z)
        self.plan.factor_apply_device(fact.L.data_ptr(), "GINVT" if kind == "precision" else "G", Z.data_ptr(), n, n_samples,
                                      X.data_ptr(), n, stream=self._stream())
        if kind == "precision":
            torch.cuda.current_stream(self.device).synchronize()
            if self.plan.solve_status() != 0:
                raise RuntimeError("SpdSolver.sample: the backward solve failed: " + api.N.last_error())
        x = X[0].clone() if n_samples == 1 else X.t().contiguous()
        if mean is None:
            return x
        if mean.dtype != torch.float64 or mean.device != self.device or mean.shape[0] != n or mean.dim() not in (1, 2):
            raise ValueError(f"SpdSolver.sample: mean must be a float64 tensor of shape ({n},) or ({n}, n_samples) on {self.device}")
        if mean.dim() == 1 and x.dim() == 2:
            mean = mean.unsqueeze(1)
        return mean + x


def _as_columns(t, n):
    return t.detach().reshape(n, -1).t().contiguous()


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, b, solver, fact, max_steps):
        n = solver.sym.n
        X = solver._solve_raw(fact, _as_columns(b, n), max_steps)
        ctx.solver, ctx.fact, ctx.max_steps, ctx.X = solver, fact, max_steps, X
        return X[0].clone() if b.dim() == 1 else X.t().contiguous()

    @staticmethod
    @once_differentiable
    def backward(ctx, gx):
        solver, fact, X = ctx.solver, ctx.fact, ctx.X
        n, nrhs = solver.sym.n, X.shape[0]
        Lam = solver._solve_raw(fact, _as_columns(gx, n), ctx.max_steps)
        gv = gb = None
        if ctx.needs_input_grad[0]:
            g2 = torch.empty(int(solver.sym.nnzA), dtype=torch.float64, device=solver.device)
            solver.plan.pattern_outer_device(Lam.data_ptr(), n, X.data_ptr(), n, nrhs, g2.data_ptr(), alpha=-1.0, beta=0.0,
                                             stream=solver._stream())
            gv = solver._to_values(g2)
        if ctx.needs_input_grad[1]:
            gb = Lam[0].clone() if gx.dim() == 1 else Lam.t().contiguous()
        return gv, gb, None, None, None


class _LogDet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, solver, fact):
        ld, col = solver.plan.logdet_device(fact.L.data_ptr(), solver._stream())
        if col != 0:
            raise RuntimeError(f"SpdSolver.logdet: the factor's pivot at column {col} is not positive and finite")
        ctx.solver, ctx.fact = solver, fact
        return torch.tensor(ld, dtype=torch.float64, device=solver.device)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        solver, fact = ctx.solver, ctx.fact
        if not ctx.needs_input_grad[0]:
            return None, None, None
        Z = torch.empty(int(solver.sym.xsize), dtype=torch.float64, device=solver.device)
        g2 = torch.empty(int(solver.sym.nnzA), dtype=torch.float64, device=solver.device)
        solver.plan.selinv_device(fact.L.data_ptr(), Z.data_ptr(), solver._stream())
        solver.plan.inverse_pattern_device(Z.data_ptr(), g2.data_ptr(), alpha=float(g), beta=0.0, stream=solver._stream())
        return solver._to_values(g2), None, None
