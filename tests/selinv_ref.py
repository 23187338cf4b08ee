"""The reference of the selected-inversion shape tests: a plain helper module of the suite (no fixtures, no collection
hooks).

* `takahashi`: the float64 numpy restatement of the Takahashi recurrence on the dense Cholesky factor, column by column
  from the last.  The same operation as the device's, not the same code: no blocks, no threshold, no gather map.  What it
  gives for `measure` is what the recurrence costs in double, whoever runs it; the device is allowed 4 times that.
* `inverse_extended`: the inverse in long double -- the restatement, one Newton step Z <- Z + Z (I - S Z) in long double,
  symmetrised -- with its residual asserted.  For D S D (shape_cases.scaled) nothing is recomputed: the reference is
  Zx_ij / (d_i d_j), which is exact.  (numpy's inv is no reference here: LU with pivoting errs by hundreds to thousands of
  u in this measure once the matrix is badly scaled.)
* `measure`: max over a mask of |Z - Zx|_ij / (u sqrt(Zx_ii Zx_jj)), u = 2^-53, formed in long double.  |Z_ij| <=
  sqrt(Z_ii Z_jj) for an SPD Z, so the error is relative to the largest value the entry can take, and the measure does not
  change under a symmetric diagonal scaling.
* `SHAPES`: block columns (wb, m = |R_b|) put on the edges the kernels care about; `reference(name)` holds everything a
  test needs of a shape, made once per process and left unchanged.
"""
from __future__ import annotations

import numpy as np

import shape_cases as SC

U = SC.U
SCALE_SEED = 100       # the scaling of a shape is shape_cases.scaling(n, SCALE_SEED + seed)
REF_CAP = 64.0         # the restatement's own measure must stay below this many u (it sits at 4 to 6)
MARGIN = 4.0           # the device's allowance over the restatement (as test_updown_gpu / test_rowmod_gpu)

# name -> (blocks, border, seed, chain, the (wb, m) classes the shape exists for)
SHAPES = {
    # widths on the edges (1, 16, 63, 64, 65 = 64 + 1, 17, 129 = 64 + 64 + 1), m around the 32-row chunk of the small path
    # and around one 64-row tile of the tiled path; the border adds (64, 66) (64, 2) (2, 0)
    # (the seed: the analysis postorders the blocks by the border row they hang from, highest first, and under one row by
    # the column count of their last column; under 38388 the first border rows are 5, 3, 1, 1, 1, 1, 0 and the blocks keep
    # their order, so the analysis gives exactly arrow_layout's supernodes)
    "edges": (((1, 31), (16, 32), (63, 33), (64, 63), (65, 64), (17, 65), (129, 1)), 130, 38388, False,
              ((1, 31), (16, 32), (63, 33), (64, 63), (64, 65), (1, 64), (17, 65), (64, 66), (64, 2), (1, 1), (2, 0))),
    # m around two and three tiles; the border adds (64, 128) (64, 64) (64, 0)
    "tall": (((8, 127), (64, 128), (33, 129), (2, 191)), 192, 22, False,
             ((8, 127), (64, 128), (33, 129), (2, 191), (64, 64), (64, 0))),
    # the catalogue's chain: every block couples to a third of the next, so a supernode's rows belong to several
    # ancestors and the gather map has several runs per supernode
    "chain": None,
}
_BUILT = {}
_REFS = {}


def _ld(a):
    assert np.finfo(np.longdouble).nmant >= 63, "the reference needs an extended-precision long double"
    return np.asarray(a, dtype=np.longdouble)


def spec(name):
    """(blocks, border, seed, chain) of a shape."""
    if name == "chain":
        c = SC.CASE_BY_NAME["chain"]
        return c.blocks, c.border, c.seed, c.chain
    return SHAPES[name][:4]


def classes(name):
    """The (wb, m) classes the shape must hold."""
    return () if SHAPES[name] is None else SHAPES[name][4]


def build(name):
    """(A, S, sym) of a shape, analysed with ZRELAX; made once per process and left unchanged."""
    if name not in _BUILT:
        if name == "chain":
            _BUILT[name] = SC.build(SC.CASE_BY_NAME["chain"])
        else:
            from parsy_bench_amd import inspector as I
            blocks, border, seed, chain = spec(name)
            A, S = SC.arrow(blocks, border, seed, chain)
            _BUILT[name] = (A, S, I.analyze(A, None, zrelax=SC.ZRELAX))
    return _BUILT[name]


def takahashi(L_dense):
    """Z = (L L')^-1, dense and symmetric, from the dense lower-triangular L."""
    L = np.tril(np.asarray(L_dense, dtype=np.float64))
    n = L.shape[0]
    Z = np.zeros((n, n))
    for j in range(n - 1, -1, -1):
        d = L[j, j]
        l = L[j + 1:, j] / d
        z = -(Z[j + 1:, j + 1:] @ l)
        Z[j + 1:, j] = z
        Z[j, j + 1:] = z
        Z[j, j] = 1.0 / (d * d) - l @ z
    return Z


def inverse_extended(S):
    """S^-1 in long double, symmetric; max|I - S Z| <= 64 eps(long double) asserted."""
    Sx = _ld(S)
    Z = _ld(takahashi(np.linalg.cholesky(np.asarray(S, dtype=np.float64))))
    eye = np.eye(S.shape[0], dtype=np.longdouble)
    Z = Z + Z @ (eye - Sx @ Z)
    Z = (Z + Z.T) / 2
    res = float(np.abs(eye - Sx @ Z).max())
    assert res <= 64 * float(np.finfo(np.longdouble).eps), f"the extended inverse's residual is {res:.3e}"
    return Z


def measure(Z, Zx, mask):
    """(max over the mask of |Z - Zx|_ij / (u sqrt(Zx_ii Zx_jj)), (i, j) where it falls)."""
    Zx = _ld(Zx)
    d = np.sqrt(np.diag(Zx))
    E = np.abs(_ld(Z) - Zx) / (d[:, None] * d[None, :] * _ld(U))
    E = np.where(mask, E, 0)
    i, j = np.unravel_index(int(np.argmax(E)), E.shape)
    return float(E[i, j]), (int(i), int(j))


def block_column_of(sym, j):
    """(supernode, block column in it, wb, m) of the block column that holds column j."""
    s = int(sym.col2Sup[j])
    c0, c1 = int(sym.super[s]), int(sym.super[s + 1])
    w, r = c1 - c0, int(sym.i_ptr[c1] - sym.i_ptr[c0])
    b = (j - c0) // 64
    wb = min(64, w - 64 * b)
    return s, b, wb, r - 64 * b - wb


def reference(name):
    """Everything the tests need of a shape, made once: sym, Sp (the dense matrix in the factor's ordering), d (the scaling
    in that ordering), mask (the pattern of L, diagonal included), Zx[scaled] (the extended inverse), Sv[scaled] (the dense
    values), Zt[scaled] (the restatement's Z) and rho[scaled] = measure(Zt, Zx, mask)."""
    if name not in _REFS:
        from parsy_bench_amd import inspector as I
        A, S, sym = build(name)
        seed = spec(name)[2]
        P = np.asarray(sym.Perm)
        Sp = S[np.ix_(P, P)]
        d = SC.scaling(sym.n, SCALE_SEED + seed)[P]
        mask = np.tril(I.bcsc_to_dense(sym, np.ones(int(sym.xsize))) != 0)
        Zx = inverse_extended(Sp)
        dx = _ld(d)
        ref = {"A": A, "S": S, "sym": sym, "seed": seed, "Sp": Sp, "d": d, "mask": mask,
               "Zx": {False: Zx, True: Zx / (dx[:, None] * dx[None, :])},
               "Sv": {False: Sp, True: Sp * d[:, None] * d[None, :]}, "Zt": {}, "rho": {}}
        for scaled in (False, True):
            ref["Zt"][scaled] = takahashi(np.linalg.cholesky(ref["Sv"][scaled]))
            ref["rho"][scaled] = measure(ref["Zt"][scaled], ref["Zx"][scaled], mask)
        _REFS[name] = ref
    return _REFS[name]


def values(name, scaled):
    """The values of the shape in the plan's order (A2x), plain or under the scaling."""
    ref = reference(name)
    sym = ref["sym"]
    return sym.permute_values(SC.scaled_values(ref["A"], SCALE_SEED + ref["seed"])) if scaled else sym.A2x
