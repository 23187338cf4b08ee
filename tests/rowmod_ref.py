"""The reference of the row delete / row add tests: a plain helper module of the suite (no fixtures, no collection hooks).

* `rowdel_dense`, `rowadd_dense`: the dense numpy restatement of include/parsy_amd.h -- plain forward substitution in
  ascending column order, then `updown_ref.updown_dense` for the rotation pass.  It is the reference of the componentwise
  error limit: what it gives for rho_factor is what the formulas cost, whoever runs them.
* `reach_of`: the row subtree T(p), restated from the symbolic arrays.
* `may_write`: the stored entries a call on row p may write.
* `column_of`, `identity_row`: the column of the symmetric matrix in the caller's ordering, and the matrix with a row and
  column made the identity's.
"""
from __future__ import annotations

import math

import numpy as np

import updown_ref as U

_OCC = {}


def rowdel_dense(L_dense, p):
    """(L_new, None): row / column p of the dense factor made the identity's, L33 updated by the column it held."""
    L = np.tril(np.asarray(L_dense, dtype=np.float64)).copy()
    n = L.shape[0]
    w = np.zeros((n, 1))
    w[p + 1:, 0] = L[p + 1:, p]
    L[p, :p] = 0.0
    L[p, p] = 1.0
    L[p + 1:, p] = 0.0
    return U.updown_dense(L, w, +1)


def rowadd_dense(L_dense, p, a):
    """(L_new, None), or (None, j) with j the first column (0-based) whose pivot fails: j == p for the add's own.  a: the
    new column p of the symmetric matrix in the factor's ordering, dense.  Row p left of the diagonal, the diagonal and
    column p of L_dense are not read."""
    L = np.tril(np.asarray(L_dense, dtype=np.float64)).copy()
    n = L.shape[0]
    a = np.asarray(a, dtype=np.float64)
    b = a[:p].copy()
    y = np.zeros(p)
    below = a[p + 1:].copy()
    d2 = float(a[p])
    for j in range(p):                      # ascending column order: every sum takes its terms in that order
        y[j] = b[j] / L[j, j]
        if y[j] != 0.0:
            b[j + 1:] -= L[j + 1:p, j] * y[j]
            below -= L[p + 1:, j] * y[j]
            d2 -= y[j] * y[j]
    L[p, :p] = y
    L[p + 1:, p] = 0.0
    if not (d2 > 0.0 and math.isfinite(d2)):
        L[p, p] = 1.0
        return None, p
    l22 = math.sqrt(d2)
    L[p, p] = l22
    w = np.zeros((n, 1))
    w[p + 1:, 0] = below / l22
    L[p + 1:, p] = w[p + 1:, 0]
    return U.updown_dense(L, w, -1)


def _occurrences(sym):
    """row -> [(supernode, position in its row list)], ascending by supernode."""
    if id(sym) not in _OCC:
        occ = [[] for _ in range(sym.n)]
        s = np.asarray(sym.s)
        for k in range(sym.nsuper):
            _, _, pi, _, r = U.panel(sym, k)
            for i, row in enumerate(s[pi:pi + r].tolist()):
                occ[row].append((k, i))
        _OCC[id(sym)] = (sym, occ)
    return _OCC[id(sym)][1]


def reach_of(sym, p):
    """(supernodes, position, ks, height) of T(p): the supernodes whose row list holds p, ascending -- p's own with its
    leading p - c0 columns, and only when p is not its first column; height 0 without a child in T(p), else 1 + the
    largest height among its children in T(p)."""
    sn, pos, ks = [], [], []
    for k, i in _occurrences(sym)[p]:
        w = U.panel(sym, k)[1]
        cols = min(i, w)
        if cols > 0:
            sn.append(k), pos.append(i), ks.append(cols)
    height = {k: 0 for k in sn}
    for k in sn:
        par = int(sym.sParent[k])
        if par in height and par != k:
            height[par] = max(height[par], height[k] + 1)
    i32 = lambda v: np.array(v, dtype=np.int32)  # noqa: E731
    return i32(sn), i32(pos), i32(ks), i32([height[k] for k in sn])


def entries_read(sym, p):
    """Stored entries of L the row pass of an add reads: per supernode of T(p) the triangle of its ks columns and the
    rows below them."""
    sn, _, ks, _ = reach_of(sym, p)
    return sum(int(c) * (int(c) + 1) // 2 + (U.panel(sym, int(k))[4] - int(c)) * int(c) for k, c in zip(sn, ks))


def first_below(sym, p):
    """The first row below p of column p of L (None: the column ends with its diagonal)."""
    rows = U.structure(sym, p)
    return int(rows[1]) if rows.size > 1 else None


def may_write(sym, p, entries=None):
    """Boolean mask over lValues: row p in the panels of T(p), column p, and the columns of updown's path entered at the
    first row below p.  entries: updown_ref.entries(sym), where the caller holds it already."""
    mask = np.zeros(int(sym.xsize), dtype=bool)
    sn, pos, ks, _ = reach_of(sym, p)
    for k, i, c in zip(sn, pos, ks):
        _, _, _, px, r = U.panel(sym, int(k))
        mask[px + np.arange(int(c), dtype=np.int64) * r + int(i)] = True
    c0, _, _, px, r = U.panel(sym, int(sym.col2Sup[p]))
    q = p - c0
    mask[px + q * r + q: px + q * r + r] = True
    fb = first_below(sym, p)
    if fb is not None:
        row, col, off, _, _ = U.entries(sym) if entries is None else entries
        psn, pfc = U.path_of(sym, [fb])
        on = np.zeros(sym.n, dtype=bool)
        for s, f in zip(psn, pfc):
            on[int(f):int(sym.super[int(s) + 1])] = True
        mask[off[on[col]]] = True
    return mask


def column_of(S_caller, row, scale=1.0, lift=0.0):
    """(indices, values) of column `row` of the dense symmetric matrix in the caller's ordering: its non-zeros, the
    off-diagonal ones scaled, the diagonal lifted."""
    col = np.array(S_caller[:, row], dtype=np.float64)
    d = col[row]
    col *= scale
    col[row] = d + lift
    ci = np.flatnonzero(col).astype(np.int32)
    return ci, np.ascontiguousarray(col[ci])


def identity_row(S, k):
    """S with row and column k made the identity's."""
    out = np.array(S, dtype=np.float64, copy=True)
    out[k, :] = 0.0
    out[:, k] = 0.0
    out[k, k] = 1.0
    return out


def rows_to_try(sym):
    """Rows in the factor's ordering: the first and last column of every supernode, column 70 of the wide ones, 0 and
    n - 1."""
    sup = np.asarray(sym.super)
    rows = {0, sym.n - 1}
    for s in range(sym.nsuper):
        rows.update((int(sup[s]), int(sup[s + 1]) - 1))
        if sup[s + 1] - sup[s] >= 129:
            rows.add(int(sup[s]) + 70)
    return sorted(rows)
