"""The reference of the update / downdate tests: a plain helper module of the suite (no fixtures, no collection hooks).

* `updown_dense`: the dense numpy restatement of the column algorithm of include/parsy_amd.h -- one rotation per
  (column of L, column of W) pair, columns of L ascending, the columns of W one after the other.  It is the reference of
  the error limits: what it gives for rho_factor is what the formulas cost, whoever runs them.
* `admissible_w`: W whose columns start at given columns of L and stay inside the structure of those columns, so that the
  pattern of L does not change.
* `panel`, `entries`, `path_of`: the layout of lValues and the etree paths, restated from the symbolic arrays.
"""
from __future__ import annotations

import math

import numpy as np


def panel(sym, s):
    """(c0, w, pi, px, r) of supernode s: first column, width, offset of its row list in sym.s, offset of its panel in
    lValues, rows."""
    c0, c1 = int(sym.super[s]), int(sym.super[s + 1])
    pi = int(sym.i_ptr[c0])
    return c0, c1 - c0, pi, int(sym.p[c0]), int(sym.i_ptr[c1]) - pi


def structure(sym, j):
    """The rows of column j of L: the row list of j's supernode from j on."""
    c0, _, pi, _, r = panel(sym, int(sym.col2Sup[j]))
    return np.asarray(sym.s[pi + (j - c0): pi + r], dtype=np.int64)


def entries(sym):
    """(row, col, off, sn) of every stored entry of L (row i of a panel holds the columns c <= min(i, w - 1)) and the
    offsets of the strict upper triangles of the diagonal blocks."""
    rows, cols, offs, sns, upper = [], [], [], [], []
    s = np.asarray(sym.s)
    for k in range(sym.nsuper):
        c0, w, pi, px, r = panel(sym, k)
        ii, cc = np.tril_indices(r, 0, w)
        rows.append(s[pi + ii].astype(np.int64))
        cols.append((c0 + cc).astype(np.int64))
        offs.append(px + cc.astype(np.int64) * r + ii)
        sns.append(np.full(ii.size, k, dtype=np.int64))
        iu, cu = np.triu_indices(w, 1)
        upper.append(px + cu.astype(np.int64) * r + iu)
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(offs), np.concatenate(sns), np.concatenate(upper)


def path_of(sym, starts):
    """(supernodes, first_col): the union of the etree paths from the supernodes of the start columns (factor's
    ordering) to the root, ascending, each supernode with the smallest column it is entered at -- the start column
    itself, or the first row below the columns of the child the path comes from."""
    first = {}
    for j in starts:
        col, s = int(j), int(sym.col2Sup[int(j)])
        while True:
            first[s] = min(first.get(s, col), col)
            c0, w, pi, _, r = panel(sym, s)
            p = int(sym.sParent[s])
            if p < 0 or p == s or p >= sym.nsuper:
                break
            assert r > w and int(sym.col2Sup[int(sym.s[pi + w])]) == p, "the parent holds the first row below"
            col, s = int(sym.s[pi + w]), p
    sn = np.array(sorted(first), dtype=np.int32)
    return sn, np.array([first[int(s)] for s in sn], dtype=np.int32)


def block_columns(sym, sn, first_col):
    """Block columns of 64 columns on a path, from the one that holds the entry column on."""
    return sum(-(-panel(sym, int(s))[1] // 64) - (int(f) - panel(sym, int(s))[0]) // 64 for s, f in zip(sn, first_col))


def admissible_w(sym, starts, seed, full=False):
    """W (n x len(starts)) in the FACTOR's ordering: column t has random values in (-1, 1), none of them zero, on a
    random non-empty subset of the structure of column starts[t] of L that holds starts[t] (full=True: on all of it)."""
    rng = np.random.default_rng(seed)
    W = np.zeros((sym.n, len(starts)))
    for t, j in enumerate(starts):
        rows = structure(sym, int(j))
        assert rows[0] == j
        keep = np.ones(rows.size, dtype=bool) if full else rng.random(rows.size) < 0.6
        keep[0] = True
        v = rng.uniform(0.05, 1.0, rows.size) * rng.choice([-1.0, 1.0], rows.size)
        W[rows[keep], t] = v[keep]
    return W


def to_caller(sym, Wp):
    """W in the caller's ordering from W in the factor's (Perm[new] = old)."""
    Wc = np.zeros_like(Wp)
    Wc[np.asarray(sym.Perm)] = Wp
    return Wc


def updown_dense(L_dense, W, sign):
    """(L_new, None), or (None, j) with j the first column (0-based) whose pivot fails (r^2 <= 0 or not finite)."""
    L = np.tril(np.asarray(L_dense, dtype=np.float64)).copy()
    n = L.shape[0]
    W = np.array(W, dtype=np.float64, copy=True).reshape(n, -1)
    sigma = float(sign)
    for j in range(n):
        for t in range(W.shape[1]):
            w = W[j, t]
            if w == 0.0:
                continue
            d = L[j, j]
            r2 = d * d + sigma * w * w
            if not (r2 > 0.0 and math.isfinite(r2)):
                return None, j
            r = math.sqrt(r2)
            c, s = r / d, w / d
            L[j, j] = r
            W[j, t] = 0.0
            new = (L[j + 1:, j] + sigma * s * W[j + 1:, t]) / c
            W[j + 1:, t] = c * W[j + 1:, t] - s * new
            L[j + 1:, j] = new
    return L, None
