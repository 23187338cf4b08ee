"""The reference of the sparse-solve tests: a plain helper module of the suite (no fixtures, no collection hooks).

Everything here is restated from the symbolic arrays (sym.sParent, sym.col2Sup, sym.super, sym.i_ptr) by brute force,
independently of csrc/reach.cpp:

* `closure`: the supernodes of a set of rows (factor's ordering) and all their ancestors.
* `pieces_of`, `steps_of`: the pieces of a supernode and the step of every piece of a closed set -- a supernode's first
  piece one step after the last pieces of its children in the set, piece k + 1 one step after piece k.
* `entries_of`: the stored entries of L a pass over a set reads.
* `kernels_of`: the kernels one device call enqueues.
* `dense_factor`: the dense L of a factor in lValues layout.
* `rho_spd`: the componentwise backward error of x against the factored matrix, in units of u.

The constants are the ones of csrc/reach.hpp; the shapes of sparse_solve_cases.py sit at their borders and move with them.
"""
from __future__ import annotations

import numpy as np

import shape_cases as SC
import updown_ref as U

PIECE = 256    # kSparsePiece
BLOCK = 8      # kSparseBlock
TILE = 64      # kSparseTile
ROWS = 256     # kSparseRows
COLS = 4       # kSparseCols
SEG = 1024     # kSparseSeg
OPS = {"A": 0, "GINV": 1, "GINVT": 2}


def parent_of(sym, s):
    """The parent of supernode s in the supernodal etree, or None for a root."""
    p = int(sym.sParent[s])
    return None if (p < 0 or p >= sym.nsuper or p == s) else p


def closure(sym, rows):
    """Sorted list: the supernodes of `rows` (factor's ordering) and all their ancestors."""
    out = set()
    for j in rows:
        s = int(sym.col2Sup[int(j)])
        while s is not None:
            out.add(s)
            s = parent_of(sym, s)
    return sorted(out)


def is_closed(sym, sn):
    have = set(int(s) for s in sn)
    return all(parent_of(sym, s) is None or parent_of(sym, s) in have for s in have)


def pieces_of(w):
    """[(first column, columns)] of a supernode of width w."""
    return [(c, min(PIECE, w - c)) for c in range(0, w, PIECE)]


def steps_of(sym, sn):
    """{(supernode, piece): step} of a closed set, by the rule alone (children found by scanning the whole etree)."""
    have = set(int(s) for s in sn)
    step = {}

    def first(s):
        kids = [c for c in have if parent_of(sym, c) == s]
        return 0 if not kids else 1 + max(last(c) for c in kids)

    def last(s):
        if (s, 0) not in step:
            f = first(s)
            for k in range(len(pieces_of(U.panel(sym, s)[1]))):
                step[(s, k)] = f + k
        return step[(s, len(pieces_of(U.panel(sym, s)[1])) - 1)]

    for s in sorted(have):
        last(s)
    return step


def counts_of(sym, sn):
    """(supernodes, pieces, steps, entries) of a pass over a closed set."""
    step = steps_of(sym, sn)
    ent = 0
    for s in sn:
        _, w, _, _, r = U.panel(sym, int(s))
        ent += w * (w + 1) // 2 + (r - w) * w
    return len(sn), len(step), (1 + max(step.values()) if step else 0), ent


def kernels_of(sym, F, K, op):
    """Kernels of one device call: the load, the gather and the clearing; per step of a pass its triangles and -- where a
    piece of the step has panel rows below its columns -- its panels."""
    k = 3
    for sn, runs in ((F, op != OPS["GINVT"]), (K, op != OPS["GINV"])):
        if not runs:
            continue
        step = steps_of(sym, sn)
        below = {}
        for (s, p), t in step.items():
            _, w, _, _, r = U.panel(sym, s)
            c0, nc = pieces_of(w)[p]
            below[t] = below.get(t, False) or r - (c0 + nc) > 0
        k += sum(2 if b else 1 for b in below.values())
    return k


def dense_factor(sym, lv):
    row, col, off, _, _ = U.entries(sym)
    L = np.zeros((sym.n, sym.n))
    L[row, col] = np.asarray(lv)[off]
    return L


def rho_spd(L, x, b):
    """max_i |b - L L' x|_i / (u (|L||L'||x| + |b|)_i) per column, in extended precision with the factor as given; rows
    whose denominator is 0 must have residual exactly 0.  Higham, Thm 10.4: <= 3 n + 2 for a solve through the factor."""
    Lx = SC._ld(L)
    X = np.asarray(x, dtype=np.float64).reshape(L.shape[0], -1)
    B = np.asarray(b, dtype=np.float64).reshape(L.shape[0], -1)
    R = np.abs(SC._ld(B) - Lx @ (Lx.T @ SC._ld(X)))
    G = np.abs(L) @ (np.abs(L).T @ np.abs(X)) + np.abs(B)
    out = np.zeros(X.shape[1])
    for q in range(X.shape[1]):
        pos = G[:, q] > 0
        assert not R[~pos, q].any(), "a residual where |L||L'||x| + |b| is zero"
        if pos.any():
            out[q] = float((R[pos, q] / (SC._ld(G[pos, q]) * SC._ld(SC.U))).max())
    return out


def columns_of(sym, sn):
    """The columns of a list of supernodes, ascending."""
    sup = np.asarray(sym.super)
    return np.concatenate([np.arange(int(sup[s]), int(sup[s + 1])) for s in sn]) if len(sn) else np.zeros(0, dtype=np.int64)
