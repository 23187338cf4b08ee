"""The cases of the sparse-solve tests: a plain helper module of the suite (no fixtures, no collection hooks).

Shapes (shape_cases.arrow, analysed with shape_cases.ZRELAX so that the engineered supernodes are the plan's) at the
borders of the constants of csrc/reach.hpp, as sparse_solve_ref.py restates them; right-hand sides by seed; selected
rows; and the catalogue: every shape once under the identity ordering with plain values and 9 right-hand sides, once under
a random ordering with the values of D A D and 8, and once with a single right-hand side of one seed.

`sp_pieces` has n = 1156, the one shape above the n <= 1000 of the other shape modules: three pieces need a supernode of
2 * 256 + 1 columns next to one of two pieces and one of exactly one.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import shape_cases as SC
import solve_cases as SV
import sparse_solve_ref as SR

P, T, R = SR.PIECE, SR.TILE, SR.ROWS

SHAPES = {s.name: s for s in [
    SV.Shape("sp_widths", ((1, 3), (2, T + 1), (15, 20), (16, 33), (17, 40), (T - 1, T), (T, T + 1), (T + 1, T + 1)), T + 2, 41,
             intent="widths 1, 2, 15, 16, 17, 63, 64, 65: tile edges; a second block column of one column"),
    SV.Shape("sp_pieces", ((2 * P + 1, 1), (P + 1, 100), (P, 129)), 130, 42,
             intent="one, two and three pieces; last pieces of one column; a piece boundary on a tile boundary"),
    SV.Shape("sp_rows", ((64, R - 1), (65, R), (17, R + 1)), R + 2, 43,
             intent="one under, at, and one over the 256-row panel workgroup"),
    SV.SHAPES["chain"],
    SV.SHAPES["subtrees_chain"],
    SV.Shape("sp_dense", (), P + 1, 44, intent="one dense supernode of 257: the reach is the root alone; pieces only"),
]}

SEEDS = ("leaf", "two_leaves", "border", "every", "empty")
XSETS = ("leaf", "border", "dozen", "all")


@dataclass(frozen=True)
class Case:
    name: str
    shape: str
    permuted: bool      # a random ordering through set_perm (else the identity)
    scaled: bool        # the values of D A D (shape_cases.scaled)
    nrhs: int
    first_seed: int     # column q of B takes SEEDS[(first_seed + q) % 5]


CASES = []
for _i, _s in enumerate(SHAPES):
    CASES += [Case(f"{_s}-id-9", _s, False, False, 9, 0), Case(f"{_s}-perm-8", _s, True, True, 8, 2),
              Case(f"{_s}-one", _s, _i % 2 == 0, _i % 4 >= 2, 1, _i % 5)]
CASE_BY_NAME = {c.name: c for c in CASES}
assert {SEEDS[c.first_seed] for c in CASES if c.nrhs == 1} >= {"leaf", "empty"}

_MADE = {}


def leaves_of(sym):
    has_child = np.zeros(sym.nsuper, dtype=bool)
    for s in range(sym.nsuper):
        p = SR.parent_of(sym, s)
        if p is not None:
            has_child[p] = True
    return [int(s) for s in np.flatnonzero(~has_child)]


def seed_rows(sym, kind, q):
    """The rows (factor's ordering, ascending) of column q of B for a seed kind."""
    sup = np.asarray(sym.super)
    col = lambda s, k: int(sup[s]) + k % int(sup[s + 1] - sup[s])  # noqa: E731
    leaves, last = leaves_of(sym), sym.nsuper - 1
    if kind == "leaf":
        rows = [col(leaves[q % len(leaves)], q + 1)]
    elif kind == "two_leaves":
        a, b = leaves[q % len(leaves)], leaves[(q + 1) % len(leaves)]
        rows = [col(a, q), col(b, q + 3)] if a != b else [col(a, q), col(a, q + 1)]
    elif kind == "border":
        rows = [col(last, q), sym.n - 1]
    elif kind == "every":
        rows = [col(s, q) for s in range(sym.nsuper)]
    else:
        rows = []
    return sorted(set(rows))


def xset_rows(sym, kind, seed=0):
    """The selected rows (factor's ordering, in the order asked for), or None for all."""
    sup = np.asarray(sym.super)
    if kind == "all":
        return None
    if kind == "leaf":
        s = leaves_of(sym)[0]
        return [int(sup[s] + (sup[s + 1] - sup[s]) // 2)]
    if kind == "border":
        return [int(sup[sym.nsuper - 1] + (sym.n - sup[sym.nsuper - 1]) // 2)]
    rows = np.random.default_rng(900 + seed).choice(sym.n, size=12, replace=False)
    if (np.diff(rows) > 0).all():
        rows = rows[::-1]
    return [int(r) for r in rows]


def make(case: Case):
    """Everything of a case that needs no device, made once per process and left unchanged: sym, the values in the
    factor's order, the dense factored matrix Sp (factor's ordering), the ordering (perm[new] = old, None: identity) and its
    inverse, B as (bp, bi, bx) in the caller's ordering and dense in the factor's (Bf), the seeds' rows per column."""
    if case.name not in _MADE:
        shape = SHAPES[case.shape]
        A, S, sym = SV.build(shape)
        assert sorted(SC.supernodes_of(sym)) == sorted(SV.engineered(shape)), (shape.name, SC.supernodes_of(sym))
        n = sym.n
        rng = np.random.default_rng(7000 + sum(map(ord, case.name)))
        perm = rng.permutation(n).astype(np.int32) if case.permuted else None
        to_caller = (lambda r: r) if perm is None else (lambda r: int(perm[r]))
        bp, bi, bx, seeds = [0], [], [], []
        Bf = np.zeros((n, case.nrhs))
        for q in range(case.nrhs):
            rows = seed_rows(sym, SEEDS[(case.first_seed + q) % len(SEEDS)], q)
            seeds.append(rows)
            vals = rng.uniform(0.5, 1.5, len(rows)) * rng.choice([-1.0, 1.0], len(rows))
            Bf[rows, q] = vals
            order = np.argsort([to_caller(r) for r in rows]) if rows else []
            bi += [to_caller(rows[k]) for k in order]
            bx += [vals[k] for k in order]
            bp.append(len(bi))
        _MADE[case.name] = dict(
            case=case, shape=shape, A=A, sym=sym, n=n, perm=perm,
            inv=None if perm is None else np.argsort(perm).astype(np.int32),
            values=SV.values(shape, A, sym, case.scaled), Sp=SV.dense(shape, S, sym, case.scaled),
            bp=np.array(bp, dtype=np.int32), bi=np.array(bi, dtype=np.int32), bx=np.array(bx, dtype=np.float64), Bf=Bf,
            seeds=seeds)
    return _MADE[case.name]


def caller_rows(made, rows):
    """Rows of the factor's ordering in the caller's (None stays None)."""
    if rows is None:
        return None
    perm = made["perm"]
    return np.array([r if perm is None else perm[r] for r in rows], dtype=np.int32)


def reaches(made, xrows):
    """(F, K) by brute force: F from the seeds of every column, K from the selected rows (factor's ordering; None: all)."""
    sym = made["sym"]
    F = SR.closure(sym, [r for rows in made["seeds"] for r in rows])
    K = list(range(sym.nsuper)) if xrows is None else SR.closure(sym, xrows)
    return F, K
