"""Engineered supernode shapes for the factor and solve kernels, and scale-invariant error measures.

A plain helper module of the suite (no fixtures, no collection hooks).  Three parts:

* `arrow`: matrices whose supernodes are made to order -- dense diagonal blocks of chosen width that couple to a chosen
  number of rows of a dense trailing border -- so that a supernode can be put at every border where a kernel changes
  behaviour (widths 16 / 32 / 64 / 128 +- 1, the 6144-entry LDS cap of the SMALL kernel, 8 / 9 updates, K extents off
  the 8- and 16-wide chunks, row counts one over a tile).  All off-diagonal values differ, so a kernel that reads the
  wrong source row cannot be right by accident.
* `rho_factor` / `rho_solve`: componentwise backward errors in units of u = 2^-53, formed in extended precision.  They are
  invariant under symmetric diagonal scaling and need no reference factor; rows that are tiny against the largest entry
  are checked as hard as the large ones (the normwise comparison of tests/test_gpu_parity.py does not see them).
* `CASES`: the catalogue -- name, blocks, border, schedule variables, and what each entry exists for.  The host tier
  (test_shape_cases_host.py) pins every entry to its schedule path; the GPU tier (test_factor_shapes_gpu.py) runs them.

Limits.  For Cholesky, |A - L L'| <= gamma_(n+1) |L||L'| componentwise (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., Thm 10.3); for substitution |b - T x| <= gamma_n |T||x| (Thm 8.5).  gamma_k = k u / (1 - k u), so in
units of u both measures are bounded by n + 1 (the (1 - k u)^-1 factor is 1 + 1e-13 at n = 1000 and rho_solve's
denominator carries |b| besides).  The bound does not depend on the order of the sums.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

U = 2.0 ** -53


# ---------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------
def _chain_set(blocks, chain):
    if chain is True:
        return set(range(len(blocks) - 1))
    if not chain:
        return set()
    out = {int(i) for i in chain}
    assert all(0 <= i < len(blocks) - 1 for i in out), "chain: block i couples to block i + 1"
    return out


def arrow_layout(blocks, border, seed, chain=False):
    """(S, supernodes): the dense symmetric matrix of `arrow` and the supernodes it is engineered to have, as
    (width, rows) in column order, the border last."""
    rng = np.random.default_rng(seed)
    blocks = [(int(w), int(k)) for w, k in blocks]
    links = _chain_set(blocks, chain)
    nb = sum(w for w, _ in blocks)
    n = nb + border
    assert border >= 1 and all(w >= 1 and 0 <= k <= border for w, k in blocks)
    mask = np.zeros((n, n), dtype=bool)
    mask[nb:, nb:] = True
    off = np.concatenate([[0], np.cumsum([w for w, _ in blocks])]).astype(int)
    below = set()        # border rows in the structure of the block before (fill passed up a chain)
    expect = []
    for i, (w, k) in enumerate(blocks):
        c0, c1 = off[i], off[i + 1]
        mask[c0:c1, c0:c1] = True
        rows = np.sort(rng.choice(border, size=k, replace=False)) + nb
        mask[np.ix_(rows, np.arange(c0, c1))] = True
        struct = set(rows.tolist()) | (below if (i - 1) in links else set())
        nxt = 0
        if i in links:
            # a random third of the next block's columns, its first column among them: the fill this block passes on
            # then reaches every column of the next block, which stays ONE supernode
            wn = blocks[i + 1][0]
            nxt = max(1, wn // 3)
            cols = np.concatenate([[0], 1 + rng.choice(wn - 1, size=nxt - 1, replace=False)]) if wn > 1 else np.array([0])
            mask[np.ix_(np.sort(cols) + c1, np.arange(c0, c1))] = True
        expect.append((w, w + nxt + len(struct)))
        below = struct
    expect.append((border, border))
    mask = mask | mask.T
    V = np.tril(rng.uniform(-1.0, 1.0, (n, n)), -1)
    S = np.where(mask, V + V.T, 0.0)
    S[np.arange(n), np.arange(n)] = np.abs(S).sum(axis=1) + rng.uniform(0.5, 1.5, n)
    if not blocks:
        expect = [(border, border)]
    return S, expect


def lower_csc(S):
    """The lower triangle of a dense symmetric matrix as the package's LowerCSC (pattern: its non-zero entries)."""
    from parsy_bench_amd.matrices import LowerCSC
    n = S.shape[0]
    Ap, Ai, Ax = [0], [], []
    for j in range(n):
        rows = np.nonzero(S[j:, j])[0] + j
        Ai.append(rows)
        Ax.append(S[rows, j])
        Ap.append(Ap[-1] + len(rows))
    return LowerCSC(n, np.array(Ap, np.int32), np.concatenate(Ai).astype(np.int32), np.concatenate(Ax).astype(np.float64))


def arrow(blocks, border, seed, chain=False):
    """(A, S): a LowerCSC and the dense symmetric matrix.  blocks = [(w, k), ...]: a dense w x w diagonal block each, all
    w columns of which couple to the same random k rows of the dense trailing border x border block.  chain=True: block
    i also couples to a random third of the columns of block i + 1 (a deeper etree, ragged gathers); chain may also be
    a collection of the indices i that do.  Off-diagonal values uniform in (-1, 1), all different; each diagonal
    entry its row's absolute sum plus uniform(0.5, 1.5).  No blocks: one dense supernode."""
    S, _ = arrow_layout(blocks, border, seed, chain)
    return lower_csc(S), S


ZRELAX = (0.0, 0.0, 0.0)   # analyse with these: the default amalgamation merges nearly full blocks into the border


def supernodes_of(sym):
    """(width, rows) of every supernode of an analysis, in column order."""
    sup = np.asarray(sym.super, dtype=np.int64)
    ip = np.asarray(sym.i_ptr, dtype=np.int64)
    return [(int(sup[s + 1] - sup[s]), int(ip[sup[s + 1]] - ip[sup[s]]) if sup[s + 1] < sym.n
             else int(sym.ssize - ip[sup[s]])) for s in range(sym.nsuper)]


# ---------------------------------------------------------------------------
# the measures
# ---------------------------------------------------------------------------
def _ld(a):
    assert np.finfo(np.longdouble).nmant >= 63, "the error measures need an extended-precision long double"
    return np.asarray(a, dtype=np.longdouble)


def rho_factor(S_perm, L_dense) -> float:
    """Componentwise backward error of a Cholesky factor in units of u = 2^-53:
    max over (|L||L'|)_ij > 0 of |S - L L'|_ij / (u (|L||L'|)_ij); where (|L||L'|)_ij == 0 the residual must be exactly 0."""
    L = np.tril(np.asarray(L_dense, dtype=np.float64))
    Lx = _ld(L)
    R = np.abs(_ld(S_perm) - Lx @ Lx.T)
    La = np.abs(L)
    G = La @ La.T
    pos = G > 0
    assert not R[~pos].any(), "a residual where |L||L'| is zero"
    return float((R[pos] / (_ld(G[pos]) * _ld(U))).max())


def rho_solve(T, x, b) -> np.ndarray:
    """Componentwise backward error of T x = b (T the dense factor or its transpose) in units of u, per column:
    max_i |b - T x|_i / (u (|T||x| + |b|)_i); rows whose denominator is 0 must have residual exactly 0."""
    T = np.asarray(T, dtype=np.float64)
    X = np.asarray(x, dtype=np.float64).reshape(T.shape[0], -1)
    B = np.asarray(b, dtype=np.float64).reshape(T.shape[0], -1)
    R = np.abs(_ld(B) - _ld(T) @ _ld(X))
    G = np.abs(T) @ np.abs(X) + np.abs(B)
    out = np.zeros(X.shape[1])
    for q in range(X.shape[1]):
        pos = G[:, q] > 0
        assert not R[~pos, q].any(), "a residual where |T||x| + |b| is zero"
        if pos.any():
            out[q] = float((R[pos, q] / (_ld(G[pos, q]) * _ld(U))).max())
    return out


def scaling(n, seed) -> np.ndarray:
    """The diagonal of D = diag(2^k), k an integer uniform in [-20, 20]."""
    return np.ldexp(1.0, np.random.default_rng(seed).integers(-20, 21, size=n))


def scaled(S, seed):
    """D S D with D = diag(scaling(n, seed)): exact (powers of two), badly scaled, exactly as well conditioned after
    equilibration."""
    d = scaling(S.shape[0], seed)
    return S * d[:, None] * d[None, :]


def scaled_values(A, seed) -> np.ndarray:
    """The values of D A D on the pattern of the LowerCSC A, in A's order."""
    d = scaling(A.n, seed)
    col = np.repeat(np.arange(A.n), np.diff(A.Ap))
    return A.Ax * d[A.Ai] * d[col]


def limit(n: int) -> int:
    return n + 1


# ---------------------------------------------------------------------------
# the catalogue
# ---------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    family: str            # a .. i as in the table below
    blocks: tuple
    border: int
    intent: str
    env: dict = field(default_factory=dict)     # schedule variables, read when the plan is built
    chain: object = False
    seed: int = 0
    expect: dict = field(default_factory=dict)  # info counter -> value, or (op, value) with op in == > >= <
    kernels: tuple = ()    # factor kernels the entry must launch (k_scatter_a: always)
    absent: tuple = ()     # ... and must not

    @property
    def n(self) -> int:
        return sum(w for w, _ in self.blocks) + self.border


_BIG = {"PARSY_PIECE_WIDTH": "128", "PARSY_BIG_MINK": "16"}
_NO_BIG = ("k_chol_big", "k_chol_dense")
_CHAIN = ("k_chol_chain",)
_TILED = ("k_chol_tiles", "k_chol_chain")

# (f) one shape for the crossings of the BIG knobs: tiled blocks of K = 130, 127, 64 (a multiple of 8 and 16), 17 and
# 25 = 8 * 3 + 1 columns whose row counts sit one over a tile, into a border of three pieces
_F_BLOCKS = ((130, 300), (127, 257), (64, 129), (200, 321), (17, 330), (25, 333))
_F_BORDER = 335
# (f) dense strips: a border of 400 = 128 + 128 + 144 columns; its first piece has 144 = 128 + 16 rows in the last one,
# a full block and a remainder of 16 rows that rides with it where a task owns 2 x 2 tiles (PARSY_BIG_SUPER=2)
_S_BLOCKS = ((144, 272), (130, 300))
_S_BORDER = 400
# (f) the groups of the pushes between a border's pieces differ between PARSY_PUSH_GROUP=1, 2 and 3 from five pieces on
_P_BLOCKS = ((130, 300), (64, 129), (17, 500), (25, 333))
_P_BORDER = 577
# (i) narrow descendants two levels below a tiled border: their streams into it are EARLY ones (complete before the level
# below the border starts), the only ones that are split; the last two blocks are chained to make the middle level
_I_BLOCKS = tuple([(40, 200)] * 16 + [(40, 150), (40, 100)])
_I_BORDER = 256

CASES = [
    # ---- a. narrow widths around 16 / 32 / 64, every panel within the LDS cap ------------------------------------------
    Case("narrow_lo", "a", ((1, 7), (2, 39), (15, 33), (16, 17), (17, 39)), 40,
         "widths 1, 2, 15, 16, 17; 5 updates into a border that stays SMALL",
         expect={"n_small": 6, "n_big": 0}, kernels=("k_chol_small",), absent=_TILED + _NO_BIG + ("k_chol_chain_rows",)),
    Case("narrow_hi", "a", ((31, 62), (32, 33), (33, 63), (63, 34), (64, 32), (16, 1), (17, 9), (1, 63)), 64,
         "widths 31, 32, 33, 63, 64; 8 updates: the most a border takes and stays SMALL", seed=1,
         expect={"n_small": 9, "n_big": 0}, kernels=("k_chol_small",), absent=_TILED + _NO_BIG + ("k_chol_chain_rows",)),
    Case("narrow_nine", "a", ((31, 62), (32, 33), (33, 63), (63, 34), (64, 32), (16, 1), (17, 9), (1, 63), (2, 5)), 64,
         "the same with a ninth update: the 64-column border goes tiled", seed=1,
         expect={"n_small": 9, "n_big": 1}, kernels=("k_chol_small",) + _CHAIN, absent=_NO_BIG),
    # ---- b. the LDS cap w * r == 6144 -----------------------------------------------------------------------------------
    Case("cap_at", "b", ((64, 32), (48, 80), (32, 160), (16, 368)), 400,
         "w * r == 6144 exactly: the largest SMALL panels of widths 64, 48, 32, 16", seed=2,
         expect={"n_small": 4, "n_big": 1}, kernels=("k_chol_small",) + _CHAIN, absent=_NO_BIG),
    Case("cap_over", "b", ((64, 33), (48, 81), (32, 161), (16, 369)), 400,
         "one row more: narrow, tall TILED supernodes (one block column, up to 7 tile rows)", seed=2,
         expect={"n_small": 0, "n_big": 5}, kernels=_CHAIN, absent=("k_chol_small",) + _NO_BIG),
    # ---- c. tile edges: widths and rows below around 64 / 128 / 192 / 256 ----------------------------------------------
    Case("tiles_70", "c", ((65, 1), (96, 63), (127, 64), (128, 65), (129, 69)), 70,
         "widths 65, 96, 127, 128, 129 over 1, 63, 64, 65, 69 rows; border of 70: one block column and six columns", seed=3,
         expect={"n_small": 0, "n_big": 6}, kernels=_CHAIN, absent=("k_chol_small",) + _NO_BIG),
    Case("tiles_130", "c", ((191, 127), (192, 129), (193, 63), (129, 1)), 130,
         "widths 191, 192, 193 over 127, 129, 63 rows; border of 130", seed=4,
         expect={"n_small": 0, "n_big": 5}, kernels=_CHAIN, absent=("k_chol_small",) + _NO_BIG),
    Case("tiles_257", "c", ((257, 65), (65, 100), (127, 100)), 130,
         "width 257 (five block columns, the last one column wide); the last two blocks chained: EARLY streams (TILES)",
         seed=5, chain=(1,), expect={"n_small": 0, "n_big": 4}, kernels=_TILED, absent=("k_chol_small",) + _NO_BIG),
    # ---- d. one dense supernode -----------------------------------------------------------------------------------------
    Case("dense_64", "d", (), 64, "one supernode of exactly one tile (4096 entries: SMALL)", seed=6,
         expect={"n_small": 1, "n_big": 0}, kernels=("k_chol_small",), absent=_TILED + _NO_BIG),
    Case("dense_65", "d", (), 65, "one column over a tile: tiled, whatever the entry count", seed=7,
         expect={"n_small": 0, "n_big": 1}, kernels=_CHAIN, absent=("k_chol_small", "k_chol_tiles") + _NO_BIG),
    Case("dense_128", "d", (), 128, "two block columns, no update: the chain alone", seed=8,
         expect={"n_small": 0, "n_big": 1}, kernels=_CHAIN, absent=("k_chol_small", "k_chol_tiles") + _NO_BIG),
    Case("dense_129", "d", (), 129, "two block columns and one column", seed=9,
         expect={"n_small": 0, "n_big": 1}, kernels=_CHAIN, absent=("k_chol_small", "k_chol_tiles") + _NO_BIG),
    Case("dense_257", "d", (), 257, "four block columns and one column", seed=10,
         expect={"n_small": 0, "n_big": 1}, kernels=_CHAIN, absent=("k_chol_small", "k_chol_tiles") + _NO_BIG),
    # ---- e. a chain of blocks: deeper etree, ragged relative indices ---------------------------------------------------
    Case("chain", "e", ((17, 20), (33, 30), (65, 25), (129, 40), (64, 30)), 100,
         "widths 17, 33, 65, 129, 64 each coupled to a third of the next: six levels, SMALL into tiled, EARLY streams",
         seed=11, chain=True, expect={"nlevels": 6}, kernels=("k_chol_small",) + _TILED, absent=_NO_BIG),
    # ---- f. BIG launches and pieces (PARSY_PIECE_WIDTH=128, PARSY_BIG_MINK=16) -----------------------------------------
    Case("big_ragged", "f", _F_BLOCKS, _F_BORDER, "PARSY_BIG_DENSE=0: every BIG entry through the ragged kernel", seed=12,
         env={**_BIG, "PARSY_BIG_DENSE": "0", "PARSY_PUSH_GROUP": "1"},
         expect={"big_tasks": (">", 0), "dense_entries": 0, "dense_tasks": 0, "n_pieces": (">", 7)},
         kernels=("k_chol_big",) + _CHAIN, absent=("k_chol_dense",)),
    Case("big_dense2", "f", _F_BLOCKS, _F_BORDER, "PARSY_BIG_DENSE=2: full blocks through k_chol_dense, the rest ragged",
         seed=12, env={**_BIG, "PARSY_BIG_DENSE": "2", "PARSY_BIG_SUPER": "2", "PARSY_PUSH_GROUP": "2"},
         expect={"big_tasks": (">", 0), "dense_entries": (">", 0), "dense_tasks": (">", 0)},
         kernels=("k_chol_big", "k_chol_dense") + _CHAIN),
    Case("big_dense4", "f", _F_BLOCKS, _F_BORDER,
         "PARSY_BIG_DENSE=4: every entry of K >= 8 through k_chol_dense -- ragged windows, K tails of 17 and 25", seed=12,
         env={**_BIG, "PARSY_BIG_DENSE": "4", "PARSY_BIG_SUPER": "2x1", "PARSY_DENSE_STRIPS": "0", "PARSY_PUSH_GROUP": "3"},
         expect={"big_tasks": (">", 0), "dense_tasks": (">", 0), "dense_strip_entries": 0},
         kernels=("k_chol_dense",) + _CHAIN),
    Case("big_strips", "f", _S_BLOCKS, _S_BORDER, "remainders of 16 and 8 rows ride with their full blocks (strips)", seed=13,
         env={**_BIG, "PARSY_BIG_DENSE": "2", "PARSY_BIG_SUPER": "2"},
         expect={"dense_strip_entries": (">", 0), "dense_tasks": (">", 0)}, kernels=("k_chol_big", "k_chol_dense") + _CHAIN),
    Case("big_no_strips", "f", _S_BLOCKS, _S_BORDER, "the same without strips (PARSY_DENSE_STRIPS=0)", seed=13,
         env={**_BIG, "PARSY_BIG_DENSE": "2", "PARSY_BIG_SUPER": "2", "PARSY_DENSE_STRIPS": "0"},
         expect={"dense_strip_entries": 0, "dense_tasks": (">", 0)}, kernels=("k_chol_big", "k_chol_dense") + _CHAIN),
    Case("push_1", "f", _P_BLOCKS, _P_BORDER, "a border of five pieces, every piece pushes by itself (PARSY_PUSH_GROUP=1)", seed=16,
         env={**_BIG, "PARSY_BIG_DENSE": "2", "PARSY_PUSH_GROUP": "1"},
         expect={"n_pieces": 9, "big_tasks": (">", 0)}, kernels=("k_chol_big", "k_chol_dense") + _CHAIN),
    Case("push_2", "f", _P_BLOCKS, _P_BORDER, "... in aligned groups of two", seed=16,
         env={**_BIG, "PARSY_BIG_DENSE": "2", "PARSY_PUSH_GROUP": "2"},
         expect={"n_pieces": 9, "big_tasks": (">", 0)}, kernels=("k_chol_big", "k_chol_dense") + _CHAIN),
    Case("push_3", "f", _P_BLOCKS, _P_BORDER, "... of three", seed=16,
         env={**_BIG, "PARSY_BIG_DENSE": "2", "PARSY_PUSH_GROUP": "3"},
         expect={"n_pieces": 9, "big_tasks": (">", 0)}, kernels=("k_chol_big", "k_chol_dense") + _CHAIN),
    # ---- g. two chain launches per level (PARSY_CHAIN_SPLIT=2) ---------------------------------------------------------
    Case("tiles_130_split", "g", ((191, 127), (192, 129), (193, 63), (129, 1)), 130,
         "tiles_130 with the rows below the diagonal squares in a launch of their own", seed=4,
         env={"PARSY_CHAIN_SPLIT": "2"}, expect={"n_small": 0, "n_big": 5},
         kernels=_CHAIN + ("k_chol_chain_rows",), absent=("k_chol_small",) + _NO_BIG),
    Case("big_ragged_split", "g", _F_BLOCKS, _F_BORDER, "big_ragged likewise", seed=12,
         env={**_BIG, "PARSY_BIG_DENSE": "0", "PARSY_PUSH_GROUP": "1", "PARSY_CHAIN_SPLIT": "2"},
         expect={"big_tasks": (">", 0), "dense_entries": 0},
         kernels=("k_chol_big", "k_chol_chain_rows") + _CHAIN, absent=("k_chol_dense",)),
    # ---- h. subtree launches --------------------------------------------------------------------------------------------
    Case("subtrees", "h", tuple((1 + (7 * i) % 16, 1 + (11 * i) % 39) for i in range(40)), 40,
         "40 blocks of widths 1 .. 16, one workgroup each (PARSY_SUBTREES=1); a border of 40 with 40 updates: tiled",
         seed=14, env={"PARSY_SUBTREES": "1"}, expect={"chol_subtrees": 40, "n_small": 40, "n_big": 1},
         kernels=("k_chol_small",) + _CHAIN, absent=_NO_BIG),
    # ---- i. split early streams -----------------------------------------------------------------------------------------
    Case("streams_split", "i", _I_BLOCKS, _I_BORDER,
         "16 sources of K = 40 two levels below a tiled border: early streams of 48 chunks cut into parts of 8 (tile scratch)",
         seed=15, chain=(16,), env={"PARSY_SPLIT_CHUNKS": "8", "PARSY_SPLIT_TARGET": "8", "PARSY_SPLIT_MAX": "8"},
         expect={"split_tiles": (">", 0), "split_parts": (">", 0)}, kernels=_TILED, absent=_NO_BIG),
    Case("streams_whole", "i", _I_BLOCKS, _I_BORDER, "the same streams, never split", seed=15, chain=(16,),
         env={"PARSY_SPLIT_CHUNKS": "1000000"}, expect={"split_tiles": 0, "split_parts": 0}, kernels=_TILED, absent=_NO_BIG),
]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES) and all(c.n <= 1000 for c in CASES)

# every variable a catalogue entry may set: a test clears them all before it applies an entry's
VARIABLES = ("PARSY_PIECE_WIDTH", "PARSY_BIG_MINK", "PARSY_BIG_DENSE", "PARSY_BIG_SUPER", "PARSY_DENSE_STRIPS", "PARSY_PUSH_GROUP",
             "PARSY_CHAIN_SPLIT", "PARSY_SUBTREES", "PARSY_SPLIT_CHUNKS", "PARSY_SPLIT_TARGET", "PARSY_SPLIT_MAX", "PARSY_SOLVE_ONE")

FACTOR_KERNELS = ("k_scatter_a", "k_chol_small", "k_chol_tiles", "k_chol_chain", "k_chol_chain_rows", "k_chol_big", "k_chol_dense")

_BUILT = {}


def build(case: Case):
    """(A, S, sym) of a catalogue entry, made once per process and left unchanged."""
    from parsy_bench_amd import inspector as I
    key = (case.blocks, case.border, case.seed, repr(case.chain))
    if key not in _BUILT:
        A, S = arrow(case.blocks, case.border, case.seed, case.chain)
        _BUILT[key] = (A, S, I.analyze(A, None, zrelax=ZRELAX))
    return _BUILT[key]


def set_env(monkeypatch, env):
    for k in VARIABLES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def holds(value, want) -> bool:
    if not isinstance(want, tuple):
        return value == want
    op, ref = want
    return {"==": value == ref, ">": value > ref, ">=": value >= ref, "<": value < ref}[op]
