"""Dense numpy restatements for the normal-matrix tests (N = F diag(w) F' + beta I + A0 on the plan's pattern, the
products by F and F', least squares through the factor): the matrices the tests use, the exact values in long double,
and the limits of include/parsy_amd.h's sums.  With u = 2^-53 and any order of the sums (Higham, Accuracy and Stability,
section 3.1):

  an entry of N   |computed - exact| <= (l_q + 4) u (sum |fx_a||w_k||fx_b| + |beta| + |A0_q|),   l_q the length of its list
  a product row   |computed - exact| <= (c + 3) u (|alpha| sum |F||w||x| + |beta_y||y|),         c the number of terms

and where the bound is 0 the result is exact.  No measured number enters a tolerance."""
import numpy as np

from parsy_bench_amd.matrices import ColumnsCSC, LowerCSC

U = 2.0 ** -53
_CACHE = {}


def ld(a):
    assert np.finfo(np.longdouble).nmant >= 63, "the limits need an extended-precision long double"
    return np.asarray(a, dtype=np.longdouble)


def from_dense(D) -> ColumnsCSC:
    """The non-zeros of a dense n x m array as F."""
    D = np.asarray(D, dtype=np.float64)
    cols = [np.flatnonzero(D[:, k]) for k in range(D.shape[1])]
    ptr = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int32)
    idx = (np.concatenate(cols) if cols else np.zeros(0)).astype(np.int32)
    dat = np.concatenate([D[c, k] for k, c in enumerate(cols)]) if cols else np.zeros(0)
    return ColumnsCSC(D.shape[0], D.shape[1], ptr, idx, np.ascontiguousarray(dat, dtype=np.float64))


def column_of(F) -> np.ndarray:
    return np.repeat(np.arange(F.m), np.diff(F.indptr))


def pattern_lower(n, F) -> LowerCSC:
    """The pattern of (|F||F|' + I), lower triangle, from numpy (what parsy_normal_pattern must return)."""
    B = (from_dense_abs(F) @ from_dense_abs(F).T + np.eye(n)) > 0
    Ap, Ai = [0], []
    for j in range(n):
        rows = np.flatnonzero(B[j:, j]) + j
        Ai.extend(rows.tolist())
        Ap.append(len(Ai))
    return LowerCSC(n, np.array(Ap, np.int32), np.array(Ai, np.int32), np.ones(len(Ai)))


def from_dense_abs(F) -> np.ndarray:
    D = np.zeros((F.n, F.m))
    D[F.indices, column_of(F)] = 1.0
    return D


def analysed(F, seed=None):
    """sym of the pattern of F F' (through NormalEquations.pattern) under a random ordering (seed) or nested dissection
    (None)."""
    from parsy_bench_amd import api, inspector as I
    Ap, Ai = api.NormalEquations.pattern(F.n, F)
    A = LowerCSC(F.n, Ap, Ai, np.ones(Ai.size))
    perm = I.order_nd(A) if seed is None else np.random.default_rng(seed).permutation(F.n).astype(np.int32)
    return I.analyze(A, perm)


def entry_coords(plan):
    """(i, j) of every A2 entry in the CALLER's ordering (i is the row of the factor's ordering, j its column)."""
    pat = plan.pattern()
    P = np.asarray(plan.sym.Perm, dtype=np.int64)
    return P[pat["row"]], P[pat["col"]]


def exact_values(F, fx, w, beta, base, ci, cj, lengths):
    """(exact, limit) per A2 entry, long double: the entries (ci, cj) of F diag(w) F' + beta I + A0 and the limit above."""
    D = np.zeros((F.n, F.m), dtype=np.longdouble)
    D[F.indices, column_of(F)] = ld(fx)
    wl = ld(np.ones(F.m) if w is None else w)
    Nx = (D * wl) @ D.T
    Na = (np.abs(D) * np.abs(wl)) @ np.abs(D).T
    exact, mag = Nx[ci, cj], Na[ci, cj]
    diag = ci == cj
    exact = exact + np.where(diag, ld(beta), ld(0.0))
    mag = mag + np.where(diag, abs(ld(beta)), ld(0.0))
    if base is not None:
        exact, mag = exact + ld(base), mag + np.abs(ld(base))
    return exact, (ld(lengths) + 4) * ld(U) * mag


def restated_values(ne, fx, w, beta=0.0, base=None):
    """The sum as the library defines it, restated from pairs(q) in float64 with the library's rounding: fma is not
    available in numpy, so the restatement is exact only where every product is (the grid generators: +-1, 0 / 1)."""
    nnz = int(ne.plan.info["nnzA"])
    pat = ne.plan.pattern()
    out = np.zeros(nnz)
    for q in range(nnz):
        a, b, k = ne.pairs(q)
        s = 0.0
        for t in range(a.size):
            s += (fx[a[t]] * (1.0 if w is None else w[k[t]])) * fx[b[t]]
        if pat["row"][q] == pat["col"][q]:
            s += beta
        if base is not None:
            s += base[q]
        out[q] = s
    return out


def product_exact(F, fx, w, op, X, alpha, beta_y, Y):
    """(exact, limit), long double, of Y = beta_y Y + alpha op(X); op "F": F diag(w) X, "FT": F' X (w not used)."""
    D = np.zeros((F.n, F.m), dtype=np.longdouble)
    D[F.indices, column_of(F)] = ld(fx)
    if op == "F":
        wl = ld(np.ones(F.m) if w is None else w)
        T = D * wl
    else:
        T = D.T
    terms = (T != 0).sum(axis=1).reshape(-1, 1)
    Y0 = ld(np.zeros((T.shape[0], X.shape[1])) if Y is None or beta_y == 0.0 else Y)
    exact = ld(beta_y) * Y0 + ld(alpha) * (T @ ld(X))
    mag = abs(ld(beta_y)) * np.abs(Y0) + abs(ld(alpha)) * (np.abs(T) @ np.abs(ld(X)))
    if op == "F":   # (the count of terms is the row's entries of F, zero weights included)
        terms = (D != 0).sum(axis=1).reshape(-1, 1)
    return exact, (ld(terms) + 3) * ld(U) * mag


def within(got, exact, limit):
    """Largest |got - exact| / limit over the entries with a positive limit; entries whose limit is 0 must be exact."""
    err = np.abs(ld(got) - exact)
    zero = limit == 0
    assert not err[zero].any(), "an entry whose bound is 0 is not exact"
    return float((err[~zero] / limit[~zero]).max()) if (~zero).any() else 0.0


# ---- the engineered matrices ------------------------------------------------------------------------------------------
def borders(borders_of_info=(8, 64, 512)):
    """F (64 x 1100): per length T in {L - 1, L, L + 1 : L a class border} and {511, 512, 513, 1025} a dedicated pair of
    rows (2 p, 2 p + 1) that share exactly T columns (both rows hold the same run of T columns and nothing else), so the
    off-diagonal list of the pair and both diagonal lists have T triples; random short columns over rows 20 .. 61; row 63
    is empty, column 1098 is empty, column 1099 has a single entry."""
    key = ("borders", tuple(borders_of_info))
    if key not in _CACHE:
        n, m = 64, 1100
        lens = sorted({L + d for L in borders_of_info for d in (-1, 0, 1)} | {511, 512, 513, 1025})
        assert 2 * len(lens) <= 20 and max(lens) <= m - 2
        rng = np.random.default_rng(41)
        D = np.zeros((n, m))
        for p, T in enumerate(lens):
            s0 = (97 * p) % (m - 2 - T + 1)
            D[2 * p:2 * p + 2, s0:s0 + T] = rng.uniform(0.25, 1.0, (2, T)) * rng.choice([-1.0, 1.0], (2, T))
        for k in range(m - 2):
            rows = rng.choice(np.arange(20, 62), size=int(rng.integers(0, 4)), replace=False)
            D[rows, k] = rng.uniform(0.25, 1.0, rows.size) * rng.choice([-1.0, 1.0], rows.size)
        D[40, m - 1] = 0.75
        assert not D[63].any() and not D[:, m - 2].any()
        _CACHE[key] = (from_dense(D), lens)
    return _CACHE[key]


def tall():
    """F (330 x 420): column 0 holds rows 0 .. 299 (45 150 pairs); the others are the edges of a path over all rows and
    random 2- and 3-row columns: short."""
    if "tall" not in _CACHE:
        n, m = 330, 420
        rng = np.random.default_rng(43)
        D = np.zeros((n, m))
        D[:300, 0] = rng.uniform(0.25, 1.0, 300) * rng.choice([-1.0, 1.0], 300)
        for k in range(1, n):
            D[k - 1, k], D[k, k] = 1.0, -rng.uniform(0.5, 1.0)
        for k in range(n, m):
            rows = rng.choice(n, size=int(rng.integers(2, 4)), replace=False)
            D[rows, k] = rng.uniform(0.25, 1.0, rows.size)
        _CACHE["tall"] = from_dense(D)
    return _CACHE["tall"]


def well_conditioned():
    """F (60 x 240), three entries per column, every row in the first 60 columns' diagonal: with w in [0.5, 1.5] and
    beta = 0.5 the normal matrix is well conditioned."""
    if "wc" not in _CACHE:
        n, m = 60, 240
        rng = np.random.default_rng(47)
        D = np.zeros((n, m))
        for k in range(m):
            rows = np.unique(np.concatenate([[k % n], rng.choice(n, size=2, replace=False)]))
            D[rows, k] = rng.uniform(0.25, 1.0, rows.size) * rng.choice([-1.0, 1.0], rows.size)
        _CACHE["wc"] = from_dense(D)
    return _CACHE["wc"]


# ---- least squares ----------------------------------------------------------------------------------------------------
def lstsq_float64(F, fx, w, beta, C, steps, w_factor=None):
    """The loop of parsy_lsq_solve_device in float64 with a dense Cholesky factor (of the normal matrix at w_factor,
    default w): x = S F W c, then `steps` corrections."""
    D = np.zeros((F.n, F.m))
    D[F.indices, column_of(F)] = fx
    wf = w if w_factor is None else w_factor
    L = np.linalg.cholesky((D * wf) @ D.T + beta * np.eye(F.n))

    def S(b):
        return np.linalg.solve(L.T, np.linalg.solve(L, b))
    X = S((D * w) @ C)
    for _ in range(steps):
        R = C - D.T @ X
        X = X + S((D * w) @ R - beta * X)
    return X


def rho_g(F, fx, w, beta, C, X) -> float:
    """The scaled gradient of the returned X in units of u: max_i |g_i| / (u (|F||w||r| + |beta||x|)_i) with r = c - F' x
    and g = F W r - beta x in long double."""
    D = np.zeros((F.n, F.m), dtype=np.longdouble)
    D[F.indices, column_of(F)] = ld(fx)
    Xl, wl = ld(X).reshape(F.n, -1), ld(w)
    R = ld(C).reshape(F.m, -1) - D.T @ Xl
    G = (D * wl) @ R - ld(beta) * Xl
    den = ld(U) * ((np.abs(D) * np.abs(wl)) @ np.abs(R) + abs(ld(beta)) * np.abs(Xl))
    assert (den > 0).all()
    return float((np.abs(G) / den).max())
