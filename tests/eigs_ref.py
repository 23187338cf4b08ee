"""A dense numpy restatement of parsy_eigs_device (csrc/eigs.hpp): the block Davidson iteration for the smallest
eigenpairs of A v = lambda M v with (L L')^-1 as preconditioner, thick restart, residual-form expansion, two projection
passes and two passes of Cholesky-QR in the M inner product with the library's drop rule.  Same sources, same padding
with the Ritz pairs beyond k, same restart and the same stopping rule; the small dense work is numpy's (eigh, cholesky)
where the library runs eigs_dense.hpp.  It is the reference of tests/test_eigs_gpu.py and also holds the inputs and the
measures both tiers share."""
import numpy as np

U = 2.0 ** -53
DROP = 2.0 ** -26          # kEigsDropPivot of eigs_dense.hpp: sqrt(u) in the unit-diagonal scaling
MAX_ITER = 200
# (k, block, max_basis) of the issue, (6, 6, 36) with M = I only, and one with the widest block (it meets the same
# condition: test_eigs_host.py)
CONFIGS = [(6, 4, 24), (1, 1, 12), (9, 8, 40), (5, 4, 24), (6, 6, 36), (8, 16, 48)]
IDENTITY_ONLY = {(6, 6, 36)}
GRIDS = {"grid12x12": (12, 12, 1), "grid24x17": (24, 17, 1), "grid8x8x8": (8, 8, 8)}
SHAPE_NAMES = ["edges", "wide", "chain"]
INPUTS = SHAPE_NAMES + list(GRIDS)
TOLS = [1e-10, 1e-12]


class NotSpd(Exception):
    pass


def ld(a):
    assert np.finfo(np.longdouble).nmant >= 63, "the measures need an extended-precision long double"
    return np.asarray(a, dtype=np.longdouble)


# ---- inputs -------------------------------------------------------------------------------------------------------
def full_dense(A, Ax=None):
    """Both triangles, dense, of the values Ax (default A's own) on the pattern of the LowerCSC A."""
    Ax = A.Ax if Ax is None else Ax
    col = np.repeat(np.arange(A.n), np.diff(A.Ap))
    S = np.zeros((A.n, A.n))
    S[A.Ai, col] = Ax
    S[col, A.Ai] = Ax
    return S


def mass_values(A, seed=5):
    """A diagonally dominant positive M on A's pattern, in A's order: off-diagonal entries uniform in (0.05, 0.25), each
    diagonal entry its row's sum plus uniform(1, 2)."""
    rng = np.random.default_rng(seed)
    col = np.repeat(np.arange(A.n), np.diff(A.Ap))
    off = A.Ai != col
    v = np.where(off, rng.uniform(0.05, 0.25, A.Ai.size), 0.0)
    rows = np.zeros(A.n)
    np.add.at(rows, A.Ai[off], v[off])
    np.add.at(rows, col[off], v[off])
    v[~off] = rows[A.Ai[~off]] + rng.uniform(1.0, 2.0, A.n)
    return v


def stale_values(A, seed=9, rel=0.02):
    """A + D in A's order: D diagonal, up to `rel` of diag A."""
    rng = np.random.default_rng(seed)
    col = np.repeat(np.arange(A.n), np.diff(A.Ap))
    v = A.Ax.copy()
    dg = A.Ai == col
    v[dg] *= 1.0 + rng.uniform(0.0, rel, int(dg.sum()))
    return v


def start_block(n, block):
    return np.random.default_rng(0).standard_normal((n, block))


_INPUTS = {}


def make_input(name):
    """(A, sym) of a named input: the engineered shapes of test_updown_gpu.py, or a 5- / 7-point grid under nested
    dissection.  Cached."""
    if name not in _INPUTS:
        import shape_cases as SC
        from parsy_bench_amd import inspector as I, matrices as M
        if name in GRIDS:
            nx, ny, nz = GRIDS[name]
            A = M.grid_spd(nx, ny, nz, 5 if nz == 1 else 7)
            sym = I.analyze(A, M.grid_nd(nx, ny, nz))
        else:
            from test_updown_gpu import SHAPES
            spec = SHAPES[name]
            A = SC.arrow(spec["blocks"], spec["border"], spec["seed"], spec["chain"])[0]
            sym = I.analyze(A, None, zrelax=SC.ZRELAX)
        _INPUTS[name] = (A, sym)
    return _INPUTS[name]


_DENSE = {}


def dense_case(name):
    """{A, sym, Ad, Md, Ast (A + D), max_row, and per (stale, mass) the reference spectrum}, cached."""
    if name not in _DENSE:
        A, sym = make_input(name)
        Ad = full_dense(A)
        c = dict(A=A, sym=sym, Ad=Ad, Md=full_dense(A, mass_values(A)), Ast=full_dense(A, stale_values(A)),
                 max_row=int((Ad != 0).sum(axis=1).max()), spectrum={}, Kinv=np.linalg.inv(Ad))
        _DENSE[name] = c
    return _DENSE[name]


def spectrum(case, stale, mass):
    key = (bool(stale), bool(mass))
    if key not in case["spectrum"]:
        case["spectrum"][key] = reference_spectrum(case["Ast"] if stale else case["Ad"], case["Md"] if mass else None)
    return case["spectrum"][key]


def runs():
    """(configuration, mass) pairs both tiers run."""
    return [(cfg, mass) for cfg in CONFIGS for mass in (False, True) if not (mass and cfg in IDENTITY_ONLY)]


def default_basis(n, k, block):
    return min(max(3 * k, k + 4 * block), n, 128)


def reference_spectrum(Ad, Md):
    """Ascending eigenvalues of the pencil by numpy eigh through M's Cholesky factor."""
    if Md is None:
        return np.linalg.eigvalsh(Ad)
    C = np.linalg.cholesky(Md)
    X = np.linalg.solve(C, np.linalg.solve(C, Ad).T)
    return np.linalg.eigvalsh((X + X.T) / 2)


# ---- the restatement ----------------------------------------------------------------------------------------------
def _orthonormalise(T, V, MV, mul_m, it):
    """Two projection passes against V, two passes of Cholesky-QR in the M inner product; (T, dropped)."""
    dropped = 0
    for _ in range(2):
        if V.shape[1]:
            T = T - V @ (MV.T @ T)
    for p in range(2):
        G = T.T @ mul_m(T)
        G = (G + G.T) / 2
        b = G.shape[0]
        d = np.diag(G).copy()
        if p == 0:
            if not (d > 0).all():
                raise NotSpd(f"iteration {it}: a column of the block has t'Mt <= 0")
            s = 1.0 / np.sqrt(d)
            G = G * s[:, None] * s[None, :]
        else:
            s = np.ones(b)
        # Cholesky G = R'R column by column; a dropped column leaves no row and no column
        keep, R = [], np.zeros((b, b))
        for j in range(b):
            col = np.zeros(len(keep))
            for a, i in enumerate(keep):
                col[a] = (G[i, j] - R[:a, i] @ col[:a]) / R[a, i]
            piv = G[j, j] - col @ col
            if p == 0:
                if piv < -DROP or piv != piv:
                    raise NotSpd(f"iteration {it}: the Gram matrix of the block is not positive definite")
                if piv < DROP:
                    dropped += 1
                    continue
            elif not piv > 0:
                raise NotSpd(f"iteration {it}: the Gram matrix of the block is not positive definite")
            R[:len(keep), j] = col
            R[len(keep), j] = np.sqrt(piv)
            keep.append(j)
        if not keep:
            return T[:, :0], dropped
        Rk = R[:len(keep)][:, keep]
        T = (T[:, keep] * s[keep][None, :]) @ np.linalg.inv(Rk)
    return T, dropped


def _square(V, MV, S, c):
    """S[:, :c] R^-1 with R'R = S[:, :c]' (V'MV) S[:, :c]: V S[:, :c] is M-orthonormal to the accuracy of V'MV."""
    W = V.T @ MV
    Sc = S[:, :c]
    R = np.linalg.cholesky(Sc.T @ ((W + W.T) / 2) @ Sc).T
    out = S.copy()
    out[:, :c] = Sc @ np.linalg.inv(R)
    return out


def eigs(Ad, Md, Kinv, X0, k, tol, max_basis=0, max_iter=MAX_ITER):
    """Ad, Md (None: I) dense symmetric; Kinv: the dense inverse the preconditioner applies (of A, or of a matrix
    nearby).  Returns (lam[k], Y[n, k], resid[k], info) as the library does."""
    n = Ad.shape[0]
    block = X0.shape[1]
    if max_basis == 0:
        max_basis = default_basis(n, k, block)
    assert k + 2 * block <= max_basis <= min(n, 128)
    mul_m = (lambda X: X) if Md is None else (lambda X: Md @ X)
    norm_a = np.abs(Ad).sum(axis=1).max()
    norm_m = 1.0 if Md is None else np.abs(Md).sum(axis=1).max()

    def eta_of(R, Y, th):
        return np.abs(R).max(axis=0) / ((norm_a + np.abs(th) * norm_m) * np.abs(Y).max(axis=0))

    info = dict(iterations=0, restarts=0, nconv=0, basis=0, dropped=0, solve_columns=0)
    T, dr = _orthonormalise(X0.copy(), np.zeros((n, 0)), np.zeros((n, 0)), mul_m, 0)
    info["dropped"] += dr
    assert T.shape[1] > 0, "the start block has no independent column"
    V, AV, MV = T, Ad @ T, mul_m(T)
    inner = tol
    while True:
        m = V.shape[1]
        G = V.T @ AV
        th, S = np.linalg.eigh((G + G.T) / 2)
        kk = min(k, m)
        Yk = V @ S[:, :kk]
        eta = eta_of(AV @ S[:, :kk] - (MV @ S[:, :kk]) * th[:kk], Yk, th[:kk])
        done = m >= k and (eta <= inner).all()
        if done or info["iterations"] >= max_iter:
            S = _square(V, MV, S, kk)
            Yk = V @ S[:, :kk]
            fresh = eta_of(Ad @ Yk - mul_m(Yk) * th[:kk], Yk, th[:kk])
            if not done or (fresh <= tol).all() or info["iterations"] >= max_iter:
                break
            inner *= 0.5   # the kept products flattered a pair: the loop asks for half from here on
            continue
        info["iterations"] += 1
        if m + block > max_basis:
            keep = min(m, k + block)
            V = V @ _square(V, MV, S, keep)[:, :keep]
            AV, MV = Ad @ V, mul_m(V)   # fresh products, not rotated ones
            S, m = np.eye(keep), keep
            info["restarts"] += 1
        src = [i for i in range(kk) if m < k or eta[i] > inner][:block]
        src += list(range(k, m))[:block - len(src)]
        R = AV @ S[:, src] - (MV @ S[:, src]) * th[src]
        info["solve_columns"] += len(src)
        T, dr = _orthonormalise(Kinv @ R, V, MV, mul_m, info["iterations"])
        info["dropped"] += dr
        if T.shape[1] == 0:
            Yk = V @ _square(V, MV, S, kk)[:, :kk]
            fresh = eta_of(Ad @ Yk - mul_m(Yk) * th[:kk], Yk, th[:kk])
            break
        V, AV, MV = np.hstack([V, T]), np.hstack([AV, Ad @ T]), np.hstack([MV, mul_m(T)])
    lam, Y, resid = np.full(k, np.nan), np.zeros((n, k)), np.full(k, np.inf)
    lam[:kk], Y[:, :kk], resid[:kk] = th[:kk], Yk, fresh
    info["nconv"] = int((resid <= tol).sum())
    info["basis"] = V.shape[1]
    return lam, Y, resid, info


# ---- the measures of both tiers -------------------------------------------------------------------------------------
def measures(Ad, Md, lam, Y):
    """In numpy.longdouble, of returned pairs: eta (the issue's normwise backward error), the rigorous eigenvalue bound
    ||r||_{M^-1} / ||y||_M per pair, and ||Y'MY - I||_max."""
    n = Ad.shape[0]
    Mx = np.eye(n) if Md is None else Md
    A, M, Yx, lx = ld(Ad), ld(Mx), ld(Y), ld(lam)
    R = A @ Yx - (M @ Yx) * lx
    norm_a, norm_m = np.abs(Ad).sum(axis=1).max(), np.abs(Mx).sum(axis=1).max()
    eta = np.abs(R).max(axis=0) / ((norm_a + np.abs(lx) * norm_m) * np.abs(Yx).max(axis=0))
    Minv = ld(np.linalg.inv(Mx))
    rn = np.sqrt(np.maximum(np.einsum("ij,ij->j", R, Minv @ R), 0))
    yn = np.sqrt(np.einsum("ij,ij->j", Yx, M @ Yx))
    orth = np.abs(Yx.T @ (M @ Yx) - np.eye(Y.shape[1])).max()
    return eta.astype(np.float64), (rn / yn).astype(np.float64), float(orth)


def reference_error(Ad, Md, lam):
    """n u ||M^-1||_2 (||A||_2 + |lambda| ||M||_2): the error of the reference spectrum itself."""
    n = Ad.shape[0]
    a2 = np.abs(np.linalg.eigvalsh(Ad)).max()
    if Md is None:
        return n * U * (a2 + np.abs(lam))
    ev = np.linalg.eigvalsh(Md)
    return n * U / ev.min() * (a2 + np.abs(lam) * ev.max())


def kappa_m(Md):
    if Md is None:
        return 1.0
    ev = np.linalg.eigvalsh(Md)
    return float(ev.max() / ev.min())
