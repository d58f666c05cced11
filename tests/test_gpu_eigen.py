"""LOBPCG on the device (poms_amd.eigen.lobpcg) against dense eigensolves and against a dense
NumPy restatement of the same algorithm: the same residual, the same [X W P] basis, the
same restart rule, a Jacobi preconditioner from diag(A).

Acceptance of an eigenvalue (Krylov-Weinstein): with rho(mu, y) = ||A y - mu B y||_{B^-1} /
||y||_B some exact eigenvalue lies within rho of mu, so
|lam_j - ex_j| <= rho(lam_j, x_j) + rho(ex_j, v_j) + n EPS ex_max, the last term for the dense
solver's own rounding.  Every k below ends at a spectral gap; sorted values are compared,
never the vectors of a near-degenerate pair."""
import functools

import numpy as np
import pytest
import scipy.linalg as sla

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


# ---- the dense restatement ---------------------------------------------------------------

def dense_rr(G, H, m):
    """poms_amd.eigen.rayleigh_ritz, restated: (theta, C, cond) or None where H is not
    numerically positive definite."""
    n = G.shape[0]
    h = np.diag(H)
    if not np.all(h > 0.0):
        return None
    d = 1.0 / np.sqrt(h)
    Gs, Hs = d[:, None] * G * d[None, :], d[:, None] * H * d[None, :]
    Gs, Hs = 0.5 * (Gs + Gs.T), 0.5 * (Hs + Hs.T)
    w = np.linalg.eigvalsh(Hs)
    if not w[0] > n * EPS * w[-1]:
        return None
    theta, Z = sla.eigh(Gs, Hs)
    return theta[:m], d[:, None] * Z[:, :m], w[-1] / w[0]


def dense_lobpcg(Ad, Bd, X0, prec, tol, maxiter, free=None):
    """(lam, X, niter, restarts, history) of LOBPCG on dense matrices from the columns of X0."""
    from poms_amd.eigen import RESTART_COND
    k = X0.shape[1]
    proj = (lambda Y: Y) if free is None else (lambda Y: Y * free[:, None])
    X = proj(X0.copy())
    AX, BX = Ad @ X, Bd @ X
    theta, C, cond = dense_rr(X.T @ AX, X.T @ BX, k)
    X, AX, BX = X @ C, AX @ C, BX @ C
    P = AP = BP = None
    history, niter, restarts = [theta], 0, 0
    nrm = lambda Y: np.sqrt(np.sum(Y * Y, axis=0))
    while True:
        R = AX - BX * theta
        res = nrm(R) / (nrm(AX) + np.abs(theta) * nrm(BX))
        if np.all(res <= tol) or niter >= maxiter:
            break
        W = proj(prec(R))
        AW, BW = Ad @ W, Bd @ W
        S, AS, BS = [X, W], [AX, AW], [BX, BW]
        if P is not None:
            S, AS, BS = S + [P], AS + [AP], BS + [BP]
        S, AS, BS = np.hstack(S), np.hstack(AS), np.hstack(BS)
        G, H = S.T @ AS, S.T @ BS
        out = dense_rr(G, H, k) if P is not None else None
        if out is None or out[2] > RESTART_COND:
            restarts += int(P is not None)
            theta, C2, cond = dense_rr(G[:2 * k, :2 * k], H[:2 * k, :2 * k], k)
            C = np.zeros((S.shape[1], k))
            C[:2 * k] = C2
        else:
            theta, C, cond = out
        Cp = C.copy()
        Cp[:k] = 0.0
        X, P, AX, AP, BX, BP = S @ C, S @ Cp, AS @ C, AS @ Cp, BS @ C, BS @ Cp
        niter += 1
        history.append(theta)
    return theta, X, niter, restarts, history


def rho(Ad, Bfac, Bd, mu, y):
    r = Ad @ y - mu * (Bd @ y)
    return np.sqrt(r @ sla.cho_solve(Bfac, r)) / np.sqrt(y @ (Bd @ y))


def accept_eigenvalues(lam, Xd, Ad, Bd, k):
    """The module docstring's acceptance, on the sorted values; returns the exact ones."""
    ex, Vx = sla.eigh(Ad, Bd)
    Bfac = sla.cho_factor(Bd)
    n = Ad.shape[0]
    assert np.all(np.diff(lam) >= 0.0)
    for j in range(k):
        bound = rho(Ad, Bfac, Bd, lam[j], Xd[:, j]) + rho(Ad, Bfac, Bd, ex[j], Vx[:, j]) + n * EPS * ex[-1]
        print(f"  lam[{j}] = {lam[j]:.15g}  exact {ex[j]:.15g}  |diff| {abs(lam[j] - ex[j]):.2e}  bound {bound:.2e}")
        assert abs(lam[j] - ex[j]) <= bound
    return ex


def columns(X):
    return np.stack([x.to_local_numpy().reshape(-1) for x in X], axis=1)


def kron_all(ms):
    return functools.reduce(np.kron, ms)


# ---- Kronecker operators, natural boundaries ----------------------------------------------

@functools.lru_cache(maxsize=None)
def kron_problem(p, cells):
    """-Δ + 1 and the mass operator on the unit square / cube, with their dense matrices."""
    from poms_amd.splines import assemble_1d, band_to_dense, uniform_knots
    from poms_amd.stencil import KronOperator, StencilVectorSpace
    nd = len(cells)
    T = [uniform_knots(p, N) for N in cells]
    MK = [assemble_1d(t, p) for t in T]
    M, K = [mk[0] for mk in MK], [mk[1] for mk in MK]
    V = StencilVectorSpace([N + p for N in cells], [p] * nd)
    A = KronOperator.laplace(V, M, K)
    B = KronOperator.product(V, M)
    Md, Kd = [band_to_dense(m) for m in M], [band_to_dense(k_) for k_ in K]
    Bd = kron_all(Md)
    Ad = Bd.copy()
    for d in range(nd):
        Ad = Ad + kron_all([Kd[e] if e == d else Md[e] for e in range(nd)])
    return V, A, B, Ad, Bd, T, M, K


def start_block(V, k, seed):
    Xn = np.random.default_rng(seed).standard_normal((k,) + tuple(V.npts))
    return [V.zeros().from_numpy(a) for a in Xn], Xn.reshape(k, -1).T.copy()


KRON_CASES = {"2d_p2_8x6": (2, (8, 6)), "2d_p3_8x6": (3, (8, 6)), "3d_p2_6x5x4": (2, (6, 5, 4))}


@pytest.mark.parametrize("case", list(KRON_CASES))
def test_kronecker_natural_boundaries(gpu, case):
    """The k = 4 lowest pairs of -Δ + 1 against eigh, with Jacobi, tol 1e-9.

    B-orthonormality: X = S C with C from eigh of the scaled H (condition kappa_H, reported as
    info["cond"]).  H as computed differs from S^T B S by at most N EPS |s_i|^T |B s_j| per
    entry (N unknowns: the dot) and as much again for the apply, and |s_i|^T |B s_j| <=
    kappa_B^1/2 ||s_i||_B ||s_j||_B (Cauchy-Schwarz in the 2-norm), i.e. 2 N EPS kappa_B^1/2
    per entry of the scaled H; eigh adds 3k EPS.  A perturbation delta of the scaled H moves
    C^T H C by at most ||delta|| / lambda_min <= ||delta|| kappa_H (lambda_max >= 1 at unit
    diagonal), and ||delta|| <= 3k max|delta_ij|: the bound 3k (2 N kappa_B^1/2 + 3k) EPS kappa_H."""
    from poms_amd import solvers
    from poms_amd.eigen import lobpcg
    p, cells = KRON_CASES[case]
    V, A, B, Ad, Bd, *_ = kron_problem(p, cells)
    k, tol, n = 4, 1e-9, Ad.shape[0]
    X0, X0d = start_block(V, k, 5)
    lam, X, info = lobpcg(A, B, k=k, X0=X0, precond=solvers.jacobi, tol=tol, maxiter=300)
    Xd = columns(X)
    print(f"{case}: niter {info['niter']} restarts {info['restarts']} cond {info['cond']:.2e} res {info['res']}")
    assert np.all(info["converged"]) and info["niter"] < 300
    assert len(info["history"]) == info["niter"] + 1
    # the residuals, recomputed from the downloaded X with the dense matrices
    AXd, BXd = Ad @ Xd, Bd @ Xd
    nrm = lambda Y: np.sqrt(np.sum(Y * Y, axis=0))
    res = nrm(AXd - BXd * lam) / (nrm(AXd) + np.abs(lam) * nrm(BXd))
    assert np.all(res <= tol * (1.0 + n * EPS) + n * EPS)
    # (the solver's own figures: each side forms r with an error of n EPS of the denominator)
    assert np.allclose(res, info["res"], rtol=1e-3, atol=2 * n * EPS)
    ex = accept_eigenvalues(lam, Xd, Ad, Bd, k)
    # history[0] is Rayleigh-Ritz on X0
    h0 = sla.eigh(X0d.T @ Ad @ X0d, X0d.T @ Bd @ X0d, eigvals_only=True)
    assert np.max(np.abs(info["history"][0] - h0)) <= k * n * EPS * ex[-1]
    # X is B-orthonormal
    kb = np.linalg.cond(Bd)
    orth = 3 * k * (2 * n * np.sqrt(kb) + 3 * k) * EPS * info["cond"]
    dev = np.max(np.abs(Xd.T @ Bd @ Xd - np.eye(k)))
    print(f"  |X^T B X - I| {dev:.2e}  bound {orth:.2e}")
    assert dev <= orth
    # the start block is the caller's: not modified
    assert np.array_equal(columns(X0), X0d)


def test_standard_problem(gpu):
    """B = None on the 2D p = 2 case against eigh(A_d); the default start block is the
    seeded standard_normal draw, one per vector in turn."""
    from poms_amd import solvers
    from poms_amd.eigen import lobpcg
    V, A, B, Ad, Bd, *_ = kron_problem(2, (8, 6))
    k, n = 4, Ad.shape[0]
    lam, X, info = lobpcg(A, None, k=k, precond=solvers.jacobi, tol=1e-9, maxiter=300, seed=3)
    print(f"standard: niter {info['niter']} restarts {info['restarts']} cond {info['cond']:.2e}")
    assert np.all(info["converged"]) and info["niter"] < 300
    Id = np.eye(n)
    ex = accept_eigenvalues(lam, columns(X), Ad, Id, k)
    rng = np.random.default_rng(3)
    X0d = np.stack([rng.standard_normal(n) for _ in range(k)], axis=1)
    h0 = sla.eigh(X0d.T @ Ad @ X0d, X0d.T @ X0d, eigvals_only=True)
    assert np.max(np.abs(info["history"][0] - h0)) <= k * n * EPS * ex[-1]


def test_dirichlet(gpu):
    """All four faces constrained, k = 3: against eigh of the free sub-blocks of the
    unconstrained dense matrices; X is exactly zero on the constrained rows."""
    from poms_amd import solvers
    from poms_amd.boundary import DirichletBC
    from poms_amd.eigen import lobpcg
    from poms_amd.splines import constrain_1d
    from poms_amd.stencil import KronOperator
    V, _, _, Ad, Bd, T, M, K = kron_problem(2, (8, 6))
    A = KronOperator.laplace(V, M, K, dirichlet="all")
    B = KronOperator.product(V, [constrain_1d(m, True, True) for m in M])
    bc = DirichletBC(V, T, "all")
    k = 3
    lam, X, info = lobpcg(A, B, k=k, precond=solvers.jacobi, project=bc.project, tol=1e-9, maxiter=300, seed=1)
    print(f"dirichlet: niter {info['niter']} restarts {info['restarts']} cond {info['cond']:.2e}")
    assert np.all(info["converged"]) and info["niter"] < 300
    free = np.ones(V.npts, dtype=bool)
    free[0, :] = free[-1, :] = free[:, 0] = free[:, -1] = False
    free = free.reshape(-1)
    Xd = columns(X)
    assert np.all(Xd[~free] == 0.0)
    accept_eigenvalues(lam, Xd[free], Ad[np.ix_(free, free)], Bd[np.ix_(free, free)], k)


# ---- a V-cycle as the preconditioner, variable coefficients ---------------------------------

def a_var(x, y, *z):
    return (1.0 + 0.5 * np.sin(3 * x) * np.cos(2 * y)) * (1.0 + z[0] / 4 if z else 1.0)


def c_var(x, y, *z):
    return 2.0 + x * y


@pytest.mark.parametrize("kind", ["galerkin", "matfree"])
def test_vcycle_preconditioner(gpu, kind):
    """-∇·(a∇u) + c u with a Chebyshev-smoothed V-cycle as the preconditioner: the eigenvalue
    acceptance, and no more iterations than the Jacobi-preconditioned dense restatement
    needs from the same start block."""
    from poms_amd.eigen import lobpcg
    from poms_amd.matfree import MatrixFreeVCycle
    from poms_amd.mg import GalerkinVCycle
    from poms_amd.splines import assemble_1d, band_to_dense, uniform_knots
    from poms_amd.stencil import KronOperator
    p, N, k, tol = 2, 16, 4, 1e-9
    cls = GalerkinVCycle if kind == "galerkin" else MatrixFreeVCycle
    vc = cls.uniform(p, N, 4, ndim=2, a=a_var, c=c_var, smoother="chebyshev")
    A, V = vc.A, vc.space
    M1 = assemble_1d(uniform_knots(p, N), p)[0]
    B = KronOperator.product(V, [M1] * 2)
    Ad = A.toarray() if kind == "galerkin" else A.assemble().toarray()
    Bd = kron_all([band_to_dense(M1)] * 2)
    X0, X0d = start_block(V, k, 9)
    lam, X, info = lobpcg(A, B, k=k, X0=X0, precond=vc.preconditioner(), tol=tol, maxiter=100)
    assert np.all(info["converged"])
    accept_eigenvalues(lam, columns(X), Ad, Bd, k)
    dinv = 1.0 / np.diag(Ad)
    ref = dense_lobpcg(Ad, Bd, X0d, lambda R: R * dinv[:, None], tol, 500)
    print(f"{kind}: niter {info['niter']} (V-cycle) against {ref[2]} (dense, Jacobi); restarts {info['restarts']}")
    assert ref[2] < 500
    assert np.max(np.abs(ref[0] - sla.eigh(Ad, Bd, eigvals_only=True)[:k])) <= 1e-9
    assert info["niter"] <= ref[2]


def test_device_iteration_follows_the_dense_restatement(gpu):
    """With the same preconditioner (Jacobi) the device iteration and the restatement take
    the same path up to rounding: the same first Ritz values and iteration counts that
    differ by a few at most."""
    from poms_amd import solvers
    from poms_amd.eigen import lobpcg
    V, A, B, Ad, Bd, *_ = kron_problem(2, (8, 6))
    k = 4
    X0, X0d = start_block(V, k, 5)
    lam, X, info = lobpcg(A, B, k=k, X0=X0, precond=solvers.jacobi, tol=1e-9, maxiter=300)
    dinv = 1.0 / np.diag(Ad)
    ref = dense_lobpcg(Ad, Bd, X0d, lambda R: R * dinv[:, None], 1e-9, 300)
    print(f"device niter {info['niter']} restarts {info['restarts']}; dense niter {ref[2]} restarts {ref[3]}")
    for it in range(3):
        assert np.allclose(info["history"][it], ref[4][it], rtol=1e-10, atol=0.0)
    assert abs(info["niter"] - ref[2]) <= max(3, ref[2] // 10)


def test_determinism(gpu):
    import torch
    from poms_amd import solvers
    from poms_amd.eigen import lobpcg
    V, A, B, *_ = kron_problem(2, (8, 6))
    X0, _ = start_block(V, 4, 5)
    runs = [lobpcg(A, B, k=4, X0=X0, precond=solvers.jacobi, tol=1e-9, maxiter=300) for _ in range(2)]
    assert np.array_equal(runs[0][0], runs[1][0])
    assert runs[0][2]["niter"] == runs[1][2]["niter"]
    for xa, xb in zip(runs[0][1], runs[1][1]):
        assert torch.equal(xa._store, xb._store)


def test_refusals(gpu):
    import types
    from poms_amd.dist import CartDistribution, SlabDistribution
    from poms_amd.eigen import block_gram, lobpcg
    from poms_amd.stencil import StencilVectorSpace
    V, A, B, *_ = kron_problem(2, (8, 6))
    V2, A2, B2, *_ = kron_problem(3, (8, 6))
    with pytest.raises(ValueError, match="same"):
        lobpcg(A, B2, k=2)
    with pytest.raises(ValueError, match="X0"):
        lobpcg(A, B, k=2, X0=[V.zeros()])
    with pytest.raises(ValueError, match="k"):
        lobpcg(A, B, k=9)
    # a slab and a Cart block are refused by their space alone (an operator's stand-in: the
    # refusal comes before the operator is used)
    for dist, npts in ((SlabDistribution(8, 0, 2), (8, 8, 8)), (CartDistribution((8, 8), (2, 1), 0), (8, 8))):
        Vs = StencilVectorSpace(list(npts), [2] * len(npts), dist=dist)
        As = types.SimpleNamespace(space=Vs, dot=None)
        with pytest.raises(NotImplementedError, match="distributed"):
            lobpcg(As, None, k=2)
        with pytest.raises(NotImplementedError, match="distributed"):
            block_gram([Vs.zeros()], [Vs.zeros()])
