"""Dirichlet boundary conditions on the device: the kernels' masks bit for bit against the
unconstrained operator, the dense contract ``Π A Π + (I − Π) D (I − Π)``, the constrained
Kronecker form against the oracle, the invariance of the constrained entries under the
solvers and the V-cycles, the constrained hierarchy, cycle parity on the free unknowns
against a CPU restatement on the reduced system, solved problems with lifted data, and
the refusals.

Spaces: 8 x 9 functions (axis 1 is one matrix-free tile of 8 columns, so its ``hi`` face
is the tile's last column; axis 2 a tile plus one, its ``hi`` face alone in a second
tile); 33 x 8 x 4 (two axis-0 chunks of 17 + 16 planes, and n = 4 <= 2p on the last axis:
every row within p of both faces); and the two shapes of test_gpu_matfree.py's
test_epilogues."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import splu

from oracle import poms_oracle as orc

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


def rel(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def maxrel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def a_var(x, y, *z):
    return (1.0 + 0.5 * np.sin(3 * x) * np.cos(2 * y)) * (1.0 + z[0] / 4 if z else 1.0)


def c_var(x, y, *z):
    return 2.0 + x * y


def a_jump(x, y):
    return np.where((x > 0.5) & (y > 0.5), 100.0, 1.0)


def face_sets(nd):
    no = (False, False)
    mixed = [(True, False), (True, True)] + [no] * (nd - 2)
    return {"all": "all", "lo0": [(True, False)] + [no] * (nd - 1), "hi_last": [no] * (nd - 1) + [(False, True)],
            "mixed": mixed}


def sheared(d):
    """F = (x + 0.3 y, y(, z)): a constant Jacobian with an off-diagonal entry."""
    from poms_amd.geometry import Mapping
    F = lambda *X: [X[0] + 0.3 * X[1]] + list(X[1:])
    jac = lambda *X: [[1.0 if i == k else (0.3 if (i, k) == (0, 1) else 0.0) for k in range(d)] for i in range(d)]
    return Mapping(F, jac, ndim=d)


SPACES = {
    "2d_p33_5x6": ((3, 3), (5, 6), False),
    "3d_p213_31x7x1": ((2, 1, 3), (31, 7, 1), False),
    "2d_p33_8x7_aligned": ((3, 3), (8, 7), True),
    "3d_p321_3x4x5": ((3, 2, 1), (3, 4, 5), False),
}


def build(form, degrees, cells, align, dirichlet=None, V=None):
    from poms_amd.assembly import assemble_stencil
    from poms_amd.geometry import MappedDomain
    from poms_amd.matfree import MatrixFreeOperator
    from poms_amd.splines import make_open_knots
    from poms_amd.stencil import StencilVectorSpace
    T = [make_open_knots(p, N + p) for p, N in zip(degrees, cells)]
    if V is None:
        V = StencilVectorSpace([N + p for p, N in zip(degrees, cells)], list(degrees), align=align)
    if form == "stencil":
        A = assemble_stencil(V, T, a=a_var, c=c_var, dirichlet=dirichlet)
    elif form == "matfree":
        A = MatrixFreeOperator(V, T, a=a_var, c=c_var, dirichlet=dirichlet)
    else:
        A = MappedDomain(V, T, sheared(V.ndim)).operator(a=a_var, c=c_var, matrix_free=True, dirichlet=dirichlet)
        assert A.tensor
    return A, V, T


def diag_of(A, V):
    if A.form == "matfree":
        return A.diagonal().cpu().numpy()
    return A._data[tuple(slice(p, p + n) for p, n in zip(V.pads, V.npts)) + tuple(V.pads)].copy()


def run_all(A, V, x, b, om):
    """dot, residual, the sweep (x_out, norm, dot) and dot_inner (vector, scalar)."""
    y = A.dot(x).to_local_numpy()
    r = A.residual(b, x).to_local_numpy()
    xo = V.empty()
    nrm, dt = A.jacobi_sweep(b, x, xo, om, want_norm=True, want_dot=True)
    q = V.empty()
    pq = A.dot_inner(x, q)
    return dict(y=y, r=r, xo=xo.to_local_numpy(), nrm=nrm, dt=dt, q=q.to_local_numpy(), pq=pq)


@pytest.mark.parametrize("form", ["stencil", "matfree", "tensor"])
@pytest.mark.parametrize("space", list(SPACES))
def test_masks_bitwise(gpu, form, space):
    from poms_amd.boundary import constrained_mask, normalize_faces
    degrees, cells, align = SPACES[space]
    A, V, _ = build(form, degrees, cells, align)
    B, _, _ = build(form, degrees, cells, align, V=V)   # never has a mask
    assert A.dirichlet is None
    rng = np.random.default_rng(7)
    xn, bn = rng.uniform(-1, 1, V.npts), rng.uniform(-1, 1, V.npts)
    x, b = V.zeros().from_numpy(xn), V.zeros().from_numpy(bn)
    D = diag_of(A, V)
    om = 2.0 / 3.0
    never = run_all(B, V, x, b, om)
    for name, faces in face_sets(V.ndim).items():
        C = constrained_mask(V.npts, faces)
        F = ~C
        assert C.any() and F.any()
        A.set_dirichlet(faces)
        assert A.dirichlet == normalize_faces(faces, V.ndim)
        got = run_all(A, V, x, b, om)
        A.set_dirichlet(None)
        assert A.dirichlet is None
        xp = V.zeros().from_numpy(np.where(C, 0.0, xn))
        ref = run_all(A, V, xp, b, om)
        # free rows: the unconstrained operator applied to Πx, bit for bit
        for k in ("y", "r", "xo", "q"):
            assert np.array_equal(got[k][F], ref[k][F]), (name, k)
        # constrained rows: the diagonal entry
        dx = D * xn
        assert np.array_equal(got["y"][C], dx[C]) and np.array_equal(got["q"][C], dx[C]), name
        bound = 4 * EPS * (np.abs(bn) + np.abs(dx))
        er, ex = np.abs(got["r"] - (bn - dx)), np.abs(got["xo"] - (xn + om * (bn - dx) / D))
        print(f"{space} {form} {name}: worst error / bound on C: residual {np.max(er[C] / bound[C]):.3f}, "
              f"sweep {np.max(ex[C] / bound[C]):.3f}; min diag {D.min():.3e}")
        assert np.all(er[C] <= bound[C]) and np.all(ex[C] <= bound[C]), name
        # the sums run over all rows
        dr = om * (bn - got["y"]) / D
        assert abs(got["nrm"] - np.sum(dr * dr)) <= 1e-13 * np.sum(dr * dr), name
        assert abs(got["dt"] - np.sum(got["xo"] * bn)) <= 1e-13 * np.sum(np.abs(got["xo"] * bn)), name
        assert abs(got["pq"] - np.sum(xn * got["y"])) <= 1e-13 * np.sum(np.abs(xn * got["y"])), name
        # set and cleared again: an operator that never had a mask
        again = run_all(A, V, x, b, om)
        for k, v in never.items():
            assert np.array_equal(again[k], v), (name, k)


@pytest.mark.parametrize("space", ["2d_p33_5x6", "3d_p321_3x4x5"])
def test_dense_contract(gpu, space):
    from poms_amd.boundary import constrained_mask
    degrees, cells, align = SPACES[space]
    A, V, _ = build("stencil", degrees, cells, align)
    Am, _, _ = build("matfree", degrees, cells, align, V=V)
    A0 = A.toarray()
    data0 = A._data.copy()
    xn = np.random.default_rng(3).uniform(-1, 1, V.npts)
    x = V.zeros().from_numpy(xn)
    for name, faces in face_sets(V.ndim).items():
        c = constrained_mask(V.npts, faces).reshape(-1)
        pi = np.diag((~c).astype(float))
        want = pi @ A0 @ pi + (np.eye(len(c)) - pi) @ np.diag(np.diag(A0)) @ (np.eye(len(c)) - pi)
        A.set_dirichlet(faces)
        AD = A.toarray()
        assert np.array_equal(AD, want), name
        assert np.array_equal(A.tocsr().toarray(), want) and np.array_equal(A.tosparse().toarray(), want)
        assert np.array_equal(A._data, data0)   # the stored coefficients are those of A
        assert maxrel(A.dot(x).to_local_numpy().reshape(-1), want @ xn.reshape(-1)) <= 1e-13, name
        Am.set_dirichlet(faces)
        assert maxrel(Am.dot(x).to_local_numpy().reshape(-1), want @ xn.reshape(-1)) <= 1e-13, name
        As = Am.assemble()
        assert As.dirichlet == Am.dirichlet
        A.set_dirichlet(None)
        Am.set_dirichlet(None)
    assert np.array_equal(A.toarray(), A0)


@pytest.mark.parametrize("ndim,p", [(2, 3), (3, 2)])
def test_kronecker_form(gpu, ndim, p):
    from poms_amd.boundary import constrained_mask, normalize_faces
    from poms_amd.splines import assemble_1d, band_to_dense, constrain_1d, dense_to_band, uniform_knots
    from poms_amd.stencil import KronOperator, StencilVectorSpace
    N = 16
    n = N + p
    M, K = assemble_1d(uniform_knots(p, N), p)
    V = StencilVectorSpace([n] * ndim, [p] * ndim)
    rng = np.random.default_rng(ndim)
    xn, bn = rng.uniform(-1, 1, V.npts), rng.uniform(-1, 1, V.npts)
    x, b = V.zeros().from_numpy(xn), V.zeros().from_numpy(bn)
    om = 2.0 / 3.0
    for name, faces in face_sets(ndim).items():
        f = normalize_faces(faces, ndim)
        A = KronOperator.laplace(V, [M] * ndim, [K] * ndim, dirichlet=faces)
        assert A.dirichlet == f
        Mt = [constrain_1d(M, lo, hi) for lo, hi in f]
        Kt = [constrain_1d(K, lo, hi) for lo, hi in f]
        y_ref = orc.kron_sum_apply(xn, Mt, Kt)
        Dg = orc.kron_sum_diag(Mt, Kt)
        y = A.dot(x).to_local_numpy()
        assert rel(y, y_ref) <= 1e-13 and np.max(np.abs(y - y_ref)) <= 1e-12 * np.max(np.abs(y_ref)), name
        r = A.residual(b, x).to_local_numpy()
        assert rel(r, bn - y_ref) <= 1e-13, name
        xo = V.empty()
        nrm = A.jacobi_sweep(b, x, xo, om, want_norm=True)
        dr = om * (bn - y_ref) / Dg
        assert rel(xo.to_local_numpy(), xn + dr) <= 1e-13, name
        assert abs(nrm - float(np.vdot(dr, dr))) <= 1e-12 * float(np.vdot(dr, dr)), name
        # the free rows are the reduced operator's: constrained rows and columns dropped
        sl = tuple(slice(1 if lo else 0, n - 1 if hi else n) for lo, hi in f)
        red = lambda F, s: dense_to_band(band_to_dense(F)[s, s], p)
        Mr, Kr = [red(M, s) for s in sl], [red(K, s) for s in sl]
        F = ~constrained_mask(V.npts, faces)
        yr = orc.kron_sum_apply(xn[sl], Mr, Kr)
        assert rel(y[F], yr.reshape(-1)) <= 1e-13, name
        assert rel(r[F], (bn[sl] - yr).reshape(-1)) <= 1e-13, name
        drr = om * (bn[sl] - yr) / orc.kron_sum_diag(Mr, Kr)
        assert rel(xo.to_local_numpy()[F], (xn[sl] + drr).reshape(-1)) <= 1e-13, name


def _projected_rhs(V, faces, seed=0):
    from poms_amd.boundary import constrained_mask
    C = constrained_mask(V.npts, faces)
    bn = np.where(C, 0.0, np.random.default_rng(seed).uniform(-1, 1, V.npts))
    return V.zeros().from_numpy(bn), C


@pytest.mark.parametrize("form", ["stencil", "matfree", "tensor", "kron"])
def test_constrained_entries_stay_zero_under_pcg(gpu, form):
    from poms_amd.solvers import damped_jacobi, pcg
    for space in ("2d_p33_5x6", "3d_p213_31x7x1"):
        degrees, cells, align = SPACES[space]
        nd = len(degrees)
        for name, faces in face_sets(nd).items():
            if form == "kron":
                from poms_amd.splines import assemble_1d, make_open_knots
                from poms_amd.stencil import KronOperator, StencilVectorSpace
                V = StencilVectorSpace([N + p for p, N in zip(degrees, cells)], list(degrees))
                MK = [assemble_1d(make_open_knots(p, N + p), p) for p, N in zip(degrees, cells)]
                A = KronOperator.laplace(V, [m for m, _ in MK], [k for _, k in MK], dirichlet=faces)
            else:
                A, V, _ = build(form, degrees, cells, align, dirichlet=faces)
            b, C = _projected_rhs(V, faces)
            x, info = pcg(A, damped_jacobi, b, tol=0.0, maxiter=10)
            xn = x.to_local_numpy()
            assert info["niter"] == 10 and np.all(np.isfinite(xn)) and np.any(xn[~C] != 0.0)
            assert np.all(xn[C] == 0.0), (space, name)


def test_constrained_entries_stay_zero_under_the_cycles(gpu):
    from poms_amd.boundary import DirichletBC
    from poms_amd.matfree import MatrixFreeVCycle
    from poms_amd.mg import GalerkinVCycle, MultilevelVCycle, TwoLevelVCycle
    mixed3 = [(True, False), (True, True), (False, False)]
    cycles = [(GalerkinVCycle.uniform(2, 16, 4, 2, a=a_jump, dirichlet="all"), "all"),
              (MatrixFreeVCycle.uniform(2, 8, 2, 3, dirichlet=mixed3), mixed3),
              (TwoLevelVCycle(3, 16, 4, ndim=2, dirichlet="all"), "all"),
              # 3D: the fused residual -> restriction runs on the constrained factors, on two levels
              (MultilevelVCycle(2, 16, 4, ndim=3, dirichlet="all"), "all")]
    assert cycles[3][0].nlevels == 3 and all(cycles[3][0].fused)
    for mg, faces in cycles:
        V = mg.space
        bc = DirichletBC(V, [mg.knots[0] if hasattr(mg, "knots") else mg.T] * V.ndim, faces)
        C = bc.mask().cpu().numpy()
        b = bc.project(mg.rhs_ones())
        assert np.all(b.to_local_numpy()[C] == 0.0) and np.all(b.to_local_numpy()[~C] == 1.0)
        x = mg.cycle(b)[0].to_local_numpy()
        assert np.all(np.isfinite(x)) and np.any(x[~C] != 0.0)
        assert np.all(x[C] == 0.0), type(mg).__name__


def kron_dense(Ps):
    return functools.reduce(np.kron, Ps)


def test_constrained_hierarchy(gpu):
    from poms_amd.boundary import constrain_dense, constrained_mask
    from poms_amd.mg import GalerkinVCycle
    mg = GalerkinVCycle.uniform(2, 32, 4, 2, a=a_jump, dirichlet="all")
    assert mg.nlevels == 4 and mg.dirichlet == ((True, True),) * 2
    rng = np.random.default_rng(1)
    for l in range(mg.nlevels - 1):
        A, Ac = mg.ops[l], mg.ops[l + 1]
        assert A.dirichlet == Ac.dirichlet == mg.dirichlet
        A.set_dirichlet(None)
        A0 = A.toarray()
        A.set_dirichlet(mg.dirichlet)
        P = kron_dense(mg.P[l])
        want = constrain_dense(P.T @ A0 @ P, Ac.space.npts, "all")
        assert maxrel(Ac.toarray(), want) <= 1e-13, l
        V = mg.spaces[l]
        rc = mg.transfers[l].restrict(V.zeros().from_numpy(rng.uniform(-1, 1, V.npts))).cpu().numpy()
        Cc = constrained_mask(Ac.space.npts, "all").reshape(-1)
        assert np.all(rc[Cc] == 0.0) and np.any(rc[~Cc] != 0.0), l
    assert np.array_equal(mg.Ac, mg.ops[-1].toarray())


def cpu_galerkin_cycle(A0, Ps, b, maxiters, tol, reorder=False, x0=None):
    """tests/test_gpu_galerkin.py's restatement of the recursive cycle of
    `sources/mg_jac.py:84-119` with scipy's Galerkin operators on every level:
    (P^T A) P from CSR storage, or with ``reorder`` P^T (A P) from CSC storage."""
    fmt = "csc" if reorder else "csr"
    As = [A0.asformat(fmt)]
    for P in Ps:
        A = As[-1]
        As.append((P.T @ (A @ P) if reorder else (P.T @ A) @ P).asformat(fmt))
    L = len(Ps) + 1
    infos = [None] * (L - 1)

    def cycle(l, bl, x0):
        A = As[l]
        if l == L - 1:
            return splu(A.tocsc()).solve(bl)
        D = A.diagonal().copy()
        apply = lambda v: A @ v
        psolve = lambda r: orc.damped_jacobi(apply, D, r)
        x, ipre = orc.pcg(apply, psolve, bl, x0=x0, tol=tol, maxiter=maxiters[l])
        ec = cycle(l + 1, Ps[l].T @ (bl - apply(x)), None)
        x = x + Ps[l] @ ec
        x, ipos = orc.pcg(apply, psolve, bl, x0=x, tol=tol, maxiter=maxiters[l])
        if infos[l] is None:
            infos[l] = (ipre, ipos)
        return x

    return cycle(0, b, x0), infos


def reduced_system(mg):
    """(A0_ff, [P_ff], free) of a GalerkinVCycle with all faces constrained."""
    from poms_amd.boundary import constrained_mask
    A = mg.ops[0]
    if A.form == "matfree":
        A = A.assemble()
    A.set_dirichlet(None)
    A0 = sp.csr_matrix(A.tosparse())
    A.set_dirichlet(mg.dirichlet)
    free = [~constrained_mask(V.npts, mg.dirichlet).reshape(-1) for V in mg.spaces]
    Ps = []
    for l, Pl in enumerate(mg.P):
        P = functools.reduce(lambda a, b: sp.kron(a, b, format="csr"), [sp.csr_matrix(p) for p in Pl])
        Ps.append(sp.csr_matrix(P)[free[l]][:, free[l + 1]])
    return A0[free[0]][:, free[0]], Ps, free[0]


@pytest.mark.parametrize("ndim,p,nf,nc,a", [(2, 2, 32, 4, a_jump),
                                            (3, 2, 8, 2, lambda x, y, z: 1.0 + x + 0.5 * y * z)])
def test_galerkin_cycle_parity_on_the_free_unknowns(gpu, ndim, p, nf, nc, a):
    from poms_amd.boundary import DirichletBC
    from poms_amd.mg import GalerkinVCycle
    mg = GalerkinVCycle.uniform(p, nf, nc, ndim, a=a, tol=0.0, dirichlet="all")
    mg.maxiters = [2] * (mg.nlevels - 1)
    assert mg.nlevels == {32: 4, 8: 3}[nf]
    b = DirichletBC(mg.space, [mg.knots[0]] * ndim, "all").project(mg.rhs_ones())
    x, infos = mg.cycle(b)
    Aff, Ps, free = reduced_system(mg)
    bf = np.ones(int(free.sum()))
    xr, rinfos = cpu_galerkin_cycle(Aff, Ps, bf, mg.maxiters, 0.0)
    xr2, _ = cpu_galerkin_cycle(Aff, Ps, bf, mg.maxiters, 0.0, reorder=True)
    tol = max(1e-9, 20.0 * rel(xr2, xr))
    for l in range(mg.nlevels - 1):
        assert infos[l][0]["niter"] == rinfos[l][0]["niter"] and infos[l][1]["niter"] == rinfos[l][1]["niter"], l
    xd = x.toarray()
    err = rel(xd[free], xr)
    print(f"constrained V-cycle parity {ndim}D: rel {err:.3e}, bound {tol:.3e}")
    assert err <= tol and np.all(xd[~free] == 0.0)


def test_two_level_cycle_parity_on_the_free_unknowns(gpu):
    from poms_amd.boundary import DirichletBC
    from poms_amd.mg import TwoLevelVCycle
    from poms_amd.splines import band_to_dense, dense_to_band
    p, nd = 3, 2
    mg = TwoLevelVCycle(p, 32, 8, ndim=nd, dirichlet="all", tol=0.0)
    b = DirichletBC(mg.space, [mg.T] * nd, "all").project(mg.rhs_ones())
    x, ipre, ipos = mg.cycle(b)
    red = lambda F: dense_to_band(band_to_dense(F)[1:-1, 1:-1], p)
    Ms, Ks = [red(mg.M1d)] * nd, [red(mg.K1d)] * nd
    Pr = mg.P1[1:-1, 1:-1]
    ones = np.ones((mg.n - 2,) * nd)
    xr, rpre, rpos = orc.vcycle_two_level(Ms, Ks, Pr, ones, tol=0.0)
    xr2, _, _ = orc.vcycle_two_level(Ms, Ks, Pr, ones, tol=0.0, reorder=True)
    tol = max(1e-9, 20.0 * rel(xr2, xr))
    assert ipre["niter"] == rpre["niter"] and ipos["niter"] == rpos["niter"]
    xd = x.to_local_numpy()
    err = rel(xd[1:-1, 1:-1], xr)
    print(f"constrained two-level parity: rel {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    inner = np.zeros_like(xd, dtype=bool)
    inner[1:-1, 1:-1] = True
    assert np.all(xd[~inner] == 0.0)


# ---- solved problems ------------------------------------------------------------------------
# CPU values (a dense NumPy restatement: Greville lift, the reduced system, p+1 Gauss points
# for the load vector and the error): cycles of the restated Galerkin cycle (tol = 0, four
# pcg iterations per smoothing, coarsest level 4 cells) to ||r|| <= 1e-10 ||b||, at N = 8 and
# N = 16.  The issue's table (p+2 points, direct solve) gives err(16); the test allows twice
# that.
CPU_CYCLES = {(1, "a"): (1, 1), (1, "b"): (2, 3), (2, "a"): (2, 2), (2, "b"): (2, 2), (3, "a"): (4, 5),
              (3, "b"): (4, 4)}
CPU_ERR16 = {(1, "a"): 1.84e-3, (1, "b"): 3.16e-4, (2, "a"): 3.11e-5, (2, "b"): 2.51e-6, (3, "a"): 9.72e-7,
             (3, "b"): 4.24e-8}


def _exact(case, lib):
    """(u, f) of -Δu + u = f with the functions of ``lib`` (numpy or torch)."""
    if case == "a":
        u = lambda x, y: lib.sin(np.pi * x) * lib.sin(np.pi * y)
        return u, lambda x, y: (2 * np.pi ** 2 + 1) * u(x, y)
    u = lambda x, y: lib.exp(x) * lib.cos(y)
    return u, u


@pytest.mark.parametrize("matrix_free", [False, True])
@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("p", [1, 2, 3])
def test_solved_problem_on_the_unit_square(gpu, p, case, matrix_free):
    """-Δu + u = f, all faces constrained: (a) u = sin πx sin πy, homogeneous data, (b)
    u = e^x cos y lifted with DirichletBC.lift.  Cycles (tol = 0, four iterations per
    smoothing) until ||r|| <= 1e-10 ||b||, at most twice the CPU restatement's count
    (CPU_CYCLES: 1-5 cycles); err(8) / err(16) >= 0.9 2^(p+1) and err(16) at most twice
    the CPU value."""
    import torch

    from poms_amd.boundary import DirichletBC
    from poms_amd.field import assemble_rhs, l2_error
    from poms_amd.matfree import MatrixFreeVCycle
    from poms_amd.mg import GalerkinVCycle
    u_np, _ = _exact(case, np)
    u_t, f_t = _exact(case, torch)
    errs = {}
    for N, cpu in zip((8, 16), CPU_CYCLES[p, case]):
        cls = MatrixFreeVCycle if matrix_free else GalerkinVCycle
        nl = 2 if N == 8 else 3
        mg = cls.uniform(p, N, 4, 2, tol=0.0, maxiters=[4] * (nl - 1), dirichlet="all")
        assert mg.nlevels == nl
        V, T = mg.space, [mg.knots[0]] * 2
        bc = DirichletBC(V, T, "all")
        xg = bc.lift(u_np)
        b = bc.homogenize(mg.A, assemble_rhs(V, T, f_t), xg)
        assert mg.A.dirichlet == ((True, True),) * 2   # homogenize put the mask back
        if case == "a":
            assert np.max(np.abs(xg.to_local_numpy())) <= 1e-15
        nb = np.sqrt(b.dot(b))
        x, k = None, 0
        while k < 2 * cpu:
            x, _ = mg.cycle(b, x0=x)
            k += 1
            r = mg.A.residual(b, x)
            if np.sqrt(r.dot(r)) <= 1e-10 * nb:
                break
        res = np.sqrt(r.dot(r)) / nb
        errs[N] = l2_error(V, T, xg + x, u_t)
        print(f"p={p} case {case} N={N} {'matrix-free' if matrix_free else 'stored'}: {k} cycles (CPU {cpu}), "
              f"||r||/||b|| {res:.2e}, L2 error {errs[N]:.3e}")
        assert res <= 1e-10, (N, k)
    print(f"   err(8)/err(16) = {errs[8] / errs[16]:.2f}, err(16) / CPU value = {errs[16] / CPU_ERR16[p, case]:.3f}")
    assert errs[8] / errs[16] >= 0.9 * 2 ** (p + 1)
    assert errs[16] <= 2.0 * CPU_ERR16[p, case]


def quarter_annulus():
    """(s, t) -> (r cos θ, r sin θ), r = 1 + s, θ = π t / 2."""
    from poms_amd.geometry import Mapping
    h = np.pi / 2
    F = lambda s, t: [(1 + s) * np.cos(h * t), (1 + s) * np.sin(h * t)]
    jac = lambda s, t: [[np.cos(h * t), -h * (1 + s) * np.sin(h * t)], [np.sin(h * t), h * (1 + s) * np.cos(h * t)]]
    return Mapping(F, jac, ndim=2)


@pytest.mark.parametrize("matrix_free", [False, True])
def test_solved_problem_on_a_quarter_annulus(gpu, matrix_free):
    """-Δu + u = f on the quarter annulus 1 <= r <= 2, u = g = x^2 - y^2 (harmonic, f = u)
    on the whole boundary, p = 2: pcg to ||r|| <= 1e-10 ||b||, err(8) / err(16) >= 0.9 2^3."""
    from poms_amd.geometry import MappedDomain
    from poms_amd.solvers import damped_jacobi, pcg
    from poms_amd.splines import uniform_knots
    from poms_amd.stencil import StencilVectorSpace
    p = 2
    u = lambda x, y: x * x - y * y
    errs = {}
    for N in (8, 16):
        T = [uniform_knots(p, N)] * 2
        V = StencilVectorSpace([N + p] * 2, [p] * 2, align=True)
        dom = MappedDomain(V, T, quarter_annulus())
        A = dom.operator(matrix_free=matrix_free, dirichlet="all")
        bc = dom.dirichlet("all")
        xg = bc.lift(u)
        b = bc.homogenize(A, dom.load_vector(u), xg)
        nb = np.sqrt(b.dot(b))
        x, info = pcg(A, damped_jacobi, b, tol=1e-20 * nb, maxiter=500)
        assert info["success"], info
        C = bc.mask().cpu().numpy()
        assert np.all(x.to_local_numpy()[C] == 0.0)
        errs[N] = dom.l2_error(xg + x, u)
        print(f"quarter annulus p=2 N={N} {'matrix-free' if matrix_free else 'stored'}: {info['niter']} iterations, "
              f"L2 error {errs[N]:.4e}")
    print(f"   err(8)/err(16) = {errs[8] / errs[16]:.2f}")
    assert errs[8] / errs[16] >= 0.9 * 2 ** (p + 1)


def test_refusals(gpu):
    import ctypes as C

    from poms_amd import _lib
    from poms_amd.assembly import assemble_stencil
    from poms_amd.matfree import MatrixFreeOperator
    from poms_amd.mg import GalerkinVCycle, MultilevelVCycle, TwoLevelVCycle, two_level_setup_1d
    from poms_amd.splines import assemble_1d, uniform_knots
    from poms_amd.stencil import KronOperator, StencilVectorSpace
    p, N = 2, 8
    T = uniform_knots(p, N)
    V = StencilVectorSpace([N + p] * 2, [p] * 2)
    A = assemble_stencil(V, [T, T])
    for bad in ([(True, True)], "every", [(True, True), True], [(True, True)] * 3):
        with pytest.raises(ValueError, match="dirichlet"):
            A.set_dirichlet(bad)
        with pytest.raises(ValueError, match="dirichlet"):
            MatrixFreeOperator(V, [T, T], dirichlet=bad)
    assert A.dirichlet is None
    # a Kronecker handle is constrained through its factors
    M, K = assemble_1d(T, p)
    Ak = KronOperator.laplace(V, [M, M], [K, K])
    assert _lib.lib.poms_op_set_dirichlet(Ak._h, 1) != 0
    msg = _lib.lib.poms_last_error()
    assert b"poms_op_set_dirichlet" in msg and b"factors" in msg
    with pytest.raises(NotImplementedError, match="factors"):
        Ak.set_dirichlet("all")
    # bits beyond 2 ndim
    assert _lib.lib.poms_op_set_dirichlet(A._h, 1 << 4) != 0
    assert b"poms_op_set_dirichlet" in _lib.lib.poms_last_error()
    out = C.c_int(-1)
    _lib.call("poms_op_set_dirichlet", A._h, 9)
    _lib.call("poms_op_get_dirichlet", A._h, C.byref(out))
    assert out.value == 9
    _lib.call("poms_op_set_dirichlet", A._h, 0)
    # a P whose boundary row is not the unit vector
    P1 = two_level_setup_1d(p, T, uniform_knots(p, N // 2))[2]
    bad = P1.copy()
    bad[0, 1] = 0.5
    A.set_dirichlet("all")
    with pytest.raises(ValueError, match="unit vector"):
        GalerkinVCycle(A, [[P1, bad]])
    GalerkinVCycle(A, [[P1, P1]])
    # Kronecker cycles: no GLT post-smoother, no distribution
    with pytest.raises(NotImplementedError, match="GLT"):
        TwoLevelVCycle(p, N, 4, ndim=2, dirichlet="all", post_smoother="glt")
    with pytest.raises(NotImplementedError, match="distributed"):
        TwoLevelVCycle(p, N, 4, ndim=3, dirichlet="all", dist=object())
    with pytest.raises(NotImplementedError, match="distributed"):
        MultilevelVCycle(p, N, 4, ndim=3, dirichlet="all", dist=object())
    with pytest.raises(ValueError, match="dirichlet"):
        TwoLevelVCycle(p, N, 4, ndim=2, dirichlet="some")


def test_a_mask_on_a_slab_is_refused(gpu):
    """A 3D general-stencil handle that owns planes [2, 6) of 8: the C entry point refuses
    the mask (the Python classes refuse a distributed space before they get there)."""
    import ctypes as C

    from poms_amd import _lib
    from poms_amd.stencil import StencilVectorSpace
    V = StencilVectorSpace([4, 5, 6], [1, 1, 1])
    lay = _lib.Layout.make((4, 5, 6), (1, 1, 1))
    data = np.zeros((6, 7, 8, 3, 3, 3))
    h = C.c_void_p()
    _lib.call("poms_op_create_stencil", V.ctx, 3, C.byref(lay), data.ctypes.data_as(C.c_void_p), 2, 8, C.byref(h))
    try:
        assert _lib.lib.poms_op_set_dirichlet(h, 1) != 0
        msg = _lib.lib.poms_last_error()
        assert b"poms_op_set_dirichlet" in msg and b"slab" in msg
    finally:
        _lib.lib.poms_op_destroy(h)


def test_a_mask_on_a_distributed_space_is_refused(gpu):
    """A slab and a Cart space (one rank's share of each, built in this process): every entry
    point that takes faces raises NotImplementedError before it assembles or launches; no
    faces at all stay allowed."""
    from poms_amd.assembly import assemble_stencil
    from poms_amd.boundary import DirichletBC
    from poms_amd.dist import CartDistribution, SlabDistribution
    from poms_amd.splines import assemble_1d, make_open_knots
    from poms_amd.stencil import KronOperator, StencilMatrix, StencilVectorSpace
    T = make_open_knots(2, 8)
    M, K = assemble_1d(T, 2)
    spaces = [StencilVectorSpace([8, 8, 8], [2, 2, 2], dist=SlabDistribution(8, 0, 2)),
              StencilVectorSpace([8, 8], [2, 2], dist=CartDistribution((8, 8), (2, 1), 0))]
    for V in spaces:
        nd = V.ndim
        assert V.is_distributed or V.is_cart
        A = StencilMatrix(V)
        for call in (lambda: A.set_dirichlet("all"),
                     lambda: A.set_dirichlet([(True, False)] + [(False, False)] * (nd - 1)),
                     lambda: assemble_stencil(V, [T] * nd, dirichlet="all"),
                     lambda: KronOperator.laplace(V, [M] * nd, [K] * nd, dirichlet="all"),
                     lambda: DirichletBC(V, [T] * nd, "all")):
            with pytest.raises(NotImplementedError, match="distributed"):
                call()
        assert A.dirichlet is None
        A.set_dirichlet(None)
        assert KronOperator.laplace(V, [M] * nd, [K] * nd, dirichlet=None).dirichlet is None


def test_a_mask_on_a_ghost_data_layout_is_refused(gpu):
    """The C entry point on a handle whose layout says that the ghosts of axes 1 and 2 hold
    data (a Cart block): refused whatever g0 and the extents say, and the handle keeps no mask."""
    import ctypes as C

    from poms_amd import _lib
    from poms_amd.stencil import StencilVectorSpace
    V = StencilVectorSpace([5, 6], [1, 1])
    lay = _lib.Layout.make(V.n3, V.p3, V.pitch if V.aligned else 0, _lib.LAYOUT_GHOST_DATA)
    data = np.zeros((7, 8, 3, 3))
    h = C.c_void_p()
    _lib.call("poms_op_create_stencil", V.ctx, 2, C.byref(lay), data.ctypes.data_as(C.c_void_p), 0, 1, C.byref(h))
    try:
        assert _lib.lib.poms_op_set_dirichlet(h, 5) != 0
        msg = _lib.lib.poms_last_error()
        assert b"poms_op_set_dirichlet" in msg and b"Cart" in msg
        out = C.c_int(-1)
        _lib.call("poms_op_get_dirichlet", h, C.byref(out))
        assert out.value == 0
    finally:
        _lib.lib.poms_op_destroy(h)


def test_a_refused_mask_leaves_the_operator_as_it_was(gpu):
    """set_dirichlet asks the library before it records the faces."""
    from poms_amd import _lib
    A, V, _ = build("stencil", (3, 3), (5, 6), False, dirichlet=[(True, False), (False, False)])
    before = A.dirichlet
    real = _lib.call

    def refuse(name, *args):
        if name == "poms_op_set_dirichlet":
            raise _lib.PomsError("poms_op_set_dirichlet: refused for the test")
        return real(name, *args)

    _lib.call = refuse
    try:
        with pytest.raises(ValueError, match="refused"):
            A.set_dirichlet("all")
    finally:
        _lib.call = real
    assert A.dirichlet == before


def test_lift_through_a_spline_mapping(gpu):
    """The control points at the Greville abscissae make a SplineMapping the identity, so the
    lift of g through its `physical` (evaluated on the device, one point on the face's axis)
    is the lift of g in the parameter coordinates."""
    from poms_amd.boundary import DirichletBC, constrained_mask
    from poms_amd.geometry import SplineMapping
    from poms_amd.splines import greville, uniform_knots
    from poms_amd.stencil import StencilVectorSpace
    degs, cells = (2, 3), (4, 5)
    T = [uniform_knots(p, N) for p, N in zip(degs, cells)]
    V = StencilVectorSpace([N + p for p, N in zip(degs, cells)], list(degs))
    gr = np.meshgrid(*[greville(t, p) for t, p in zip(T, degs)], indexing="ij")
    mapping = SplineMapping(V, T, [V.zeros().from_numpy(g) for g in gr])
    g = lambda x, y: np.exp(x) * np.cos(y) + x * y
    faces = [(True, True), (False, True)]
    got = DirichletBC(V, T, faces, mapping=mapping).lift(g).to_local_numpy()
    want = DirichletBC(V, T, faces).lift(g).to_local_numpy()
    C = constrained_mask(V.npts, faces)
    assert np.any(want[C] != 0.0) and not got[~C].any()
    assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))
