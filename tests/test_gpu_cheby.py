"""The Chebyshev-Jacobi smoother on the device: the fused step (csrc/stencil_general.hip,
csrc/matfree.hip, EPI_CHEBY) against its float64 composition and against the composed
path, its storage invariants, the eigenvalue estimate, the solver against a dense
restatement of the recurrence, graph capture, and the V-cycles smoothed with it against
a dense restatement of the same cycle: one cycle, cycle counts, symmetry and the cycle
as pcg's preconditioner.

Shapes: the stencil kernel is one thread per row (odd extents, several blocks in 3D);
the matrix-free kernel has tiles of T = 8 columns (9 = T + 1, 17 = 2T + 1) and cuts
axis 0 into two chunks from 32 planes on (33 planes)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
NO = (False, False)


def a_var(x, y, *z):
    return (1.0 + 0.5 * np.sin(3 * x) * np.cos(2 * y)) * (1.0 + z[0] / 4 if z else 1.0)


def c_var(x, y, *z):
    return 2.0 + x * y


def sheared(d):
    """F = (x + 0.3 y, y(, z)): a constant Jacobian with an off-diagonal entry."""
    from poms_amd.geometry import Mapping
    F = lambda *X: [X[0] + 0.3 * X[1]] + list(X[1:])
    jac = lambda *X: [[1.0 if i == k else (0.3 if (i, k) == (0, 1) else 0.0) for k in range(d)] for i in range(d)]
    return Mapping(F, jac, ndim=d)


def some_faces(nd):
    """Axis 0 lo; the last axis both."""
    return [(True, False)] + [NO] * (nd - 2) + [(True, True)]


# form, functions per axis, degrees
STEP_CASES = {
    "stencil_2d_9x12_p23": ("stencil", (9, 12), (2, 3)),
    "stencil_3d_6x9x17_p123": ("stencil", (6, 9, 17), (1, 2, 3)),
    "matfree_2d_9x17_p23": ("matfree", (9, 17), (2, 3)),
    "matfree_3d_33x9x10_p122": ("matfree", (33, 9, 10), (1, 2, 2)),
    "tensor_2d_9x17_p23": ("tensor", (9, 17), (2, 3)),
}


def build(form, npts, degrees, align, dirichlet=None):
    from poms_amd.assembly import assemble_stencil
    from poms_amd.geometry import MappedDomain
    from poms_amd.matfree import MatrixFreeOperator
    from poms_amd.splines import make_open_knots
    from poms_amd.stencil import StencilVectorSpace
    T = [make_open_knots(p, n) for p, n in zip(degrees, npts)]
    V = StencilVectorSpace(list(npts), list(degrees), align=align)
    if form == "stencil":
        A = assemble_stencil(V, T, a=a_var, c=c_var, dirichlet=dirichlet)
    elif form == "matfree":
        A = MatrixFreeOperator(V, T, a=a_var, c=c_var, dirichlet=dirichlet)
    else:
        A = MappedDomain(V, T, sheared(V.ndim)).operator(a=a_var, c=c_var, matrix_free=True, dirichlet=dirichlet)
        assert A.tensor
    return A, V


def diag_of(A, V):
    if A.form == "matfree":
        return A.diagonal().cpu().numpy()
    return A._data[tuple(slice(p, p + n) for p, n in zip(V.pads, V.npts)) + tuple(V.pads)].copy()


def composition(A, V, bn, xn, yn, alpha, beta):
    """x + beta (x - y_old) + alpha (b - A.dot(x))/diag elementwise in float64, and the
    bound 8 eps (|x| + |beta| (|x| + |y_old|) + |alpha| (|b| + |A x|)/diag): three
    roundings after the row's sum, doubled twice."""
    Ax = A.dot(V.zeros().from_numpy(xn)).to_local_numpy()
    D = diag_of(A, V)
    want = xn + beta * (xn - yn) + alpha * (bn - Ax) / D
    bound = 8 * EPS * (np.abs(xn) + abs(beta) * (np.abs(xn) + np.abs(yn)) + abs(alpha) * (np.abs(bn) + np.abs(Ax)) / D)
    return want, bound


@pytest.mark.parametrize("align", [False, True], ids=["unaligned", "aligned"])
@pytest.mark.parametrize("faces", [False, True], ids=["nofaces", "faces"])
@pytest.mark.parametrize("case", list(STEP_CASES))
def test_fused_step(gpu, case, faces, align):
    import torch
    from poms_amd.boundary import constrained_mask
    form, npts, degrees = STEP_CASES[case]
    fs = some_faces(len(npts)) if faces else None
    A, V = build(form, npts, degrees, align, dirichlet=fs)
    assert A.cheby_supported
    rng = np.random.default_rng(11)
    bn, xn, yn = (rng.uniform(-1, 1, V.npts) for _ in range(3))
    b, x = V.zeros().from_numpy(bn), V.zeros().from_numpy(xn)
    alpha, beta = 0.37, 0.61
    # (a) against the float64 composition; ghosts and dead pitch columns of y untouched
    want, bound = composition(A, V, bn, xn, yn, alpha, beta)
    y = V.zeros()
    y._store.fill_(7.25)
    y.from_numpy(yn)
    outside = torch.ones_like(y._store, dtype=torch.bool)
    V.interior(V.view(outside)).fill_(False)
    A.cheby_step(b, x, y, alpha, beta)
    got = y.to_local_numpy()
    err = np.abs(got - want)
    print(f"{case} faces={faces} align={align}: worst error / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    assert bool(torch.all(y._store[outside] == 7.25))
    # (b) two calls give the same bits
    y2 = V.zeros().from_numpy(yn)
    A.cheby_step(b, x, y2, alpha, beta)
    assert np.array_equal(y2.to_local_numpy(), got)
    # (c) fused against composed (jacobi_sweep and two axpby), the same bound
    y3 = V.zeros().from_numpy(yn)
    A.cheby_step(b, x, y3, alpha, beta, _composed=True)
    errc = np.abs(y3.to_local_numpy() - got)
    print(f"    fused against composed: {np.max(errc / bound):.3f}")
    assert np.all(errc <= bound)
    # (d) beta = 0: the old y is not read (NaN there does not reach the result)
    want0, bound0 = composition(A, V, bn, xn, np.zeros(V.npts), alpha, 0.0)
    y0 = V.zeros()
    V.interior(y0._data).fill_(float("nan"))
    A.cheby_step(b, x, y0, alpha, 0.0)
    got0 = y0.to_local_numpy()
    assert np.all(np.isfinite(got0)) and np.all(np.abs(got0 - want0) <= bound0)
    # (e) constrained entries stay exactly 0 from zero data
    if faces:
        C = constrained_mask(V.npts, fs)
        assert C.any() and (~C).any()
        z = lambda a: V.zeros().from_numpy(np.where(C, 0.0, a))
        yz = z(yn)
        A.cheby_step(z(bn), z(xn), yz, alpha, beta)
        gz = yz.to_local_numpy()
        assert np.all(gz[C] == 0.0) and np.any(gz[~C] != 0.0)


@pytest.mark.parametrize("nd,p", [(2, 3), (3, 2)])
def test_composed_step_kronecker(gpu, nd, p):
    """The Kronecker forms have no fused step: cheby_step composes jacobi_sweep and axpby."""
    from oracle import poms_oracle as orc
    from poms_amd import _lib
    from poms_amd.splines import assemble_1d, uniform_knots
    from poms_amd.stencil import KronOperator, StencilVectorSpace
    N = 9
    M, K = assemble_1d(uniform_knots(p, N), p)
    n = N + p
    V = StencilVectorSpace([n] * nd, [p] * nd)
    A = KronOperator.laplace(V, [M] * nd, [K] * nd)
    assert not A.cheby_supported
    rng = np.random.default_rng(5)
    bn, xn, yn = (rng.uniform(-1, 1, V.npts) for _ in range(3))
    b, x, y = (V.zeros().from_numpy(a) for a in (bn, xn, yn))
    alpha, beta = 0.41, 0.55
    Ax = A.dot(x).to_local_numpy()
    D = orc.kron_sum_diag([M] * nd, [K] * nd)
    want = xn + beta * (xn - yn) + alpha * (bn - Ax) / D
    bound = 8 * EPS * (np.abs(xn) + beta * (np.abs(xn) + np.abs(yn)) + alpha * (np.abs(bn) + np.abs(Ax)) / D)
    A.cheby_step(b, x, y, alpha, beta)
    err = np.abs(y.to_local_numpy() - want)
    print(f"{nd}D p={p}: worst error / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    # the entry point itself refuses the form, aliasing and null pointers
    import ctypes as C
    from poms_amd import runtime as rt
    args = lambda h, bb, xx, yy: (h, 0.1, 0.2, bb, xx, yy, 0, V.local_npts[0] if nd == 3 else 1, rt.stream_handle())
    with pytest.raises(_lib.PomsError, match="Kronecker"):
        _lib.call("poms_op_cheby_step", *args(A._h, rt.ptr(b._data), rt.ptr(x._data), rt.ptr(y._data)))
    with pytest.raises(_lib.PomsError, match="alias"):
        _lib.call("poms_op_cheby_step", *args(A._h, rt.ptr(b._data), rt.ptr(x._data), rt.ptr(x._data)))
    with pytest.raises(_lib.PomsError, match="null"):
        _lib.call("poms_op_cheby_step", *args(A._h, rt.ptr(b._data), None, rt.ptr(y._data)))
    with pytest.raises(ValueError, match="alias"):
        A.cheby_step(b, x, x, alpha, beta)


def uniform_stencil(nd, p, N, dirichlet=None, align=False):
    from poms_amd.assembly import assemble_stencil
    from poms_amd.splines import uniform_knots
    from poms_amd.stencil import StencilVectorSpace
    T = uniform_knots(p, N)
    V = StencilVectorSpace([N + p] * nd, [p] * nd, align=align)
    return assemble_stencil(V, [T] * nd, dirichlet=dirichlet), V


@pytest.mark.parametrize("nd,p,N", [(2, 1, 16), (2, 2, 16), (2, 3, 16), (3, 2, 8), (3, 3, 8)])
def test_estimate_lmax(gpu, nd, p, N):
    """Ten Lanczos steps from the specified start vector: never above lambda_max(D^-1 A), and
    within 3 % of it (the CPU restatement alone gives >= 0.985 on exactly these cases)."""
    from poms_amd.solvers import estimate_lmax
    A, V = uniform_stencil(nd, p, N)
    Ad = A.toarray()
    d = np.diag(Ad)
    lam = np.linalg.eigvalsh(Ad / np.sqrt(np.outer(d, d)))[-1]
    est = estimate_lmax(A, iters=10, seed=0)
    print(f"{nd}D p={p} N={N}: lambda_max {lam:.4f}, estimate {est:.4f}, ratio {est / lam:.4f}")
    assert 0.97 * lam <= est <= lam * (1 + 1e-10)


def dense_chebyshev(Ad, d, b, x0, alpha, beta, dtype=np.float64):
    Ad, d, b = Ad.astype(dtype), d.astype(dtype), b.astype(dtype)
    x = np.zeros_like(b) if x0 is None else x0.astype(dtype)
    xm = x
    for a, be in zip(alpha, beta):
        xm, x = x, x + dtype(be) * (x - xm) + dtype(a) * (b - Ad @ x) / d
    return x


@pytest.mark.parametrize("form", ["stencil", "matfree"])
@pytest.mark.parametrize("from_zero", [False, True], ids=["x0", "zero"])
def test_chebyshev_solver(gpu, form, from_zero):
    """chebyshev(A, b, x0, degree=7) against the dense NumPy recurrence, 2D p = 3, N = 8, every
    face constrained.  Tolerance 100 degree W eps max|x| with W the stencil width, and the
    restatement in long double as well: float64 and long double differ by 1.1e-15 to 2.0e-15,
    far less than a tenth of the tolerance (2.7e-11 to 3.3e-11), so it is not widened."""
    from poms_amd.matfree import MatrixFreeOperator
    from poms_amd.solvers import chebyshev, chebyshev_coefficients
    from poms_amd.splines import uniform_knots
    from poms_amd.stencil import StencilVectorSpace
    p, N, degree = 3, 8, 7
    if form == "stencil":
        A, V = uniform_stencil(2, p, N, dirichlet="all")
        Ad = A.toarray()
    else:
        V = StencilVectorSpace([N + p] * 2, [p] * 2)
        A = MatrixFreeOperator(V, [uniform_knots(p, N)] * 2, a=a_var, c=c_var, dirichlet="all")
        Ad = A.assemble().toarray()
    d = np.diag(Ad).copy()
    rng = np.random.default_rng(3)
    bn = rng.uniform(-1, 1, V.npts)
    x0n = None if from_zero else rng.uniform(-1, 1, V.npts)
    b = V.zeros().from_numpy(bn)
    x0 = None if from_zero else V.zeros().from_numpy(x0n)
    x, info = chebyshev(A, b, x0=x0, degree=degree)
    assert info["niter"] == degree and info["lmax"] == pytest.approx(1.1 * A._lmax_est)
    assert info["lmin"] == pytest.approx(info["lmax"] / 30.0)
    if x0 is not None:
        assert np.array_equal(x0.to_local_numpy(), x0n)   # the caller's x0 is not written
    alpha, beta = chebyshev_coefficients(info["lmin"], info["lmax"], degree)
    flat = lambda a: None if a is None else a.reshape(-1)
    want = dense_chebyshev(Ad, d, flat(bn), flat(x0n), alpha, beta)
    want_ld = dense_chebyshev(Ad, d, flat(bn), flat(x0n), alpha, beta, dtype=np.longdouble)
    W = (2 * p + 1) ** 2
    tol = 100 * degree * W * EPS * np.max(np.abs(want))
    dld = float(np.max(np.abs(want - want_ld)))
    err = float(np.max(np.abs(x.to_local_numpy().reshape(-1) - want)))
    print(f"{form} from_zero={from_zero}: error {err:.3e}, tolerance {tol:.3e}, float64 - long double {dld:.3e}")
    assert dld <= tol / 10
    assert err <= tol


def test_graph_capture(gpu):
    """One step, and a whole smoothing call with its buffers supplied, allocate and
    synchronise nothing: captured after one warm-up, the replay is bitwise the eager result."""
    import torch
    from poms_amd.solvers import chebyshev, chebyshev_work
    A, V = build("matfree", (9, 17), (2, 3), True, dirichlet=some_faces(2))
    rng = np.random.default_rng(4)
    b, x = (V.zeros().from_numpy(rng.uniform(-1, 1, V.npts)) for _ in range(2))
    yn = rng.uniform(-1, 1, V.npts)
    y = V.zeros().from_numpy(yn)
    A.cheby_step(b, x, y, 0.3, 0.6)
    want = y._store.clone()
    y.from_numpy(yn)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        A.cheby_step(b, x, y, 0.3, 0.6)
    y.from_numpy(yn)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y._store, want)
    # the solver
    work = chebyshev_work(A)
    xs, _ = chebyshev(A, b, degree=5, work=work)
    assert any(xs is w for w in work)
    want = xs._store.clone()
    for w in work:
        V.interior(w._data).zero_()
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=st):
        xs2, _ = chebyshev(A, b, degree=5, work=work)
    for w in work:
        V.interior(w._data).zero_()
    torch.cuda.synchronize()
    g2.replay()
    torch.cuda.synchronize()
    assert xs2 is xs and torch.equal(xs._store, want)


# ---- the V-cycles: a dense restatement of the same cycle ------------------------------

def kron_all(ms):
    return functools.reduce(np.kron, ms)


class DenseCycle:
    """The cycle of `_VCycle._level` with the Chebyshev smoother in dense NumPy: the level
    operators as the device applies them, the constrained prolongations, the coefficients
    from the cycle's own lambda_max estimates, an exact coarse solve."""

    def __init__(self, vc, A0=None):
        from poms_amd.boundary import constrain_prolongation
        from poms_amd.solvers import chebyshev_coefficients
        L = len(vc.transfers)
        self.A = [vc.ops[l].toarray() if (l or A0 is None) else A0 for l in range(L)]
        self.d = [np.diag(A).copy() for A in self.A]
        faces = vc.dirichlet or [NO] * len(vc.P[0])
        self.P = [kron_all([constrain_prolongation(Pd, lo, hi) for Pd, (lo, hi) in zip(vc.P[l], faces)])
                  for l in range(L)]
        self.Ac = vc.Ac
        self.coef = []
        for l in range(L):
            hi = vc.cheby_safety * vc.cheby_lmax[l]
            self.coef.append(chebyshev_coefficients(hi / vc.cheby_ratio, hi, vc.cheby_degrees[l]))

    def level(self, l, b, x0):
        sm = lambda x: dense_chebyshev(self.A[l], self.d[l], b, x, *self.coef[l])
        x = sm(x0)
        rc = self.P[l].T @ (b - self.A[l] @ x)
        ec = np.linalg.solve(self.Ac, rc) if l + 1 == len(self.A) else self.level(l + 1, rc, None)
        return sm(x + self.P[l] @ ec)

    def cycle(self, b, x0=None):
        return self.level(0, b, x0)

    def cycles_to(self, b, tol, most=60):
        x, k = None, 0
        while k < most:
            x, k = self.cycle(b, x), k + 1
            if np.linalg.norm(b - self.A[0] @ x) <= tol * np.linalg.norm(b):
                break
        return k, x


def dense_pcg(A, B, b, tol, maxiter=100):
    """`solvers.pcg` (the reference's loop and stop test) with the dense cycle B as psolve."""
    x = np.zeros_like(b)
    r = b.copy()
    nrmr0 = np.sqrt(r @ r)
    s = B(r)
    sr = s @ r
    p = s
    k = 0
    for k in range(1, maxiter + 1):
        q = A @ p
        alpha = sr / (p @ q)
        r = r - alpha * q
        nrmr = r @ r
        x = x + alpha * p
        if nrmr < tol * nrmr0:
            k -= 1
            break
        srold, s = sr, B(r)
        sr = s @ r
        p = s + (sr / srold) * p
    return x, k


@functools.lru_cache(maxsize=None)
def cycles(kind):
    """The two hierarchies of the V-cycle tests with their dense restatements, built once."""
    from poms_amd.matfree import MatrixFreeVCycle
    from poms_amd.mg import GalerkinVCycle
    if kind == "galerkin":
        vc = GalerkinVCycle.uniform(3, 16, 4, 2, dirichlet="all", smoother="chebyshev", cheby_degree=4)
        ref = DenseCycle(vc)
    else:
        vc = MatrixFreeVCycle.uniform(2, 16, 4, 2, a=a_var, c=c_var, dirichlet="all", smoother="chebyshev")
        ref = DenseCycle(vc, A0=vc.A.assemble().toarray())
    rng = np.random.default_rng(8)
    return vc, ref, rng.uniform(-1, 1, vc.space.npts)


@pytest.mark.parametrize("kind", ["galerkin", "matfree"])
def test_vcycle_against_dense(gpu, kind):
    vc, ref, bn = cycles(kind)
    assert vc.smoother == "chebyshev" and vc.nlevels == 3
    V = vc.space
    b = V.zeros().from_numpy(bn)
    x, infos = vc.cycle(b)
    want = ref.cycle(bn.reshape(-1))
    e = float(np.linalg.norm(x.to_local_numpy().reshape(-1) - want) / np.linalg.norm(want))
    print(f"{kind}: one cycle against the restatement {e:.3e}")
    assert e <= 1e-10
    assert all(i[0]["niter"] == i[1]["niter"] == dg for i, dg in zip(infos, vc.cheby_degrees))
    # cycles to ||r|| <= 1e-10 ||b||
    kref, xref = ref.cycles_to(bn.reshape(-1), 1e-10)
    xk, k, nb = None, 0, float(np.sqrt(b.dot(b)))
    while k < 60:
        xk, k = vc.cycle(b, x0=xk)[0], k + 1
        r = vc.A.residual(b, xk)
        if np.sqrt(r.dot(r)) <= 1e-10 * nb:
            break
    print(f"{kind}: {k} cycles to 1e-10 (restatement {kref})")
    assert k == kref and k < 60


def test_vcycle_default_smoother_unchanged(gpu):
    from poms_amd.mg import GalerkinVCycle
    kw = dict(dirichlet="all")
    va = GalerkinVCycle.uniform(3, 16, 4, 2, **kw)
    vb = GalerkinVCycle.uniform(3, 16, 4, 2, smoother="jacobi", **kw)
    assert va.smoother == vb.smoother == "jacobi"
    bn = np.random.default_rng(8).uniform(-1, 1, va.space.npts)
    xa, ia = va.cycle(va.space.zeros().from_numpy(bn))
    xb, ib = vb.cycle(vb.space.zeros().from_numpy(bn))
    assert np.array_equal(xa.to_local_numpy(), xb.to_local_numpy())
    assert ia == ib


@pytest.mark.parametrize("kind", ["galerkin", "matfree"])
def test_cycle_is_symmetric(gpu, kind):
    vc, _, _ = cycles(kind)
    V = vc.space
    rng = np.random.default_rng(21)
    u, v = (V.zeros().from_numpy(rng.uniform(-1, 1, V.npts)) for _ in range(2))
    Bv, Bu = vc.cycle(v)[0], vc.cycle(u)[0]
    uBv, vBu = u.dot(Bv), v.dot(Bu)
    print(f"{kind}: <u,Bv> {uBv:.15e}, <v,Bu> {vBu:.15e}, relative difference {abs(uBv - vBu) / abs(uBv):.2e}")
    assert abs(uBv - vBu) <= 1e-11 * abs(uBv)


def test_pcg_preconditioned_by_the_cycle(gpu):
    from poms_amd.solvers import pcg
    vc, ref, bn = cycles("galerkin")
    V = vc.space
    b = V.zeros().from_numpy(bn)
    x, info = pcg(vc.A, vc.preconditioner(), b, tol=1e-10)
    xr, kr = dense_pcg(ref.A[0], ref.cycle, bn.reshape(-1), 1e-10)
    e = float(np.linalg.norm(x.to_local_numpy().reshape(-1) - xr) / np.linalg.norm(xr))
    print(f"pcg: {info['niter']} iterations (restatement {kr}), solution {e:.3e}")
    assert info["success"] and info["niter"] == kr
    assert e <= 1e-9


def test_vcycle_refusals(gpu):
    from poms_amd.dist import SlabDistribution
    from poms_amd.matfree import MatrixFreeVCycle
    from poms_amd.mg import GalerkinVCycle, MultilevelVCycle, TwoLevelVCycle
    with pytest.raises(ValueError, match="smoother"):
        TwoLevelVCycle(2, 8, 4, ndim=2, smoother="gauss-seidel")
    with pytest.raises(ValueError, match="smoother"):
        GalerkinVCycle.uniform(2, 8, 4, 2, smoother="gauss-seidel")
    with pytest.raises(ValueError, match="smoother"):
        MatrixFreeVCycle.uniform(2, 8, 4, 2, smoother="gauss-seidel")
    with pytest.raises(ValueError, match="GLT"):
        TwoLevelVCycle(2, 8, 4, ndim=2, smoother="chebyshev", post_smoother="glt")
    for cls in (TwoLevelVCycle, MultilevelVCycle):
        with pytest.raises(ValueError, match="distributed"):
            cls(2, 8, 4, ndim=3, smoother="chebyshev", dist=SlabDistribution(10, 0, 2))
    # the Kronecker cycles take the smoother too (the composed step)
    mg = TwoLevelVCycle(3, 8, 4, ndim=2, smoother="chebyshev", cheby_degree=3)
    x, ipre, ipos = mg.cycle(mg.rhs_ones())
    assert ipre["niter"] == ipos["niter"] == 3 and np.all(np.isfinite(x.to_local_numpy()))
