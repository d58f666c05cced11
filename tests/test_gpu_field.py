"""Spline fields on the device (csrc/spline_field.hip, poms_amd/field.py): evaluation,
load vector and fused L2 error against a long-double reference kept here, the tie to the
verified mass operator, and a manufactured solution converging at the B-spline rate.

Reference: dense collocation tables from ``basis_funs_ders``, contracted axis by axis
with ``np.tensordot`` in ``np.longdouble``.

Tolerance (derived, not tuned): a sum-factorised value with at most ``L`` terms per axis
carries a forward error of at most ``(3 L + 6) 2^-53 S``, ``S`` being the same contraction
of the absolute tables and the absolute input; ``L = p+1`` for the evaluation and
``L = (p+1) nq`` for the load vector.  Every comparison is elementwise against it.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from poms_amd.splines import assemble_1d, band_to_dense, basis_funs_ders, find_span, uniform_knots

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble


def _nonuniform_knots(p, cells, power=1.4):
    breaks = np.linspace(0.0, 1.0, cells + 1) ** power
    return np.concatenate([np.zeros(p), breaks, np.ones(p)])


def _colloc(T, p, pts):
    """Dense (2, Q, n) values / first derivatives of every basis function at ``pts``."""
    n = len(T) - p - 1
    out = np.zeros((2, len(pts), n))
    for q, x in enumerate(pts):
        s = find_span(T, p, x)
        D = basis_funs_ders(T, p, x, s, 1)
        out[:, q, s - p:s + 1] = D
    return out


def _contract(mats, a):
    """``(mats[0] (x) mats[1] (x) ...) a`` by one tensordot per axis, in long double."""
    a = np.asarray(a, dtype=LD)
    for d, m in enumerate(mats):
        a = np.moveaxis(np.tensordot(np.asarray(m, dtype=LD), a, axes=(1, d)), 0, d)
    return a


def _within(got, ref, S, L, extra=0.0):
    """max over the entries of |got - ref| / bound; the bound is (3 L + 6) u S (+ extra)."""
    bound = (3 * L + 6) * U * np.asarray(S, dtype=np.float64) + extra
    err = np.abs(np.asarray(got, dtype=LD) - ref).astype(np.float64)
    bad = err > bound
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    print(f"max err/bound = {ratio:.3f} (max err {err.max():.3e}, L = {L})")
    return not bad.any()


CASES = {
    # name: (degrees, cells, knots, align)
    "1d_p2": ((2,), (150,), "uniform", False),
    "2d_p23": ((2, 3), (6, 5), "nonuniform", False),
    "3d_p3": ((3, 3, 3), (3, 2, 17), "uniform", False),
    "3d_p3_aligned": ((3, 3, 3), (3, 2, 17), "uniform", True),
    "3d_p5": ((5, 5, 5), (3, 3, 3), "uniform", False),
    "3d_p1": ((1, 1, 1), (4, 4, 4), "nonuniform", False),
    # the load vector's first pass: two tiles of basis functions (256 + 46) in the register kernel,
    "1d_p2_300": ((2,), (300,), "uniform", False, 4),
    # two points per span: 256 points reach 130 columns, past the 128 the last pass stages in one go,
    "1d_p2_nq2": ((2,), (300,), "nonuniform", False, 2),
    # rows of 1200 points, more than a tile of it holds: the general kernel, two LDS segments,
    "1d_p2_nq8": ((2,), (150,), "uniform", False, 8),
    # and 51 points per basis function, 2550 per row: the general kernel, three segments
    "1d_p2_nq17": ((2,), (150,), "nonuniform", False, 17),
}


class Case:
    def __init__(self, name, chunk_bytes=None):
        import torch
        from poms_amd.field import QuadGrid
        from poms_amd.stencil import StencilVectorSpace
        self.p, self.cells, kind, self.align = CASES[name][:4]
        self.nquad = nquad = CASES[name][4] if len(CASES[name]) > 4 else None
        self.nd = len(self.p)
        self.knots = [uniform_knots(p, c) if kind == "uniform" else _nonuniform_knots(p, c)
                      for p, c in zip(self.p, self.cells)]
        self.npts = tuple(len(T) - p - 1 for T, p in zip(self.knots, self.p))
        self.V = StencilVectorSpace(self.npts, self.p, align=self.align)
        kw = {} if chunk_bytes is None else {"chunk_bytes": chunk_bytes}
        self.grid = QuadGrid(self.V, self.knots, nquad, **kw)
        rng = np.random.default_rng(sum(map(ord, name)))
        self.x = rng.uniform(-1, 1, self.npts)
        self.xv = self.V.zeros().from_numpy(self.x)
        self.f = rng.uniform(-1, 1, self.grid.shape)
        self.u = rng.uniform(-1, 1, self.grid.shape)
        self.col = [_colloc(T, p, pts) for T, p, pts in zip(self.knots, self.p, self.grid.points)]
        self.nq = [nquad or p + 1 for p in self.p]
        self.torch = torch

    def mats(self, der):
        return [c[k] for c, k in zip(self.col, der)]

    @functools.lru_cache(maxsize=None)
    def eval_ref(self, der):
        m = self.mats(der)
        return _contract(m, self.x), _contract([np.abs(a) for a in m], np.abs(self.x)).astype(np.float64)

    @functools.lru_cache(maxsize=None)
    def load_ref(self):
        m = [(w[:, None] * c[0]).T for w, c in zip(self.grid.weights, self.col)]
        return _contract(m, self.f), _contract([np.abs(a) for a in m], np.abs(self.f)).astype(np.float64)

    def chunked(self, k):
        """The same space and data on a grid walked in chunks of ``k`` axis-0 points."""
        return _case(self.name, 8 * self.grid.shape[1] * self.grid.shape[2] * k)


@functools.lru_cache(maxsize=None)
def _case(name, chunk_bytes=None):
    c = Case(name, chunk_bytes)
    c.name = name
    return c


def _ders(nd):
    return [(0,) * nd] + [tuple(int(k == d) for k in range(nd)) for d in range(nd)]


EVAL_PARAMS = [(name, der) for name in CASES for der in _ders(len(CASES[name][0]))]


# ---- 1. evaluation --------------------------------------------------------------------
@pytest.mark.parametrize("name,der", EVAL_PARAMS, ids=[f"{n}-der{''.join(map(str, d))}" for n, d in EVAL_PARAMS])
def test_evaluate_against_reference(gpu, name, der):
    c = _case(name)
    got = c.grid.evaluate(c.xv, der=der)
    assert tuple(got.shape) == c.grid.shape == tuple(ce * nq for ce, nq in zip(c.cells, c.nq))
    ref, S = c.eval_ref(der)
    assert _within(got.cpu().numpy(), ref, S, max(c.p) + 1)


def _irregular_points(rng, k):
    inner = rng.uniform(0.0, 1.0, k - 3)
    return np.sort(np.concatenate([[0.0, 1.0], inner, inner[:1]]))   # both ends, one repeated point


@pytest.mark.parametrize("name", ["2d_p23", "3d_p3", "3d_p3_aligned"])
def test_evaluate_on_point_grid(gpu, name):
    from poms_amd.field import PointGrid, evaluate
    c = _case(name)
    rng = np.random.default_rng(5)
    pts = [_irregular_points(rng, k) for k in (7, 11, 9)[:c.nd]]
    g = PointGrid(c.V, c.knots, pts)
    assert g.shape == tuple(len(q) for q in pts) and g.weights is None
    col = [_colloc(T, p, q) for T, p, q in zip(c.knots, c.p, pts)]
    for der in _ders(c.nd):
        m = [a[k] for a, k in zip(col, der)]
        ref = _contract(m, c.x)
        S = _contract([np.abs(a) for a in m], np.abs(c.x)).astype(np.float64)
        assert _within(g.evaluate(c.xv, der=der).cpu().numpy(), ref, S, max(c.p) + 1)
    # open knots interpolate the corner coefficients at the domain's corners
    v = evaluate(c.V, c.knots, c.xv, pts).cpu().numpy()
    assert abs(v[(0,) * c.nd] - c.x[(0,) * c.nd]) <= 1e-14 and abs(v[(-1,) * c.nd] - c.x[(-1,) * c.nd]) <= 1e-14


def test_evaluate_on_sparse_points(gpu):
    """Few points on many spans: consecutive points share no inputs (the middle pass reloads
    its window) and one tile of points reaches more columns than the last pass stages."""
    from poms_amd.field import PointGrid
    from poms_amd.stencil import StencilVectorSpace
    p, cells = (2, 2), (30, 400)
    knots = [_nonuniform_knots(pd, c, 1.2) for pd, c in zip(p, cells)]
    npts = tuple(c + pd for c, pd in zip(cells, p))
    V = StencilVectorSpace(npts, p)
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, npts)
    xv = V.zeros().from_numpy(x)
    pts = [_irregular_points(rng, 8), _irregular_points(rng, 9)]
    g = PointGrid(V, knots, pts)
    col = [_colloc(T, pd, q) for T, pd, q in zip(knots, p, pts)]
    for der in _ders(2):
        m = [a[k] for a, k in zip(col, der)]
        S = _contract([np.abs(a) for a in m], np.abs(x)).astype(np.float64)
        assert _within(g.evaluate(xv, der=der).cpu().numpy(), _contract(m, x), S, 3)


# ---- 2. chunking ----------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 5])
def test_chunked_evaluation_is_bitwise_the_unchunked(gpu, k):
    c = _case("3d_p3")
    ck = c.chunked(k)
    assert ck.grid.chunk_q0 == k and c.grid.chunk_q0 == c.grid.shape[0]
    for der in _ders(3):
        assert c.torch.equal(ck.grid.evaluate(ck.xv, der=der), c.grid.evaluate(c.xv, der=der))


# ---- 3. load vector -------------------------------------------------------------------
def _as_callable(c, f_dev):
    """A callable of the per-axis point tensors that reproduces the array ``f_dev``."""
    p0 = c.torch.from_numpy(c.grid.points[0]).to(f_dev.device)

    def f(*X):
        assert len(X) == c.nd and all(x.dim() == c.nd and x.is_cuda for x in X)
        if c.nd < 3:
            return f_dev
        idx = c.torch.searchsorted(p0, X[0].reshape(-1).contiguous())
        return f_dev[idx]
    return f


def _outside_interior(V, vec):
    s = vec._store.clone()
    V.interior(V.view(s)).zero_()
    return s


@pytest.mark.parametrize("name", list(CASES))
def test_load_vector_against_reference(gpu, name):
    c = _case(name)
    ref, S = c.load_ref()
    L = max((p + 1) * nq for p, nq in zip(c.p, c.nq))
    b = c.grid.load_vector(c.f)
    assert _within(b.to_local_numpy(), ref, S, L)
    f_dev = c.torch.from_numpy(c.f).to(gpu)
    b_call = c.grid.load_vector(_as_callable(c, f_dev))
    assert c.torch.equal(b_call._store, b._store)
    assert c.torch.equal(c.grid.load_vector(f_dev)._store, b._store)          # twice: the same bits
    assert not _outside_interior(c.V, b).any()                                # ghosts, dead pitch columns
    # into a vector that holds something else: the interior is overwritten, the rest untouched
    out = c.V.zeros().from_numpy(np.full(c.npts, 7.0))
    assert c.grid.load_vector(c.f, out=out) is out and c.torch.equal(out._store, b._store)


@pytest.mark.parametrize("k", [1, 5])
def test_chunked_load_vector(gpu, k):
    c = _case("3d_p3_aligned")
    ck = c.chunked(k)
    ref, S = c.load_ref()
    L = max((p + 1) * nq for p, nq in zip(c.p, c.nq))
    b = ck.grid.load_vector(ck.f)
    assert _within(b.to_local_numpy(), ref, S, L)
    f_dev = c.torch.from_numpy(ck.f).to(gpu)
    assert c.torch.equal(ck.grid.load_vector(_as_callable(ck, f_dev))._store, b._store)
    assert not _outside_interior(ck.V, b).any()


# ---- 4. the verified operators --------------------------------------------------------
@pytest.mark.parametrize("name", ["2d_p23", "3d_p3", "3d_p3_aligned", "3d_p1"])
def test_load_of_evaluation_is_the_mass_operator(gpu, name):
    from poms_amd.stencil import KronOperator
    c = _case(name)
    M = [assemble_1d(T, p)[0] for T, p in zip(c.knots, c.p)]
    ref = KronOperator.product(c.V, M).dot(c.xv).to_local_numpy()
    vals = c.grid.evaluate(c.xv)
    b = c.grid.load_vector(vals)
    m = [(w[:, None] * a[0]).T for w, a in zip(c.grid.weights, c.col)]
    S = _contract([np.abs(a) for a in m], np.abs(vals.cpu().numpy())).astype(np.float64)
    L = max((p + 1) * nq for p, nq in zip(c.p, c.nq))
    assert _within(b.to_local_numpy(), ref.astype(LD), S, L, extra=1e-13 * np.abs(ref).max())


@pytest.mark.parametrize("name", list(CASES))
def test_load_vector_of_one_sums_to_the_volume(gpu, name):
    from poms_amd.field import assemble_rhs
    c = _case(name)
    b = c.grid.load_vector(1.0)
    assert abs(float(c.V.interior(b._data).sum().item()) - 1.0) <= 1e-13     # the unit cube / square / interval
    assert c.torch.equal(assemble_rhs(c.V, c.knots, 1.0, c.nquad)._store, b._store)


# ---- 5. fused error ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("k", [None, 2])
def test_fused_l2_error(gpu, name, k):
    c = _case(name)
    g = c.grid if k is None or c.nd < 3 else c.chunked(k).grid
    t = c.torch
    W = functools.reduce(lambda a, b: a[..., None] * b, [t.from_numpy(w).to(gpu) for w in g.weights])
    u_dev = t.from_numpy(c.u).to(gpu)
    for der in _ders(c.nd):
        ev = g.evaluate(c.xv, der=der)
        ref = float((W * (ev - u_dev) ** 2).sum().item())
        got = g.l2_error(c.xv, u_dev, der=der) ** 2
        print(f"{name} der {der}: fused {got:.17e}, torch {ref:.17e}, rel {abs(got - ref) / ref:.2e}")
        assert abs(got - ref) <= 1e-12 * ref
        ref0 = float((W * ev ** 2).sum().item())
        got0 = g.l2_error(c.xv, None, der=der) ** 2
        assert abs(got0 - ref0) <= 1e-12 * ref0
        assert g.l2_error(c.xv, u_dev, der=der) ** 2 == got                   # twice: the same bits
        assert g.l2_error(c.xv, _as_callable(c, u_dev), der=der) ** 2 == got  # u as a callable


def test_h1_seminorm_error(gpu):
    c = _case("3d_p3")
    t = c.torch
    grads = [t.from_numpy(np.roll(c.u, d + 1, axis=d)).to(gpu) for d in range(3)]
    parts = [c.grid.l2_error(c.xv, grads[d], der=tuple(int(k == d) for k in range(3))) ** 2 for d in range(3)]
    got = c.grid.h1_seminorm_error(c.xv, grads)
    assert abs(got - math.sqrt(sum(parts))) <= 1e-14 * got


# ---- 6. manufactured solution ---------------------------------------------------------
def _solve_manufactured(nd, p, N):
    """-Δu + u = f with u = Π cos(π x_d) (natural boundary conditions), N^nd cells:
    the device solve's coefficients, the L2 error and the dense system."""
    import torch
    from poms_amd.field import QuadGrid, assemble_rhs
    from poms_amd.solvers import jacobi, pcg
    from poms_amd.stencil import KronOperator, StencilVectorSpace
    T = uniform_knots(p, N)
    n = N + p
    M, K = assemble_1d(T, p)
    V = StencilVectorSpace([n] * nd, [p] * nd)
    A = KronOperator.laplace(V, [M] * nd, [K] * nd)
    u = lambda *X: functools.reduce(lambda a, b: a * b, [torch.cos(math.pi * x) for x in X])
    f = lambda *X: (1.0 + nd * math.pi ** 2) * u(*X)
    b = assemble_rhs(V, [T] * nd, f)
    bn = math.sqrt(b.dot(b))
    x, rn = None, bn
    for _ in range(5):   # pcg stops on its recurrence's ||r||^2 < tol ||r0||; the true residual decides here
        x, _info = pcg(A, jacobi, b, x0=x, tol=(2e-14 * bn) ** 2 / rn, maxiter=1000)
        r = A.residual(b, x)
        rn = math.sqrt(r.dot(r))
        if rn <= 1e-13 * bn:
            break
    print(f"{nd}D p={p} N={N}: ||b - A x|| / ||b|| = {rn / bn:.2e}")
    assert rn <= 1e-12 * bn
    err = QuadGrid(V, [T] * nd).l2_error(x, u)
    return x.to_local_numpy(), b.to_local_numpy(), err, (band_to_dense(M), band_to_dense(K))


def _dense_solve(nd, Md, Kd, b):
    def kron(fs):
        return functools.reduce(np.kron, fs)
    A = kron([Md] * nd)
    for d in range(nd):
        A = A + kron([Kd if k == d else Md for k in range(nd)])
    return np.linalg.solve(A, b.reshape(-1)).reshape(b.shape)


@pytest.mark.parametrize("nd,p,Ns", [(2, 3, (8, 16, 32)), (3, 2, (4, 8))], ids=["2d_p3", "3d_p2"])
def test_manufactured_solution_converges_at_the_spline_rate(gpu, nd, p, Ns):
    errs = []
    for N in Ns:
        x, b, err, (Md, Kd) = _solve_manufactured(nd, p, N)
        errs.append(err)
        if x.size <= 1000:
            xd = _dense_solve(nd, Md, Kd, b)
            rel = np.linalg.norm(x - xd) / np.linalg.norm(xd)
            print(f"{nd}D p={p} N={N}: coefficients vs dense solve {rel:.2e}")
            assert rel <= 1e-9
    ratios = [a / b for a, b in zip(errs, errs[1:])]
    print(f"{nd}D p={p}: L2 errors {errs}, ratios {ratios}")
    assert all(r >= 0.8 * 2 ** (p + 1) for r in ratios)


# ---- 7. errors ------------------------------------------------------------------------
def test_distributed_space_is_not_implemented(gpu):
    from poms_amd.dist import SlabDistribution
    from poms_amd.field import PointGrid, QuadGrid
    from poms_amd.stencil import StencilVectorSpace
    T = uniform_knots(2, 6)
    V = StencilVectorSpace([8, 8, 8], [2, 2, 2], dist=SlabDistribution(8, 0, 2))
    with pytest.raises(NotImplementedError, match="undistributed"):
        QuadGrid(V, [T] * 3)
    with pytest.raises(NotImplementedError):
        PointGrid(V, [T] * 3, [[0.0, 0.5]] * 3)


def test_bad_arguments_raise_before_any_launch(gpu):
    from poms_amd import _lib
    from poms_amd.field import PointGrid
    c = _case("3d_p3")
    g = c.grid
    pg = PointGrid(c.V, c.knots, [[0.0, 0.5, 1.0]] * 3)
    with pytest.raises(ValueError, match="weights"):
        pg.load_vector(1.0)
    with pytest.raises(ValueError, match="weights"):
        pg.l2_error(c.xv, 0.0)
    with pytest.raises(ValueError, match="der"):
        g.evaluate(c.xv, der=(2, 0, 0))
    with pytest.raises(ValueError, match="der"):
        g.l2_error(c.xv, None, der=(0, 0))
    with pytest.raises(ValueError, match="shape"):
        g.load_vector(np.zeros(g.shape[:-1] + (g.shape[-1] + 1,)))
    with pytest.raises(ValueError, match="shape"):
        g.l2_error(c.xv, c.torch.zeros(g.shape[1:], dtype=c.torch.float64, device=gpu))
    with pytest.raises(TypeError):
        g.evaluate(_case("3d_p5").xv)
    # the C entry points check their own ranges: nothing is launched on a bad call
    der = (C.c_int * 3)(0, 0, 0)
    out = c.torch.zeros(g.shape, dtype=c.torch.float64, device=gpu)
    x, o = C.c_void_p(c.xv._data.data_ptr()), C.c_void_p(out.data_ptr())
    Q0 = g.shape[0]
    assert _lib.lib.poms_field_eval(g._h, x, der, 0, Q0 + 1, o, None) != 0
    assert _lib.lib.poms_field_eval(g._h, x, der, -1, 2, o, None) != 0
    assert _lib.lib.poms_field_eval(g._h, x, (C.c_int * 3)(0, 2, 0), 0, Q0, o, None) != 0
    assert _lib.lib.poms_field_eval(c.chunked(5).grid._h, x, der, 0, 6, o, None) != 0
    assert b"max_chunk" in _lib.lib.poms_last_error()
    assert _lib.lib.poms_field_load(pg._h, o, 0, 3, 0, x, None) != 0
    assert _lib.lib.poms_field_error(pg._h, x, der, None, 0, 3, o, None) != 0
    assert not out.any()
