"""Robin and Neumann boundary conditions on the device: the stored stencil and the
matrix-free operator with face terms against a dense oracle built here from NumPy
(``A₀.toarray()`` of the operator without ``robin`` plus ``S`` from collocation matrices at
Gauss points, scattered to the boundary rows), the epilogues, reproducibility, storage, the
face-free builds, the combination with Dirichlet faces, the Kronecker form, the hierarchies,
the refusals, and solved problems against CPU restatements.

Shapes: the smallest that reach every branch of the 8 x 8 tiles and the >= 16-plane axis-0
chunks of the matrix-free kernel (9 x 17 functions: a ragged second tile; 33 x 9 x 17: the
axis-0 hi face lies in the second chunk)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


def maxrel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def a_var(x, y, *z):
    return (1.0 + 0.5 * np.sin(3 * x) * np.cos(2 * y)) * (1.0 + z[0] / 4 if z else 1.0)


def c_var(x, y, *z):
    return 2.0 + x * y


def open_knots(breaks, p):
    b = np.asarray(breaks, dtype=np.float64)
    return np.concatenate([[b[0]] * p, b, [b[-1]] * p])


# test_gpu_matfree.py's: graded spacing, and the interior knot 0.5 twice (an empty span)
NONUNIFORM = [0, .02, .06, .14, .3, .5, .5, .62, .7, .75, .9, 1]


def knots_of(degrees, cells):
    from poms_amd.splines import make_open_knots
    return [open_knots(NONUNIFORM, p) if N == "nonuniform" else make_open_knots(p, N + p)
            for p, N in zip(degrees, cells)]


# ---- the NumPy side: Gauss points, collocation matrices, the dense face mass and loads ----
def gauss(T, nq):
    """Gauss points and weights on the non-empty spans of T."""
    xg, wg = np.polynomial.legendre.leggauss(nq)
    br = np.unique(np.asarray(T, float))
    pts = np.concatenate([a + 0.5 * (b - a) * (xg + 1.0) for a, b in zip(br[:-1], br[1:])])
    w = np.concatenate([0.5 * (b - a) * wg for a, b in zip(br[:-1], br[1:])])
    return pts, w


def colloc(T, p, pts, der=0):
    """C[q, j] = B_j^(der)(pts[q])."""
    from poms_amd.splines import basis_funs_ders, find_span
    T = np.asarray(T, float)
    Cm = np.zeros((len(pts), len(T) - p - 1))
    for q, x in enumerate(pts):
        s = find_span(T, p, float(x))
        Cm[q, s - p:s + 1] = basis_funs_ders(T, p, float(x), s, der)[der]
    return Cm


def all_faces(nd):
    return [(d, s) for d in range(nd) for s in (0, 1)]


def beta_of(face, nd, mapped=False):
    """A different variable β per face: a callable of the face's d-1 parameter coordinates
    (of the d physical coordinates under a mapping)."""
    k = 2 * face[0] + face[1]
    if mapped or nd == 3:
        return lambda *X: 1.0 + 0.25 * k + 0.5 * X[0] + 0.3 * X[-1] * X[0]
    return lambda t: 1.0 + 0.25 * k + 0.5 * t + 0.3 * np.sin(2 * t)


def face_grid(T, degrees, face, nq=None):
    """Per axis (points, weights) of the face's quadrature grid; the normal axis is its end point."""
    axis, side = face
    out = []
    for d, (t, p) in enumerate(zip(T, degrees)):
        if d == axis:
            out.append((np.array([t[p] if side == 0 else t[len(t) - p - 1]]), np.ones(1)))
        else:
            out.append(gauss(t, p + 1 if nq is None else nq))
    return out


def face_values(T, degrees, face, f, mapping=None):
    """(f w ds, grid) on the face's quadrature grid, the normal axis kept with one point."""
    axis, _ = face
    grid = face_grid(T, degrees, face)
    G = np.meshgrid(*[g[0] for g in grid], indexing="ij")
    w = functools.reduce(np.multiply.outer, [g[1] for g in grid])
    if mapping is None:
        X = [g for d, g in enumerate(G) if d != axis]
    else:
        X = [np.broadcast_to(np.asarray(x, float), G[0].shape) for x in mapping.F(*G)]
        J = mapping.jac(*G)
        nd = len(T)
        Jn = np.stack([np.stack([np.broadcast_to(np.asarray(J[i][k], float), G[0].shape) for k in range(nd)], axis=-1)
                       for i in range(nd)], axis=-2)
        tang = [k for k in range(nd) if k != axis]
        if nd == 2:
            w = w * np.linalg.norm(Jn[..., :, tang[0]], axis=-1)
        else:
            w = w * np.linalg.norm(np.cross(Jn[..., :, tang[0]], Jn[..., :, tang[1]]), axis=-1)
    v = np.broadcast_to(np.asarray(f(*X) if callable(f) else float(f), float), G[0].shape)
    return v * w, grid


def face_basis(T, degrees, face, grid):
    """Collocation matrices per axis at the face's grid: the normal axis has one row, the unit
    vector of the end function."""
    return [colloc(t, p, g[0]) for t, p, g in zip(T, degrees, grid)]


def dense_face_mass(T, degrees, robin, mapping=None):
    """S = sum_faces int_Γ β φ_i φ_j ds as a dense matrix over the grid in C order."""
    shape = tuple(len(t) - p - 1 for t, p in zip(T, degrees))
    n = int(np.prod(shape))
    S = np.zeros((n, n))
    for face, beta in robin.items():
        v, grid = face_values(T, degrees, face, beta, mapping)
        Cs = face_basis(T, degrees, face, grid)
        B = Cs[0]
        for Cd in Cs[1:]:   # B[q, i] over the tensor grid and the tensor basis, C order
            B = np.einsum("qi,rj->qrij", B, Cd).reshape(B.shape[0] * Cd.shape[0], -1)
        S += B.T @ (v.reshape(-1, 1) * B)
    return S


def dense_face_load(T, degrees, g, mapping=None):
    """sum_faces int_Γ g φ_i ds as an array of the grid's shape."""
    shape = tuple(len(t) - p - 1 for t, p in zip(T, degrees))
    out = np.zeros(shape)
    for face, gf in g.items():
        v, grid = face_values(T, degrees, face, gf, mapping)
        for d, Cd in enumerate(face_basis(T, degrees, face, grid)):
            v = np.moveaxis(np.tensordot(Cd.T, v, axes=(1, d)), 0, d)
        out += v
    return out


# ---- parity --------------------------------------------------------------------------------
# name: (degrees, cells, faces, align).  The aligned spaces have a row pitch (dead columns
# behind every row) and a shifted start: 17 + 6 columns in rows of 32, 17 + 4 in rows of 32.
CASES = {
    "2d_p33_6x14": ((3, 3), (6, 14), "all", False),               # 9 x 17 functions: a ragged second tile
    "2d_p33_6x14_aligned": ((3, 3), (6, 14), "all", True),
    "2d_p23_6x5": ((2, 3), (6, 5), "all", False),
    "2d_p33_nonuniform": ((3, 3), ("nonuniform", 7), "all", False),
    "3d_p321_3x4x5": ((3, 2, 1), (3, 4, 5), "all", False),
    "3d_p222_31x7x15": ((2, 2, 2), (31, 7, 15), "all", False),   # 33 x 9 x 17: axis-0 hi in the second chunk
    "3d_p222_31x7x15_aligned": ((2, 2, 2), (31, 7, 15), "all", True),
    "2d_p33_6x14_one_face": ((3, 3), (6, 14), [(1, 1)], False),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(V, T, robin, A0 dense, S dense) of a case: the references, computed once and shared."""
    from poms_amd.assembly import assemble_stencil
    from poms_amd.stencil import StencilVectorSpace
    degrees, cells, faces, align = CASES[name]
    T = knots_of(degrees, cells)
    nd = len(degrees)
    V = StencilVectorSpace([len(t) - p - 1 for t, p in zip(T, degrees)], list(degrees), align=align)
    assert V.aligned == align and (V.pitch > V.padded_shape[-1]) == align   # (dead pitch columns where aligned)
    robin = {f: beta_of(f, nd) for f in (all_faces(nd) if faces == "all" else faces)}
    A0 = assemble_stencil(V, T, a=a_var, c=c_var).toarray()
    S = dense_face_mass(T, degrees, robin)
    for M in (A0, S):
        M.setflags(write=False)
    return V, T, robin, A0, S


def operators(name):
    from poms_amd.assembly import assemble_stencil
    from poms_amd.matfree import MatrixFreeOperator
    V, T, robin, A0, S = case(name)
    As = assemble_stencil(V, T, a=a_var, c=c_var, robin=robin)
    Am = MatrixFreeOperator(V, T, a=a_var, c=c_var, robin=robin)
    return As, Am


@pytest.mark.parametrize("name", list(CASES))
def test_stored_stencil_equals_the_dense_oracle(gpu, name):
    from poms_amd.assembly import assemble_stencil
    from poms_amd.boundary import RobinBC
    V, T, robin, A0, S = case(name)
    want = A0 + S
    A = assemble_stencil(V, T, a=a_var, c=c_var, robin=robin)
    assert A.face_terms() == tuple(robin)
    err = np.max(np.abs(A.toarray() - want)) / np.max(np.abs(want))
    print(f"{name}: stored stencil against the oracle {err:.2e}")
    assert err <= 1e-13
    assert np.array_equal(A.toarray(), A.toarray().T) or maxrel(A.toarray(), A.toarray().T) <= 1e-13
    # no stale host copy: a stencil whose host data was read takes the term afterwards
    B = assemble_stencil(V, T, a=a_var, c=c_var)
    assert np.array_equal(B.toarray(), A0) and B.face_terms() == ()
    RobinBC(V, T, robin).apply(B)
    assert np.array_equal(B.toarray(), A.toarray())
    x = V.zeros().from_numpy(np.random.default_rng(1).uniform(-1, 1, V.npts))
    assert np.array_equal(B.dot(x).to_local_numpy(), A.dot(x).to_local_numpy())


@pytest.mark.parametrize("name", list(CASES))
def test_matrix_free_equals_the_stored_stencil(gpu, name):
    """dot to 1e-13 (maxrel) on a random x, the diagonal against the stencil's centre, two calls
    bitwise equal, ghost cells and dead pitch columns exactly zero."""
    import torch
    V, T, robin, A0, S = case(name)
    As, Am = operators(name)
    assert Am.face_terms() == tuple(robin)
    xn = np.random.default_rng(2).uniform(-1, 1, V.npts)
    x = V.zeros().from_numpy(xn)
    ys, ym = As.dot(x).to_local_numpy(), Am.dot(x).to_local_numpy()
    print(f"{name}: matrix-free against stored {maxrel(ym, ys):.2e}, against the oracle "
          f"{maxrel(ym, ((A0 + S) @ xn.reshape(-1)).reshape(V.npts)):.2e}")
    assert maxrel(ym, ys) <= 1e-13
    assert maxrel(ym, ((A0 + S) @ xn.reshape(-1)).reshape(V.npts)) <= 1e-13
    centre = As._data[tuple(slice(p, p + n) for p, n in zip(V.pads, V.npts)) + tuple(V.pads)]
    d = Am.diagonal().cpu().numpy()
    assert maxrel(d, centre) <= 1e-13
    assert maxrel(d, np.diag(A0 + S).reshape(V.npts)) <= 1e-13
    # the assembled form of the matrix-free operator has the same face terms
    assert maxrel(Am.assemble().toarray(), As.toarray()) <= 1e-13
    # reproducibility and storage
    out = V.zeros()
    V.interior(out._data).fill_(float("nan"))
    Am.dot(x, out=out)
    assert np.array_equal(out.to_local_numpy(), ym)
    store = out._store.clone()
    inner = torch.zeros_like(store)
    V.interior(V.view(inner)).fill_(1.0)
    assert bool(torch.isfinite(V.interior(out._data)).all())
    assert int(inner.sum().item()) == V.dimension and int((inner == 0).sum().item()) > 0
    assert bool((store[inner == 0] == 0).all())
    # the same for the stored stencil and for an epilogue that reads and writes y
    for A in (As, Am):
        out = V.zeros()
        A.dot(x, out=out)
        b = V.zeros().from_numpy(xn[::-1].copy())
        A.cheby_step(b, x, out, 0.4, 0.3)
        assert bool((out._store[inner == 0] == 0).all())


def count(degrees):
    """test_gpu_matfree.py's count() at nq = p + 1."""
    return sum((p + 1) * (2 * (p + 1) + 1) for p in degrees) + 8 + (3 if len(degrees) == 2 else 0)


@pytest.mark.parametrize("name", ["2d_p33_6x14", "2d_p33_6x14_aligned", "3d_p321_3x4x5", "3d_p222_31x7x15",
                                  "3d_p222_31x7x15_aligned"])
def test_matrix_free_epilogues(gpu, name):
    """residual, jacobi_sweep with both sums, dot_inner and cheby_step against the same
    quantities composed in NumPy from dot, diagonal(), b and x.  Vectors: test_epilogues' bound
    (L + 2 roundings of |b| + S_i, here with S_i = (|A + S| |x|)_i, which is no larger than its
    sum of absolute factors) plus (2p+1)^(d-1) roundings per face; scalars within 1e-13 sum |terms|."""
    V, T, robin, A0, S = case(name)
    degrees = V.pads
    _, A = operators(name)
    rng = np.random.default_rng(5)
    xn, bn, yn = (rng.uniform(-1, 1, V.npts) for _ in range(3))
    x, b = V.zeros().from_numpy(xn), V.zeros().from_numpy(bn)
    y = A.dot(x).to_local_numpy()
    D = A.diagonal().cpu().numpy()
    Sabs = (np.abs(A0 + S) @ np.abs(xn).reshape(-1)).reshape(V.npts)
    nf = sum(int(np.prod([2 * p + 1 for d, p in enumerate(degrees) if d != f[0]])) for f in robin)
    L = count(degrees) + 2 + nf
    r = A.residual(b, x).to_local_numpy()
    assert np.all(np.abs(r - (bn - y)) <= L * EPS * (np.abs(bn) + Sabs))
    om = 2.0 / 3.0
    dr = om * (bn - y) / D
    xo = V.empty()
    nrm, dot = A.jacobi_sweep(b, x, xo, om, want_norm=True, want_dot=True)
    got = xo.to_local_numpy()
    vb = L * EPS * (np.abs(xn) + om * (np.abs(bn) + Sabs) / D)
    assert np.all(np.abs(got - (xn + dr)) <= vb)
    assert abs(nrm - np.sum(dr * dr)) <= 1e-13 * np.sum(dr * dr)
    assert abs(dot - np.sum((xn + dr) * bn)) <= 1e-13 * np.sum(np.abs((xn + dr) * bn))
    q = V.empty()
    pq = A.dot_inner(x, q)
    assert np.all(np.abs(q.to_local_numpy() - y) <= L * EPS * Sabs)
    assert abs(pq - np.sum(xn * y)) <= 1e-13 * np.sum(np.abs(xn * y))
    assert A.cheby_supported
    al, be = 0.4, 0.3
    yv = V.zeros().from_numpy(yn)
    A.cheby_step(b, x, yv, al, be)
    want = xn + be * (xn - yn) + al * (bn - y) / D
    cb = L * EPS * (np.abs(xn) + be * (np.abs(xn) + np.abs(yn)) + al * (np.abs(bn) + Sabs) / D)
    assert np.all(np.abs(yv.to_local_numpy() - want) <= cb)
    # two calls give the same bits
    xo2 = V.empty()
    nrm2, dot2 = A.jacobi_sweep(b, x, xo2, om, want_norm=True, want_dot=True)
    assert nrm2 == nrm and dot2 == dot and np.array_equal(xo2.to_local_numpy(), got)


def run_all(A, V, x, b, om=2.0 / 3.0):
    xo, q = V.empty(), V.empty()
    nrm, dt = A.jacobi_sweep(b, x, xo, om, want_norm=True, want_dot=True)
    pq = A.dot_inner(x, q)
    return [A.dot(x).to_local_numpy(), A.residual(b, x).to_local_numpy(), xo.to_local_numpy(), q.to_local_numpy(),
            np.array([nrm, dt, pq])]


@pytest.mark.parametrize("name", ["2d_p33_6x14", "2d_p33_6x14_aligned", "3d_p222_31x7x15"])
def test_face_free_builds(gpu, name):
    """An operator that never had a face term: the results are bitwise those of one created
    without ``robin=`` (the FACE = false builds), and it reports no face."""
    from poms_amd.matfree import MatrixFreeOperator
    V, T, robin, _, _ = case(name)
    rng = np.random.default_rng(7)
    x, b = (V.zeros().from_numpy(rng.uniform(-1, 1, V.npts)) for _ in range(2))
    plain = MatrixFreeOperator(V, T, a=a_var, c=c_var)
    for empty in ({}, None):
        A = MatrixFreeOperator(V, T, a=a_var, c=c_var, robin=empty)
        assert A.face_terms() == ()
        for u, v in zip(run_all(A, V, x, b), run_all(plain, V, x, b)):
            assert np.array_equal(u, v)
    # and one that has a face term differs on that face only
    one = MatrixFreeOperator(V, T, a=a_var, c=c_var, robin={(0, 1): 1.5})
    du = one.dot(x).to_local_numpy() - plain.dot(x).to_local_numpy()
    assert np.any(du[-1] != 0.0) and not np.any(du[:-1])


@pytest.mark.parametrize("form", ["stencil", "matfree"])
@pytest.mark.parametrize("name", ["2d_p33_6x14", "2d_p33_6x14_aligned", "3d_p321_3x4x5"])
def test_with_dirichlet_faces(gpu, form, name):
    """Robin on the axis-1 faces, Dirichlet on axis 0 lo: dot is constrain_dense(A + S) on a
    random x that is non-zero on C, and A + S again after set_dirichlet(None)."""
    from poms_amd.assembly import assemble_stencil
    from poms_amd.boundary import constrain_dense
    from poms_amd.matfree import MatrixFreeOperator
    V, T, _, A0, _ = case(name)
    nd = V.ndim
    robin = {f: beta_of(f, nd) for f in ((1, 0), (1, 1))}
    faces = [(True, False)] + [(False, False)] * (nd - 1)
    dense = A0 + dense_face_mass(T, V.pads, robin)
    make = assemble_stencil if form == "stencil" else MatrixFreeOperator
    A = make(V, T, a=a_var, c=c_var, robin=robin, dirichlet=faces)
    xn = np.random.default_rng(3).uniform(-1, 1, V.npts)
    x = V.zeros().from_numpy(xn)
    want = (constrain_dense(dense, V.npts, faces) @ xn.reshape(-1)).reshape(V.npts)
    assert maxrel(A.dot(x).to_local_numpy(), want) <= 1e-13
    A.set_dirichlet(None)
    assert maxrel(A.dot(x).to_local_numpy(), (dense @ xn.reshape(-1)).reshape(V.npts)) <= 1e-13
    # a face named in both sets: the mask wins on it
    both = [(False, False), (True, False)] + [(False, False)] * (nd - 2)
    A.set_dirichlet(both)
    want = (constrain_dense(dense, V.npts, both) @ xn.reshape(-1)).reshape(V.npts)
    assert maxrel(A.dot(x).to_local_numpy(), want) <= 1e-13


@pytest.mark.parametrize("nd,p,cells", [(2, 3, (6, 9)), (3, 2, (5, 4, 6))])
def test_kronecker_form(gpu, nd, p, cells):
    """KronOperator.laplace(robin=) with constant β against the stored stencil with the same β."""
    from poms_amd.assembly import assemble_stencil
    from poms_amd.splines import assemble_1d, make_open_knots
    from poms_amd.stencil import KronOperator, StencilVectorSpace
    T = [make_open_knots(p, N + p) for N in cells]
    V = StencilVectorSpace([N + p for N in cells], [p] * nd)
    robin = {f: 0.5 + 0.75 * k for k, f in enumerate(all_faces(nd))}
    MK = [assemble_1d(t, p, canonical=False) for t in T]
    Ak = KronOperator.laplace(V, [m for m, _ in MK], [k for _, k in MK], robin=robin)
    As = assemble_stencil(V, T, robin=robin)
    assert Ak.face_terms() == tuple(robin)
    x = V.zeros().from_numpy(np.random.default_rng(4).uniform(-1, 1, V.npts))
    assert maxrel(Ak.dot(x).to_local_numpy(), As.dot(x).to_local_numpy()) <= 1e-13
    with pytest.raises(ValueError, match="robin"):
        KronOperator.laplace(V, [m for m, _ in MK], [k for _, k in MK], robin={(0, 0): lambda *X: 1.0 + X[0]})


def kron_dense(Ps):
    return functools.reduce(np.kron, Ps)


def test_galerkin_hierarchy(gpu):
    """Every coarse operator of GalerkinVCycle(A + S, P) is the dense P^T (A + S) P to 1e-12."""
    from poms_amd.assembly import assemble_stencil
    from poms_amd.mg import GalerkinVCycle, uniform_hierarchy
    p, nd = 2, 2
    cells, knots, P1, V = uniform_hierarchy(p, 16, 4, nd)
    T = [knots[0]] * nd
    robin = {f: beta_of(f, nd) for f in all_faces(nd)}
    A = assemble_stencil(V, T, a=a_var, c=c_var, robin=robin)
    dense = assemble_stencil(V, T, a=a_var, c=c_var).toarray() + dense_face_mass(T, [p] * nd, robin)
    mg = GalerkinVCycle(A, [[P1l] * nd for P1l in P1])
    assert mg.nlevels == 3
    for l, P1l in enumerate(P1):
        Pd = kron_dense([P1l] * nd)
        dense = Pd.T @ dense @ Pd
        got = mg.ops[l + 1].toarray() if l + 1 < len(mg.ops) else mg.Ac
        err = np.max(np.abs(got - dense)) / np.max(np.abs(dense))
        print(f"level {l + 1}: {err:.2e}")
        assert err <= 1e-12
    assert np.max(np.abs(mg.Ac - dense)) <= 1e-12 * np.max(np.abs(dense))


@pytest.mark.parametrize("nd", [2, 3])
def test_rediscretised_level_one(gpu, nd):
    """MatrixFreeVCycle.uniform(robin={...: 2.0}): constant β (and a = c = 1) is integrated exactly
    on both levels, so the rediscretised level-1 operator is the Galerkin one to 1e-12."""
    from poms_amd.matfree import MatrixFreeVCycle
    p = 2
    robin = {f: 2.0 for f in all_faces(nd)[1:]}
    mg = MatrixFreeVCycle.uniform(p, 8, 4, nd, robin=robin)
    A0 = mg.ops[0].assemble().toarray()
    assert mg.ops[0].face_terms() == tuple(robin) and mg.ops[1].face_terms() == tuple(robin)
    Pd = kron_dense([mg.P1[0]] * nd)
    want = Pd.T @ A0 @ Pd
    got = mg.ops[1].toarray()
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print(f"{nd}D: rediscretised level 1 against the Galerkin product {err:.2e}")
    assert err <= 1e-12
    # and the faces matter: without them level 1 is a different matrix
    plain = MatrixFreeVCycle.uniform(p, 8, 4, nd).ops[1].toarray()
    assert np.max(np.abs(plain - want)) >= 1e-3 * np.max(np.abs(want))


def test_refusals(gpu):
    import ctypes as C

    import torch

    from poms_amd import _lib
    from poms_amd.assembly import assemble_stencil
    from poms_amd.boundary import RobinBC, add_face_term
    from poms_amd.dist import SlabDistribution
    from poms_amd.matfree import MatrixFreeOperator
    from poms_amd.splines import assemble_1d, uniform_knots
    from poms_amd.stencil import KronOperator, StencilVectorSpace
    p, N = 2, 6
    T = uniform_knots(p, N)
    n = N + p
    V = StencilVectorSpace([n, n], [p, p])
    As = assemble_stencil(V, [T, T])
    Am = MatrixFreeOperator(V, [T, T])
    S = np.zeros((1, n, 1, 2 * p + 1))
    ptr = S.ctypes.data_as(C.c_void_p)
    m, half = (C.c_int64 * 2)(1, n), (C.c_int * 2)(0, p)
    add = _lib.lib.poms_op_add_face_term
    err = lambda: _lib.lib.poms_last_error()
    for A in (As, Am):
        h = A._h
        for args, word in (((h, 0, 0, None, m, half), b"null"), ((h, 0, 0, ptr, None, half), b"null"),
                           ((h, 0, 0, ptr, m, None), b"null"), ((h, 2, 0, ptr, m, half), b"axis"),
                           ((h, -1, 0, ptr, m, half), b"axis"), ((h, 0, 2, ptr, m, half), b"side"),
                           ((h, 0, 0, ptr, (C.c_int64 * 2)(1, n + 1), half), b"extents"),
                           ((h, 0, 0, ptr, (C.c_int64 * 2)(n, 1), half), b"extents"),
                           ((h, 0, 0, ptr, m, (C.c_int * 2)(0, p + 1)), b"half"),
                           ((h, 0, 0, ptr, m, (C.c_int * 2)(p, p)), b"half")):
            assert add(*args) != 0
            assert b"poms_op_add_face_term" in err() and word in err(), (args[1:3], err())
        # during a stream capture: a global-mode capture makes the legacy stream's query fail,
        # which both set-up calls read as a capture in progress (poms_op_set_dirichlet goes
        # first: it launches nothing, so a capture it did not see would take no harm)
        # (an empty global-mode capture on a blocking stream of the HIP runtime the library is
        # linked to, begun and ended here: nothing is launched into it)
        torch.cuda.synchronize()
        hip = _lib.lib
        st, graph = C.c_void_p(), C.c_void_p()
        hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
        hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        hip.hipGraphDestroy.argtypes = hip.hipStreamDestroy.argtypes = [C.c_void_p]
        assert hip.hipStreamCreate(C.byref(st)) == 0
        assert hip.hipStreamBeginCapture(st, 0) == 0
        rc = msg = None
        seen = _lib.lib.poms_op_set_dirichlet(h, 1) != 0 and b"capture" in err()
        if seen:   # (never launch into a capture that the calls cannot see)
            rc = add(h, 0, 0, ptr, m, half)
            msg = err()
        hip.hipStreamEndCapture(st, C.byref(graph))   # (asking the legacy stream may have ended the capture)
        if graph.value:
            hip.hipGraphDestroy(graph)
        hip.hipStreamDestroy(st)
        hip.hipGetLastError()
        assert seen, "a global-mode capture on a blocking stream was not seen by poms_op_set_dirichlet"
        assert rc != 0 and b"poms_op_add_face_term" in msg and b"capture" in msg
        _lib.call("poms_op_set_dirichlet", h, 0)
        out = C.c_int(-1)
        _lib.call("poms_op_face_terms", h, C.byref(out))
        assert out.value == 0 and A.face_terms() == ()
    # Kronecker forms
    M, K = assemble_1d(T, p)
    Ak = KronOperator.laplace(V, [M, M], [K, K])
    assert add(Ak._h, 0, 0, ptr, m, half) != 0
    assert b"poms_op_add_face_term" in err() and b"factors" in err()
    with pytest.raises(NotImplementedError, match="factors"):
        add_face_term(Ak, (0, 0), S)
    with pytest.raises(ValueError, match="robin"):
        KronOperator.laplace(V, [M, M], [K, K], robin={(0, 0): lambda y: 1.0 + y})
    # slabs: the Python classes refuse the space, the C entry point the handle
    Vs = StencilVectorSpace([8, 8, 8], [2, 2, 2], dist=SlabDistribution(8, 0, 2))
    T8 = uniform_knots(2, 6)
    for call in (lambda: RobinBC(Vs, [T8] * 3, {(0, 0): 1.0}),
                 lambda: assemble_stencil(Vs, [T8] * 3, robin={(1, 0): 1.0}),
                 lambda: KronOperator.laplace(Vs, [M] * 3, [K] * 3, robin={(1, 0): 1.0})):
        with pytest.raises(NotImplementedError, match="distributed"):
            call()
    lay = _lib.Layout.make((4, 5, 6), (1, 1, 1))
    data = np.zeros((6, 7, 8, 3, 3, 3))
    hs = C.c_void_p()
    _lib.call("poms_op_create_stencil", V.ctx, 3, C.byref(lay), data.ctypes.data_as(C.c_void_p), 2, 8, C.byref(hs))
    try:
        S3 = np.zeros((5, 6, 3, 3))
        assert add(hs, 0, 0, S3.ctypes.data_as(C.c_void_p), (C.c_int64 * 2)(5, 6), (C.c_int * 2)(1, 1)) != 0
        assert b"poms_op_add_face_term" in err() and b"slab" in err()
    finally:
        _lib.lib.poms_op_destroy(hs)
    # a Cart block: a layout whose ghosts of axes 1 and 2 hold data
    layc = _lib.Layout.make(V.n3, V.p3, 0, _lib.LAYOUT_GHOST_DATA)
    datac = np.zeros((n + 2 * p, n + 2 * p, 2 * p + 1, 2 * p + 1))
    hc = C.c_void_p()
    _lib.call("poms_op_create_stencil", V.ctx, 2, C.byref(layc), datac.ctypes.data_as(C.c_void_p), 0, 1, C.byref(hc))
    try:
        assert add(hc, 0, 0, ptr, m, half) != 0
        assert b"poms_op_add_face_term" in err() and b"Cart" in err()
        out = C.c_int(-1)
        _lib.call("poms_op_face_terms", hc, C.byref(out))
        assert out.value == 0
    finally:
        _lib.lib.poms_op_destroy(hc)
    # spellings
    for bad in ({(2, 0): 1.0}, {(0, 3): 1.0}, [(0, 0)]):
        with pytest.raises(ValueError, match="robin"):
            assemble_stencil(V, [T, T], robin=bad)
        with pytest.raises(ValueError, match="robin"):
            MatrixFreeOperator(V, [T, T], robin=bad)
    # adding twice adds twice
    rb = RobinBC(V, [T, T], {(1, 1): 1.25})
    once = rb.apply(assemble_stencil(V, [T, T])).toarray()
    twice = rb.apply(rb.apply(assemble_stencil(V, [T, T]))).toarray()
    base = As.toarray()
    assert maxrel(twice - base, 2.0 * (once - base)) <= 1e-14
    # a host edit uploads plain coefficients: they keep the terms, no face is named any more
    B = rb.apply(assemble_stencil(V, [T, T]))
    assert B.face_terms() == ((1, 1),) and [f for f, _ in B._face_terms] == [(1, 1)]
    B[0, 0, 0, 0] = B[0, 0, 0, 0] + 1.0
    want = once.copy()
    want[0, 0] += 1.0
    assert np.array_equal(B.toarray(), want) and B.face_terms() == () and B._face_terms == []
    Am2 = rb.apply(rb.apply(MatrixFreeOperator(V, [T, T])))
    x = V.zeros().from_numpy(np.random.default_rng(0).uniform(-1, 1, V.npts))
    assert maxrel(Am2.dot(x).to_local_numpy(), (twice @ x.to_local_numpy().reshape(-1)).reshape(V.npts)) <= 1e-13
    assert maxrel(Am2.diagonal().cpu().numpy(), np.diag(twice).reshape(V.npts)) <= 1e-13


def test_measure_and_face_points(gpu):
    """RobinBC.face_points and .measure: the sum of w ds is the length of every edge of the
    quarter annulus (π on r = 2, π/2 on r = 1, 1 on the straight edges; the integrands are
    constants, 1e-14 relative) and the area of every face of a sheared box; without a mapping
    it is the Gauss weights; the mass and the load of β = g = 1 sum to the same measure."""
    from poms_amd.geometry import MappedDomain, Mapping
    from poms_amd.boundary import RobinBC
    from poms_amd.splines import uniform_knots
    from poms_amd.stencil import StencilVectorSpace
    p, N = 2, 8
    T = [uniform_knots(p, N)] * 2
    V = StencilVectorSpace([N + p] * 2, [p] * 2, align=True)
    rb = MappedDomain(V, T, quarter_annulus()).robin({f: 1.0 for f in all_faces(2)})
    for face, want in (((0, 1), np.pi), ((0, 0), np.pi / 2), ((1, 0), 1.0), ((1, 1), 1.0)):
        pts = rb.face_points(face)
        assert [len(q) for q in pts] == [1 if d == face[0] else N * (p + 1) for d in range(2)]
        assert pts[face[0]][0] == float(face[1])
        assert np.allclose(pts[1 - face[0]], gauss(T[0], p + 1)[0], rtol=1e-15, atol=0.0)
        ms = rb.measure(face)
        assert ms.is_cuda and tuple(ms.shape) == (N * (p + 1),)
        assert abs(float(ms.sum().item()) - want) <= 1e-14 * want
        # partition of unity: the entries of the mass, and of the load of g = 1, sum to the length
        assert abs(rb.mass(face).sum() - want) <= 1e-13 * want
        assert abs(float(rb.load_vector({face: 1.0}).to_local_numpy().sum()) - want) <= 1e-13 * want
    flat = RobinBC(V, T, {})
    assert np.allclose(flat.measure((1, 0)).cpu().numpy(), gauss(T[0], p + 1)[1], rtol=1e-15, atol=0.0)
    # 3D: F = (x + 0.3 y, y, 2 z): faces of area 2 sqrt(1.09), 2, 1
    F = lambda x, y, z: [x + 0.3 * y, y, 2.0 * z]
    jac = lambda x, y, z: [[1.0, 0.3, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 2.0]]
    T3 = [uniform_knots(p, 3)] * 3
    V3 = StencilVectorSpace([3 + p] * 3, [p] * 3)
    rb3 = RobinBC(V3, T3, {}, mapping=Mapping(F, jac, ndim=3))
    for axis, want in ((0, 2.0 * np.sqrt(1.09)), (1, 2.0), (2, 1.0)):
        for side in (0, 1):
            ms = rb3.measure((axis, side))
            assert tuple(ms.shape) == (3 * (p + 1),) * 2
            assert abs(float(ms.sum().item()) - want) <= 1e-14 * want
            assert abs(rb3.mass((axis, side), beta=1.0).sum() - want) <= 1e-13 * want
            assert abs(float(rb3.load_vector({(axis, side): 1.0}).to_local_numpy().sum()) - want) <= 1e-13 * want


# ---- solved problems -----------------------------------------------------------------------
def load_nd(T, degrees, f, weight=None):
    """b[i] = sum_q w f φ_i at p+1 Gauss points per element (times ``weight`` on the grid)."""
    gr = [gauss(t, p + 1) for t, p in zip(T, degrees)]
    G = np.meshgrid(*[g[0] for g in gr], indexing="ij")
    v = f(*G) * functools.reduce(np.multiply.outer, [g[1] for g in gr])
    if weight is not None:
        v = v * weight(*G)
    for d, (t, p, g) in enumerate(zip(T, degrees, gr)):
        v = np.moveaxis(np.tensordot(colloc(t, p, g[0]).T, v, axes=(1, d)), 0, d)
    return v


def kron_sum_dense(T, degrees):
    """-Δ + 1 as the dense Kronecker sum of assemble_1d's factors."""
    from poms_amd.splines import assemble_1d, band_to_dense
    MK = [[band_to_dense(F) for F in assemble_1d(t, p)] for t, p in zip(T, degrees)]
    nd = len(T)
    A = kron_dense([m for m, _ in MK])
    for d in range(nd):
        A = A + kron_dense([MK[e][1] if e == d else MK[e][0] for e in range(nd)])
    return A


def greville_lift(T, degrees, faces_lo0, u):
    """Coefficients of the Greville interpolant of u on the face x_0 = 0 (zero elsewhere), 2D."""
    from poms_amd.splines import greville
    shape = tuple(len(t) - p - 1 for t, p in zip(T, degrees))
    xg = np.zeros(shape)
    if faces_lo0:
        gv = greville(T[1], degrees[1])
        xg[0, :] = np.linalg.solve(colloc(T[1], degrees[1], gv), u(np.zeros_like(gv), gv))
    return xg


def restate(A, b, xg, fixed):
    """Solve on the free rows; returns the full coefficients and cond(A_ff)."""
    fr = ~fixed.reshape(-1)
    Aff = A[np.ix_(fr, fr)]
    rhs = (b.reshape(-1) - A @ xg.reshape(-1))[fr]
    x = xg.reshape(-1).copy()
    x[fr] += np.linalg.solve(Aff, rhs)
    return x.reshape(b.shape), float(np.linalg.cond(Aff))


U2 = lambda lib: (lambda x, y: lib.exp(x) * lib.cos(y))
SQUARE_ROBIN = {(1, 0): 2.0, (1, 1): lambda x: 1.0 + x}
SQUARE_G = {(0, 1): lambda y: np.e * np.cos(y),
            (1, 0): lambda x: 2.0 * np.exp(x),
            (1, 1): lambda x: -np.exp(x) * np.sin(1.0) + (1.0 + x) * np.exp(x) * np.cos(1.0)}
SQUARE_DIR = [(True, False), (False, False)]


@functools.lru_cache(maxsize=None)
def square_restatement(p, N):
    from poms_amd.splines import uniform_knots
    T, deg = [uniform_knots(p, N)] * 2, [p, p]
    A = kron_sum_dense(T, deg) + dense_face_mass(T, deg, SQUARE_ROBIN)
    b = load_nd(T, deg, U2(np)) + dense_face_load(T, deg, SQUARE_G)
    xg = greville_lift(T, deg, True, U2(np))
    fixed = np.zeros(b.shape, dtype=bool)
    fixed[0, :] = True
    return restate(A, b, xg, fixed)


@pytest.mark.parametrize("matrix_free", [False, True])
@pytest.mark.parametrize("p", [1, 2, 3])
def test_solved_problem_on_the_unit_square(gpu, p, matrix_free):
    """-Δu + u = f, u = e^x cos y (f = u): Dirichlet on x = 0 (Greville lift), the flux
    e cos y on x = 1, Robin β = 2 on y = 0 and β = 1 + x on y = 1.  pcg preconditioned by the
    Chebyshev V-cycle to ||r|| <= 1e-12 ||b||; the coefficients agree with the dense CPU
    restatement within cond(A_ff) 1e-12, and err(8) / err(16) >= 0.9 2^(p+1)."""
    import torch

    from poms_amd.boundary import DirichletBC, RobinBC
    from poms_amd.field import assemble_rhs, l2_error
    from poms_amd.matfree import MatrixFreeVCycle
    from poms_amd.mg import GalerkinVCycle
    from poms_amd.solvers import pcg
    errs = {}
    for N in (8, 16):
        cls = MatrixFreeVCycle if matrix_free else GalerkinVCycle
        mg = cls.uniform(p, N, 4, 2, smoother="chebyshev", dirichlet=SQUARE_DIR, robin=SQUARE_ROBIN)
        V, T = mg.space, [mg.knots[0]] * 2
        assert mg.A.face_terms() == tuple(SQUARE_ROBIN)
        b = RobinBC(V, T, SQUARE_ROBIN).load_vector(SQUARE_G, out=assemble_rhs(V, T, U2(torch)))
        bc = DirichletBC(V, T, SQUARE_DIR)
        xg = bc.lift(U2(np))
        b = bc.homogenize(mg.A, b, xg)
        nb = np.sqrt(b.dot(b))
        x, info = pcg(mg.A, mg.preconditioner(), b, tol=1e-24 * nb, maxiter=200)
        r = mg.A.residual(b, x)
        res = np.sqrt(r.dot(r)) / nb
        xc, cond = square_restatement(p, N)
        got = (xg + x).to_local_numpy()
        dif = np.linalg.norm(got - xc) / np.linalg.norm(xc)
        errs[N] = l2_error(V, T, xg + x, U2(torch))
        print(f"unit square p={p} N={N} {'matrix-free' if matrix_free else 'stored'}: {info['niter']} iterations, "
              f"||r||/||b|| {res:.2e}, cond {cond:.1f}, |x - x_cpu|/|x_cpu| {dif:.2e}, L2 error {errs[N]:.3e}")
        assert info["success"] and res <= 1e-12, info
        assert dif <= cond * 1e-12
    print(f"   err(8)/err(16) = {errs[8] / errs[16]:.2f}")
    assert errs[8] / errs[16] >= 0.9 * 2 ** (p + 1)


def test_solved_problem_in_3d(gpu):
    """-Δu + u = u on the unit cube, u = e^x cos y (1 + z) (harmonic), degrees (2, 2, 2), 4 cells
    per axis, Robin on all six faces (β constant on four, variable on two): the stored and the
    matrix-free coefficients agree with the dense restatement within cond(A) 1e-12."""
    import torch

    from poms_amd.assembly import assemble_stencil
    from poms_amd.boundary import RobinBC
    from poms_amd.field import assemble_rhs
    from poms_amd.matfree import MatrixFreeOperator
    from poms_amd.solvers import damped_jacobi, pcg
    from poms_amd.splines import uniform_knots
    from poms_amd.stencil import StencilVectorSpace
    p, N = 2, 4
    T, deg = [uniform_knots(p, N)] * 3, [p] * 3
    u = lambda lib: (lambda x, y, z: lib.exp(x) * lib.cos(y) * (1.0 + z))
    un = u(np)
    beta = {(0, 0): 1.0, (0, 1): 2.0, (1, 0): 0.5, (1, 1): lambda x, z: 1.0 + x * z, (2, 0): 1.5,
            (2, 1): lambda x, y: 2.0 + np.sin(x + y)}
    bval = lambda f, *X: beta[f](*X) if callable(beta[f]) else beta[f]
    # g = d_n u + β u on every face
    g = {(0, 0): lambda y, z: (-1.0 + bval((0, 0))) * un(0.0, y, z),
         (0, 1): lambda y, z: (1.0 + bval((0, 1))) * un(1.0, y, z),
         (1, 0): lambda x, z: bval((1, 0)) * un(x, 0.0, z),                      # d_y u = 0 on y = 0
         (1, 1): lambda x, z: -np.exp(x) * np.sin(1.0) * (1.0 + z) + bval((1, 1), x, z) * un(x, 1.0, z),
         (2, 0): lambda x, y: -np.exp(x) * np.cos(y) + bval((2, 0)) * un(x, y, 0.0),
         (2, 1): lambda x, y: np.exp(x) * np.cos(y) + bval((2, 1), x, y) * un(x, y, 1.0)}
    A = kron_sum_dense(T, deg) + dense_face_mass(T, deg, beta)
    bn = load_nd(T, deg, un) + dense_face_load(T, deg, g)
    xc, cond = restate(A, bn, np.zeros_like(bn), np.zeros(bn.shape, dtype=bool))
    V = StencilVectorSpace([N + p] * 3, deg)
    rb = RobinBC(V, T, beta)
    b = rb.load_vector(g, out=assemble_rhs(V, T, u(torch)))
    assert np.linalg.norm(b.to_local_numpy() - bn) <= 1e-13 * np.linalg.norm(bn)
    nb = np.sqrt(b.dot(b))
    for name, Aop in (("stored", assemble_stencil(V, T, robin=rb)), ("matrix-free", MatrixFreeOperator(V, T, robin=rb))):
        x, info = pcg(Aop, damped_jacobi, b, tol=1e-24 * nb, maxiter=300)
        r = Aop.residual(b, x)
        res = np.sqrt(r.dot(r)) / nb
        dif = np.linalg.norm(x.to_local_numpy() - xc) / np.linalg.norm(xc)
        print(f"3D {name}: {info['niter']} iterations, ||r||/||b|| {res:.2e}, cond {cond:.1f}, "
              f"|x - x_cpu|/|x_cpu| {dif:.2e}")
        assert info["success"] and res <= 1e-12, info
        assert dif <= cond * 1e-12


def quarter_annulus():
    """(s, t) -> (r cos θ, r sin θ), r = 1 + s, θ = π t / 2."""
    from poms_amd.geometry import Mapping
    h = np.pi / 2
    F = lambda s, t: [(1 + s) * np.cos(h * t), (1 + s) * np.sin(h * t)]
    jac = lambda s, t: [[np.cos(h * t), -h * (1 + s) * np.sin(h * t)], [np.sin(h * t), h * (1 + s) * np.cos(h * t)]]
    return Mapping(F, jac, ndim=2)


ANNULUS_U = lambda x, y: x * x - y * y
# d_r u = 2 u / r: the flux u on r = 2; on r = 1 the outward normal is -r, so g = -2 u + β u = -u
ANNULUS_ROBIN = {(0, 0): 1.0}
ANNULUS_G = {(0, 0): lambda x, y: -ANNULUS_U(x, y), (0, 1): ANNULUS_U}
ANNULUS_DIR = [(False, False), (True, True)]


def annulus_restatement(p, N):
    """The case on the CPU, dense: (coefficients, physical L2 error, cond of the free block)."""
    from poms_amd.splines import greville, uniform_knots
    mp = quarter_annulus()
    T, deg = [uniform_knots(p, N)] * 2, [p, p]
    gr = [gauss(t, p + 1) for t in T]
    G = np.meshgrid(*[g[0] for g in gr], indexing="ij")
    w = np.multiply.outer(gr[0][1], gr[1][1])
    J = mp.jac(*G)
    det = J[0][0] * J[1][1] - J[0][1] * J[1][0]
    Ji = [[J[1][1] / det, -J[0][1] / det], [-J[1][0] / det, J[0][0] / det]]   # J^-1
    Gt = [[(Ji[i][0] * Ji[j][0] + Ji[i][1] * Ji[j][1]) * det for j in range(2)] for i in range(2)]
    B = [colloc(t, p, g[0]) for t, g in zip(T, gr)]
    D = [colloc(t, p, g[0], 1) for t, g in zip(T, gr)]
    full = lambda a, b: np.einsum("qi,rj->qrij", a, b).reshape(a.shape[0] * b.shape[0], -1)
    B0, D0, D1 = full(B[0], B[1]), full(D[0], B[1]), full(B[0], D[1])
    wv = lambda f: (w * f).reshape(-1, 1)
    A = B0.T @ (wv(det) * B0)
    for i, Di in enumerate((D0, D1)):
        for j, Dj in enumerate((D0, D1)):
            A += Di.T @ (wv(Gt[i][j]) * Dj)
    A += dense_face_mass(T, deg, ANNULUS_ROBIN, mp)
    X = mp.F(*G)
    b = (B0.T @ (w * det * ANNULUS_U(*X)).reshape(-1)).reshape(N + p, N + p) + dense_face_load(T, deg, ANNULUS_G, mp)
    # Dirichlet on t = 0 and t = 1: the Greville interpolant of u along s
    gv = greville(T[0], p)
    Ci = colloc(T[0], p, gv)
    xg = np.zeros(b.shape)
    fixed = np.zeros(b.shape, dtype=bool)
    for idx, t in ((0, 0.0), (N + p - 1, 1.0)):
        xg[:, idx] = np.linalg.solve(Ci, ANNULUS_U(*mp.F(gv, np.full_like(gv, t))))
        fixed[:, idx] = True
    x, cond = restate(A, b, xg, fixed)
    e = (B0 @ x.reshape(-1)).reshape(w.shape) - ANNULUS_U(*X)
    return x, float(np.sqrt(np.sum(w * det * e * e))), cond


def test_solved_problem_on_a_quarter_annulus(gpu):
    """-Δu + u = f on 1 <= r <= 2, 0 <= θ <= π/2, u = x^2 - y^2 (f = u), p = 2: Dirichlet on the
    straight edges, flux data on r = 2, Robin β = 1 on r = 1.  pcg to 1e-12; the stored and the
    matrix-free L2 errors agree to 1e-9 relative and err(8) / err(16) >= 0.9 2^3 (the CPU
    restatement of this case, annulus_restatement, gives 8.831e-4 / 1.061e-4 = 8.32, above
    that factor, so the factor stands; its free block has condition 74 and 267)."""
    from poms_amd.geometry import MappedDomain
    from poms_amd.solvers import damped_jacobi, pcg
    from poms_amd.splines import uniform_knots
    from poms_amd.stencil import StencilVectorSpace
    p = 2
    errs = {}
    for N in (8, 16):
        T = [uniform_knots(p, N)] * 2
        V = StencilVectorSpace([N + p] * 2, [p] * 2, align=True)
        dom = MappedDomain(V, T, quarter_annulus())
        xc, ec, cond = annulus_restatement(p, N)
        for mf in (False, True):
            # (a dict or the domain's RobinBC: both spellings reach the same operator)
            A = dom.operator(matrix_free=mf, dirichlet=ANNULUS_DIR,
                             robin=dom.robin(ANNULUS_ROBIN) if mf else ANNULUS_ROBIN)
            bc = dom.dirichlet(ANNULUS_DIR)
            xg = bc.lift(ANNULUS_U)
            b = bc.homogenize(A, dom.boundary_load(ANNULUS_G, out=dom.load_vector(ANNULUS_U)), xg)
            nb = np.sqrt(b.dot(b))
            x, info = pcg(A, damped_jacobi, b, tol=1e-24 * nb, maxiter=1000)
            r = A.residual(b, x)
            res = np.sqrt(r.dot(r)) / nb
            errs[N, mf] = dom.l2_error(xg + x, ANNULUS_U)
            dif = np.linalg.norm((xg + x).to_local_numpy() - xc) / np.linalg.norm(xc)
            print(f"quarter annulus p=2 N={N} {'matrix-free' if mf else 'stored'}: {info['niter']} iterations, "
                  f"||r||/||b|| {res:.2e}, L2 error {errs[N, mf]:.4e} (CPU {ec:.4e}), |x - x_cpu|/|x_cpu| {dif:.2e}, "
                  f"cond {cond:.1f}")
            assert info["success"] and res <= 1e-12, info
            assert dif <= cond * 1e-12
        assert abs(errs[N, True] - errs[N, False]) <= 1e-9 * errs[N, False]
    for mf in (False, True):
        print(f"   err(8)/err(16) = {errs[8, mf] / errs[16, mf]:.2f}")
        assert errs[8, mf] / errs[16, mf] >= 0.9 * 2 ** (p + 1)
