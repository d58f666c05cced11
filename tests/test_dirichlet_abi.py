"""Dirichlet boundary conditions without a device: the two C entry points are declared,
bound and exported and refuse null arguments with a message; the face spellings, the
constrained 1D factors, the unit-row check on the prolongations and the host part of the
lift are checked against dense NumPy."""
import ctypes as C
import itertools

import numpy as np
import pytest

from poms_amd import _lib
from poms_amd.boundary import (check_unit_rows, collocation_1d, constrain_dense, constrain_prolongation,
                               constrained_mask, faces_mask, lift_host, mask_faces, normalize_faces)
from poms_amd.splines import (assemble_1d, band_to_dense, constrain_1d, dense_to_band, greville, uniform_knots)

SIDES = list(itertools.product((False, True), repeat=2))


def test_dirichlet_symbols_are_declared_bound_and_exported():
    for name, nargs in (("poms_op_set_dirichlet", 2), ("poms_op_get_dirichlet", 2)):
        assert name in _lib.header_symbols()
        assert name in _lib._SIGS
        fn = getattr(_lib.lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs
    assert _lib.lib.poms_abi_version() >= 8


def test_dirichlet_entry_points_reject_null_arguments():
    assert _lib.lib.poms_op_set_dirichlet(None, 3) != 0
    msg = _lib.lib.poms_last_error().lower()
    assert b"null" in msg and b"poms_op_set_dirichlet" in msg
    out = C.c_int(-7)
    assert _lib.lib.poms_op_get_dirichlet(None, C.byref(out)) != 0
    msg = _lib.lib.poms_last_error().lower()
    assert b"null" in msg and b"poms_op_get_dirichlet" in msg
    assert out.value == -7
    assert _lib.lib.poms_op_get_dirichlet(None, None) != 0
    with pytest.raises(_lib.PomsError, match="null"):
        _lib.call("poms_op_set_dirichlet", None, 0)


def test_dirichlet_name_is_exported_lazily():
    import poms_amd
    assert "DirichletBC" in poms_amd.__all__
    assert poms_amd.DirichletBC.__name__ == "DirichletBC"


def test_face_spellings():
    for nd in (1, 2, 3):
        for none in (None, False, [(False, False)] * nd):
            assert normalize_faces(none, nd) is None and faces_mask(none, nd) == 0
        for every in (True, "all", [(True, True)] * nd, np.ones((nd, 2), dtype=bool)):
            assert normalize_faces(every, nd) == ((True, True),) * nd
            assert faces_mask(every, nd) == (1 << (2 * nd)) - 1
    # bit 2 d + side
    assert faces_mask([(True, False), (False, False)], 2) == 1
    assert faces_mask([(False, True), (False, False)], 2) == 2
    assert faces_mask([(False, False), (True, False)], 2) == 4
    assert faces_mask([(False, False), (False, False), (False, True)], 3) == 32
    assert faces_mask([(True, False), (True, True), (False, False)], 3) == 1 + 4 + 8
    assert faces_mask([[1, 0], [0, 1]], 2) == 1 + 8
    for nd in (2, 3):
        for m in range(1 << (2 * nd)):
            assert faces_mask(mask_faces(m, nd), nd) == m
    for bad in ([(True, True)], [(True, True)] * 3, [(True, True), (True,)], [(True, True), True],
                [(True, True), (True, False, True)], "every", "", [(True, "yes"), (True, True)], 5,
                [(2, 0), (0, 0)]):
        with pytest.raises(ValueError, match="dirichlet"):
            normalize_faces(bad, 2)


@pytest.mark.parametrize("p", [1, 2, 3])
def test_constrain_1d_against_dense(p):
    rng = np.random.default_rng(p)
    for n in (p + 1, 9):
        F = dense_to_band(rng.uniform(0.5, 1.5, (n, n)), p)   # a full (unsymmetric) band
        Fd = band_to_dense(F)
        for lo, hi in SIDES:
            pi = np.ones(n)
            if lo:
                pi[0] = 0.0
            if hi:
                pi[-1] = 0.0
            want = pi[:, None] * Fd * pi[None, :] + np.diag((1.0 - pi) * np.diag(Fd))
            got = constrain_1d(F, lo, hi)
            assert got.shape == F.shape
            assert np.array_equal(band_to_dense(got), want)
            assert np.array_equal(constrain_dense(Fd, (n,), [(lo, hi)]), want)
        assert np.array_equal(F, dense_to_band(Fd, p))   # the input is not changed
    M, K = assemble_1d(uniform_knots(p, 6), p)
    Mt = band_to_dense(constrain_1d(M, True, True))
    assert np.array_equal(Mt[1:-1, 1:-1], band_to_dense(M)[1:-1, 1:-1])
    assert np.all(np.linalg.eigvalsh(Mt) > 0)


def test_constrained_mask_and_dense_constraint():
    m = constrained_mask((3, 4), [(True, False), (True, True)])
    want = np.zeros((3, 4), dtype=bool)
    want[0, :] = want[:, 0] = want[:, -1] = True
    assert np.array_equal(m, want)
    assert not constrained_mask((3, 4), None).any()
    rng = np.random.default_rng(0)
    A = rng.uniform(-1, 1, (12, 12))
    c = want.reshape(-1)
    AD = constrain_dense(A, (3, 4), [(True, False), (True, True)])
    assert np.array_equal(AD[np.ix_(~c, ~c)], A[np.ix_(~c, ~c)])
    assert not AD[np.ix_(~c, c)].any() and not AD[np.ix_(c, ~c)].any()
    assert np.array_equal(AD[np.ix_(c, c)], np.diag(np.diag(A)[c]))


@pytest.mark.parametrize("p", [2, 3])
def test_unit_row_check_on_the_prolongations(p):
    from poms_amd.mg import two_level_setup_1d
    P1 = two_level_setup_1d(p, uniform_knots(p, 8), uniform_knots(p, 4))[2]
    e0 = np.zeros(P1.shape[1])
    e0[0] = 1.0
    assert np.array_equal(P1[0], e0) and np.array_equal(P1[-1], e0[::-1])
    check_unit_rows([P1, P1], "all")
    check_unit_rows([P1, P1], None)
    bad = P1.copy()
    bad[0, 1] = 0.25
    with pytest.raises(ValueError, match="unit vector"):
        check_unit_rows([P1, bad], "all")
    with pytest.raises(ValueError, match="unit vector"):
        check_unit_rows([bad, P1], [(True, False), (False, False)])
    check_unit_rows([bad, P1], [(False, True), (True, True)])   # the bad side is not constrained
    bad_hi = P1.copy()
    bad_hi[-1, -2] = 1e-3
    with pytest.raises(ValueError, match="unit vector"):
        check_unit_rows([bad_hi, P1], [(False, True), (False, False)])
    Pt = constrain_prolongation(P1, True, False)
    assert not Pt[:, 0].any() and np.array_equal(Pt[:, 1:], P1[:, 1:])
    # under the condition, Π_f P Π_c = P Π_c
    assert not constrain_prolongation(P1, True, True)[[0, -1]].any()


def _poly(coefs):
    return lambda *x: sum(c * np.prod([xi ** e for xi, e in zip(x, ex)], axis=0) for ex, c in coefs.items())


@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("nd", [2, 3])
def test_lift_reproduces_polynomials_on_every_face(p, nd):
    """g a polynomial of degree <= p per axis: the lift's face coefficients are those of g
    itself (its spline coefficients on the face), so the spline of the face coefficients
    equals g at any point of the face, to 1e-13 relative."""
    rng = np.random.default_rng(10 * p + nd)
    cells = (4, 5, 3)[:nd]
    degs = [p] * nd
    knots = [uniform_knots(p, N) for N in cells]
    coefs = {ex: rng.uniform(-1, 1) for ex in itertools.product(range(p + 1), repeat=nd)}
    g = _poly(coefs)
    X = lift_host(knots, degs, "all", g)
    shape = tuple(N + p for N in cells)
    assert X.shape == shape
    c = constrained_mask(shape, "all")
    assert not X[~c].any()
    pts = [np.linspace(0.0, 1.0, 7) for _ in range(nd)]
    for d in range(nd):
        for idx, end in ((0, 0.0), (shape[d] - 1, 1.0)):
            face = np.take(X, idx, axis=d)
            axes = [e for e in range(nd) if e != d]
            val = face
            for k, e in enumerate(axes):   # evaluate the face spline at pts
                Cm = collocation_1d(knots[e], p, pts[e])
                val = np.moveaxis(np.tensordot(Cm, val, axes=(1, k)), 0, k)
            grid = [np.array([end]) if e == d else pts[e] for e in range(nd)]
            want = np.take(g(*np.meshgrid(*grid, indexing="ij")), 0, axis=d)
            assert np.max(np.abs(val - want)) <= 1e-13 * np.max(np.abs(want))


def test_lift_faces_agree_on_shared_edges():
    p = 3
    knots = [uniform_knots(p, 5), uniform_knots(p, 4)]
    g = lambda x, y: np.exp(x) * np.cos(y)
    only = lambda d, s: [tuple(e == d and t == s for t in (0, 1)) for e in range(2)]
    a = lift_host(knots, [p, p], only(0, 0), g)      # face x = 0
    b = lift_host(knots, [p, p], only(1, 1), g)      # face y = 1
    assert abs(a[0, -1] - b[0, -1]) <= 1e-14 * abs(g(0.0, 1.0))
    assert abs(a[0, -1] - g(0.0, 1.0)) <= 1e-14
    both = lift_host(knots, [p, p], [(True, False), (False, True)], g)
    assert np.array_equal(both[0, :-1], a[0, :-1]) and np.array_equal(both[:, -1], b[:, -1])   # later faces overwrite
    # a scalar is the constant function
    assert np.allclose(lift_host(knots, [p, p], "all", 2.5)[constrained_mask((8, 7), "all")], 2.5, rtol=0, atol=1e-14)
    assert np.array_equal(greville(knots[0], p)[[0, -1]], [0.0, 1.0])
