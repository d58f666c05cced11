"""Robin and Neumann boundary conditions without a device: the two C entry points are
declared, bound and exported and refuse null arguments with a message; the constant-β
Kronecker factor against a dense ``K + β e eᵀ``; the surface measure on the quarter annulus
(constant integrands) and on a sheared box against the cross product formed in NumPy."""
import ctypes as C

import numpy as np
import pytest

from poms_amd import _lib


def test_robin_symbols_are_declared_bound_and_exported():
    for name, nargs in (("poms_op_add_face_term", 6), ("poms_op_face_terms", 2)):
        assert name in _lib.header_symbols()
        assert name in _lib._SIGS
        fn = getattr(_lib.lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs
    assert _lib.lib.poms_abi_version() >= 11


def test_robin_entry_points_reject_null_arguments():
    m, half, S = (C.c_int64 * 2)(1, 4), (C.c_int * 2)(0, 1), np.zeros(12)
    assert _lib.lib.poms_op_add_face_term(None, 0, 0, S.ctypes.data_as(C.c_void_p), m, half) != 0
    msg = _lib.lib.poms_last_error().lower()
    assert b"null" in msg and b"poms_op_add_face_term" in msg
    out = C.c_int(-7)
    assert _lib.lib.poms_op_face_terms(None, C.byref(out)) != 0
    msg = _lib.lib.poms_last_error().lower()
    assert b"null" in msg and b"poms_op_face_terms" in msg
    assert out.value == -7
    with pytest.raises(_lib.PomsError, match="null"):
        _lib.call("poms_op_face_terms", None, None)


def test_robin_name_is_exported_lazily():
    import poms_amd
    assert "RobinBC" in poms_amd.__all__
    assert poms_amd.RobinBC.__name__ == "RobinBC"


def test_robin_spellings():
    from poms_amd.boundary import normalize_robin
    assert normalize_robin(None, 2) == {} and normalize_robin({}, 3) == {}
    f = lambda x: x
    got = normalize_robin({(1, 1): f, (0, 1): 2.0, (1, 0): 3}, 2)
    assert list(got) == [(0, 1), (1, 0), (1, 1)] and got[(1, 1)] is f   # axis 0 lo, axis 0 hi, axis 1 lo, ...
    for bad in ({(2, 0): 1.0}, {(0, 2): 1.0}, {0: 1.0}, {(0, 0, 0): 1.0}, [(0, 0)], {(-1, 0): 1.0}):
        with pytest.raises(ValueError, match="robin"):
            normalize_robin(bad, 2)


@pytest.mark.parametrize("p", [1, 2, 3])
def test_robin_1d_against_dense(p):
    from poms_amd.splines import assemble_1d, band_to_dense, robin_1d, uniform_knots
    _, K = assemble_1d(uniform_knots(p, 6), p)
    Kd = band_to_dense(K)
    n = Kd.shape[0]
    for lo, hi in ((0.0, 0.0), (2.0, 0.0), (0.0, 0.75), (1.5, 3.0)):
        want = Kd.copy()
        want[0, 0] += lo
        want[n - 1, n - 1] += hi
        got = robin_1d(K, lo, hi)
        assert got.shape == K.shape
        assert np.array_equal(band_to_dense(got), want)
    assert np.array_equal(band_to_dense(K), Kd)   # the input is not changed
    # one function of degree p: the two corners are different entries of a p+1 square
    _, K1 = assemble_1d(uniform_knots(p, 1), p)
    want = band_to_dense(K1)
    want[0, 0] += 1.0
    want[-1, -1] += 2.0
    assert np.array_equal(band_to_dense(robin_1d(K1, 1.0, 2.0)), want)


def gauss(T, p, nq):
    """Gauss points and weights on the non-empty spans of T (NumPy only)."""
    xg, wg = np.polynomial.legendre.leggauss(nq)
    br = np.unique(np.asarray(T, float))
    pts = np.concatenate([a + 0.5 * (b - a) * (xg + 1.0) for a, b in zip(br[:-1], br[1:])])
    w = np.concatenate([0.5 * (b - a) * wg for a, b in zip(br[:-1], br[1:])])
    return pts, w


def quarter_annulus():
    """(s, t) -> (r cos θ, r sin θ), r = 1 + s, θ = π t / 2."""
    from poms_amd.geometry import Mapping
    h = np.pi / 2
    F = lambda s, t: [(1 + s) * np.cos(h * t), (1 + s) * np.sin(h * t)]
    jac = lambda s, t: [[np.cos(h * t), -h * (1 + s) * np.sin(h * t)], [np.sin(h * t), h * (1 + s) * np.cos(h * t)]]
    return Mapping(F, jac, ndim=2)


def test_surface_measure_on_the_quarter_annulus():
    """ds is constant on every edge (π r / 2 on the arcs, 1 on the straight edges), so the
    Gauss sums give the lengths π (r = 2), π/2 (r = 1) and 1 to 1e-14 relative."""
    from poms_amd.geometry import surface_measure
    from poms_amd.splines import uniform_knots
    mp = quarter_annulus()
    pts, w = gauss(uniform_knots(2, 8), 2, 3)
    for axis, end, want in ((0, 1.0, np.pi), (0, 0.0, np.pi / 2), (1, 0.0, 1.0), (1, 1.0, 1.0)):
        grid = [np.array([end]) if d == axis else pts for d in range(2)]
        J = mp.jacobian(grid, device="cpu")
        ds = surface_measure(J, axis)
        assert tuple(ds.shape) == tuple(len(g) for g in grid)
        tot = float((ds.numpy().reshape(-1) * w).sum())
        assert abs(tot - want) <= 1e-14 * want, (axis, end, tot)
    with pytest.raises(ValueError, match="axis"):
        surface_measure(J, 2)


def test_surface_measure_on_a_sheared_box():
    """A 3D mapping with a position-dependent shear: |∂F/∂ξ_a × ∂F/∂ξ_b| against np.cross."""
    from poms_amd.geometry import Mapping, surface_measure
    F = lambda x, y, z: [x + 0.3 * y * y + 0.2 * z, 1.5 * y + 0.1 * x * z, 2.0 * z + 0.25 * x * y]
    jac = lambda x, y, z: [[1.0, 0.6 * y, 0.2], [0.1 * z, 1.5, 0.1 * x], [0.25 * y, 0.25 * x, 2.0]]
    mp = Mapping(F, jac, ndim=3)
    rng = np.random.default_rng(3)
    for axis in range(3):
        for end in (0.0, 1.0):
            grid = [np.array([end]) if d == axis else np.sort(rng.uniform(0, 1, 4 + d)) for d in range(3)]
            J = mp.jacobian(grid, device="cpu")
            ds = surface_measure(J, axis).numpy()
            Jn = np.stack([np.stack([J[i][k].numpy() for k in range(3)], axis=-1) for i in range(3)], axis=-2)
            a, b = [k for k in range(3) if k != axis]
            want = np.linalg.norm(np.cross(Jn[..., :, a], Jn[..., :, b]), axis=-1)
            assert ds.shape == want.shape
            assert np.max(np.abs(ds - want)) <= 1e-14 * np.max(want)
