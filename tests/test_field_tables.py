"""Host tables of the spline-field kernels (no GPU): B-splines at arbitrary points, the
per-point view of the quadrature tables with the support ranges of the gather-form load
vector, and the argument checks of the C entry points that need no device."""
import ctypes as C

import numpy as np
import pytest

from poms_amd import _lib
from poms_amd.assembly import axis_tables, point_tables, quad_point_tables, support_ranges
from poms_amd.splines import basis_funs_ders, find_span, make_open_knots, uniform_knots


def _nonuniform_knots(p, breaks):
    breaks = np.asarray(breaks, dtype=float)
    return np.concatenate([np.full(p, breaks[0]), breaks, np.full(p, breaks[-1])])


# p = 3, non-uniform, the interior knot 0.45 repeated (an empty span in the middle)
T_REP = _nonuniform_knots(3, [0.0, 0.1, 0.2, 0.3, 0.45, 0.45, 0.6, 0.7, 0.85, 1.0])


@pytest.mark.parametrize("p", [1, 2, 3, 5])
def test_point_tables_partition_of_unity(p):
    T = _nonuniform_knots(p, np.linspace(0.0, 1.0, 8) ** 1.5)
    rng = np.random.default_rng(p)
    pts = np.sort(np.concatenate([[T[p], T[-1], 0.5, 0.5], rng.uniform(T[p], T[-1], 9), T[p + 1:-p - 1]]))
    t = point_tables(T, p, pts)
    assert t["basis"].shape == (pts.size, p + 1, 2) and t["first"].shape == (pts.size,)
    assert np.abs(t["basis"][:, :, 0].sum(axis=1) - 1.0).max() <= 1e-14
    scale = np.abs(t["basis"][:, :, 1]).sum(axis=1).max()
    assert np.abs(t["basis"][:, :, 1].sum(axis=1)).max() <= 1e-14 * scale
    assert t["basis"][:, :, 0].min() >= 0.0
    # every row is find_span's span and basis_funs_ders' values
    for q, x in enumerate(pts):
        s = find_span(T, p, x)
        assert t["first"][q] == s - p
        assert np.array_equal(t["basis"][q].T, basis_funs_ders(T, p, x, s, 1))
    assert np.all(np.diff(t["first"]) >= 0)


@pytest.mark.parametrize("T,p", [(uniform_knots(2, 5), 2), (T_REP, 3), (make_open_knots(1, 4), 1)])
def test_point_tables_end_points(T, p):
    n = len(T) - p - 1
    t = point_tables(T, p, [T[p], T[n]])
    assert t["first"][0] == 0                      # first span
    last = max(s for s in range(p, n) if T[s + 1] > T[s])
    assert t["first"][1] == last - p == n - 1 - p  # last non-empty span
    assert abs(t["basis"][0, 0, 0] - 1.0) <= 1e-14 and abs(t["basis"][1, p, 0] - 1.0) <= 1e-14   # interpolatory ends of open knots
    assert np.all(t["basis"][0, 1:, 0] == 0.0) and np.all(t["basis"][1, :p, 0] == 0.0)


def test_point_tables_rejects_bad_points():
    T = uniform_knots(2, 4)
    with pytest.raises(ValueError):
        point_tables(T, 2, [0.5, 0.25])
    with pytest.raises(ValueError):
        point_tables(T, 2, [-0.1, 0.5])
    with pytest.raises(ValueError):
        point_tables(T, 2, [0.5, 1.0 + 1e-9])
    with pytest.raises(ValueError):
        point_tables(T, 2, [])


@pytest.mark.parametrize("nquad", [None, 2, 6])
def test_quad_point_tables_flatten_axis_tables(nquad):
    p = 3
    a = axis_tables(T_REP, p, nquad)
    t = quad_point_tables(T_REP, p, nquad)
    nq = p + 1 if nquad is None else nquad
    assert a["nel"] == 8 and t["Q"] == 8 * nq and t["nq"] == nq
    assert np.array_equal(t["points"], a["points"].reshape(-1)) and np.all(np.diff(t["points"]) > 0)
    assert np.array_equal(t["weights"], a["weights"].reshape(-1))
    assert abs(t["weights"].sum() - 1.0) <= 1e-14
    for q in range(t["Q"]):
        e, g = divmod(q, nq)
        assert t["first"][q] == a["first"][e]
        assert np.array_equal(t["basis"][q], a["basis"][e, g])
    # the flat tables agree with the point tables at the same points
    pt = point_tables(T_REP, p, t["points"])
    assert np.array_equal(pt["first"], t["first"]) and np.array_equal(pt["basis"], t["basis"])


@pytest.mark.parametrize("nquad", [None, 1, 5])
def test_support_ranges_cover_exactly_the_support(nquad):
    p = 3
    t = quad_point_tables(T_REP, p, nquad)
    n, Q = t["n"], t["Q"]
    assert t["qlo"].shape == (n,) and t["qhi"].shape == (n,)
    for i in range(n):
        inside = [q for q in range(Q) if t["first"][q] <= i <= t["first"][q] + p]
        assert inside, "every basis function of an open knot vector has quadrature points"
        assert inside == list(range(t["qlo"][i], t["qhi"][i]))
    assert np.all(np.diff(t["qlo"]) >= 0) and np.all(np.diff(t["qhi"]) >= 0)
    # the empty span shortens the supports that straddle the repeated knot
    full = (p + 1) * t["nq"]
    assert (t["qhi"] - t["qlo"]).max() == full and (t["qhi"] - t["qlo"])[5] < full


def test_support_ranges_of_sparse_points():
    # points that leave some basis functions without any point: empty ranges, qlo == qhi
    T, p = uniform_knots(2, 8), 2
    t = point_tables(T, p, [0.0, 0.01, 0.99, 1.0])
    qlo, qhi = support_ranges(t["first"], p, t["n"])
    for i in range(t["n"]):
        inside = [q for q in range(4) if t["first"][q] <= i <= t["first"][q] + p]
        assert inside == list(range(qlo[i], qhi[i]))
    assert np.any(qlo == qhi)


def test_field_entry_points_reject_null_handles():
    lib = _lib.lib
    der = (C.c_int * 3)(0, 0, 0)
    assert lib.poms_field_destroy(None) == 0
    assert lib.poms_field_eval(None, None, der, 0, 1, None, None) != 0
    assert b"null" in lib.poms_last_error().lower()
    assert lib.poms_field_load(None, None, 0, 1, 0, None, None) != 0
    assert lib.poms_field_error(None, None, der, None, 0, 1, None, None) != 0
    h = C.c_void_p()
    assert lib.poms_field_create(None, 3, None, None, None, None, None, None, None, None, 1, C.byref(h)) != 0
    with pytest.raises(_lib.PomsError):
        _lib.call("poms_field_eval", None, None, der, 0, 1, None, None)


def test_field_names_are_exported_lazily():
    import poms_amd
    for name in ("QuadGrid", "PointGrid", "assemble_rhs", "evaluate", "l2_error"):
        assert name in poms_amd.__all__
