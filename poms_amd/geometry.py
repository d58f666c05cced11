"""Mapped domains: the pull-back of ``-∇·(a∇u) + c u`` from a physical domain
``Ω = F([0,1]^d)`` to the parameter cube.

With ``J = ∂F/∂ξ`` the operator becomes one with a full symmetric tensor on the
parameter domain,

    -∇̂·(G ∇̂u) + γ u,   G = a |det J| J⁻¹ J⁻ᵀ,   γ = c |det J|,

which :func:`~poms_amd.assembly.assemble_stencil` and
:class:`~poms_amd.matfree.MatrixFreeOperator` take as a tensor coefficient.  The
reference assembles on the unit square only (`sources/matrix_assembler.py:84-179`);
this module supplies what a mapped domain adds: the Jacobian at the quadrature points
(:class:`Mapping` from callables, :class:`SplineMapping` from control points through
the spline-evaluation kernels), the pointwise pull-back (:func:`pullback`, closed-form
adjugate, elementwise torch operations on whatever device the Jacobian lives on), and
:class:`MappedDomain`, which ties a space, a mapping and a quadrature together.

Component order of ``G``: the upper triangle in row-major order, 3D ``00 01 02 11 12
22``, 2D ``00 01 11``, one plane per component (shape ``(ncomp,) + grid``).
"""
from __future__ import annotations

import math

import numpy as np
import torch

F64 = torch.float64


def _grid(J):
    d = len(J)
    if d not in (2, 3) or any(len(row) != d for row in J):
        raise ValueError("the Jacobian must be 2 x 2 or 3 x 3 (J[i][k] = dF_i / dxi_k)")
    return d


def pullback(J, a=None, c=None, mass_coef: float = 1.0):
    """``(G, gamma, det)`` from the Jacobian at a grid of points.

    ``J[i][k] = ∂F_i/∂ξ_k``: ``d x d`` float64 tensors of the grid's shape (a nested
    sequence, or one tensor of shape ``(d, d) + grid``), on any device.  ``a`` / ``c``:
    None (1 and ``mass_coef``), scalars or tensors of the grid's shape.  Returns
    ``G = a adj(J) adj(J)ᵀ / det`` as ``(ncomp,) + grid``, ``gamma = c det`` and
    ``det``, on the Jacobian's device.  Raises ``ValueError`` if ``det <= 0`` anywhere
    (one host read)."""
    d = _grid(J)
    J = [[torch.as_tensor(J[i][k], dtype=F64) for k in range(d)] for i in range(d)]
    if d == 2:
        det = J[0][0] * J[1][1] - J[0][1] * J[1][0]
        K = [[J[1][1], -J[0][1]], [-J[1][0], J[0][0]]]
    else:
        # adj(J)[i][j] = the cofactor of J[j][i]
        def cof(r, s):
            r0, r1 = [k for k in range(3) if k != r]
            s0, s1 = [k for k in range(3) if k != s]
            m = J[r0][s0] * J[r1][s1] - J[r0][s1] * J[r1][s0]
            return m if (r + s) % 2 == 0 else -m
        K = [[cof(j, i) for j in range(3)] for i in range(3)]
        det = J[0][0] * K[0][0] + J[0][1] * K[1][0] + J[0][2] * K[2][0]
    if not bool((det > 0).all()):
        raise ValueError(f"the mapping is not orientation-preserving and invertible at every point: "
                         f"min det J = {float(det.min()):.3e} <= 0")
    scale = 1.0 / det if a is None else torch.as_tensor(a, dtype=F64, device=det.device) / det
    comps = []
    for i in range(d):
        for j in range(i, d):
            s = K[i][0] * K[j][0]
            for k in range(1, d):
                s = s + K[i][k] * K[j][k]
            comps.append(s * scale)
    G = torch.stack([torch.broadcast_to(g, det.shape) for g in comps]).contiguous()
    cc = float(mass_coef) if c is None else torch.as_tensor(c, dtype=F64, device=det.device)
    gamma = (det * cc).contiguous()
    return G, gamma, det.contiguous()


def surface_measure(J, axis: int):
    """The surface Jacobian of the face ``ξ_axis = const`` from the Jacobian ``J[i][k] =
    ∂F_i/∂ξ_k`` at a grid of points on it (the nested tensors :meth:`_MappingBase.jacobian`
    returns for a grid whose ``axis`` has one point): ``|∂F/∂ξ_t|`` in 2D (``t`` the other
    axis), ``|∂F/∂ξ_a × ∂F/∂ξ_b|`` in 3D (``a``, ``b`` the other two).  Closed form,
    elementwise torch operations on the Jacobian's device; the result has the grid's shape."""
    d = _grid(J)
    if not 0 <= int(axis) < d:
        raise ValueError(f"axis must be 0 .. {d - 1}, got {axis}")
    J = [[torch.as_tensor(J[i][k], dtype=F64) for k in range(d)] for i in range(d)]
    if d == 2:
        t = 1 - int(axis)
        return torch.sqrt(J[0][t] * J[0][t] + J[1][t] * J[1][t])
    a, b = [k for k in range(3) if k != int(axis)]
    n0 = J[1][a] * J[2][b] - J[2][a] * J[1][b]
    n1 = J[2][a] * J[0][b] - J[0][a] * J[2][b]
    n2 = J[0][a] * J[1][b] - J[1][a] * J[0][b]
    return torch.sqrt(n0 * n0 + n1 * n1 + n2 * n2)


class _MappingBase:
    """``physical`` and ``jacobian`` at a tensor grid of points; :meth:`pullback` on top."""

    ndim: int

    def physical(self, points_per_axis, device=None):
        raise NotImplementedError

    def jacobian(self, points_per_axis, device=None):
        raise NotImplementedError

    def pullback(self, points_per_axis, a=None, c=None, mass_coef: float = 1.0, device=None):
        """``(G, gamma, det)`` on the tensor grid of ``points_per_axis`` (one 1D array
        per axis) as float64 tensors on ``device`` (default: the current GPU), ``G`` in
        the layout the operators read.  ``a`` / ``c``: None (1 and ``mass_coef``),
        scalars, arrays of the grid's shape, or NumPy callables of the *physical*
        coordinates ``x = F(ξ)``."""
        J = self.jacobian(points_per_axis, device)
        dev = J[0][0].device
        if callable(a) or callable(c):
            x = [xi.cpu().numpy() for xi in self.physical(points_per_axis, device)]
        shape = tuple(len(np.atleast_1d(p)) for p in points_per_axis)

        def field(f):
            if f is None:
                return None
            v = np.asarray(f(*x) if callable(f) else f, dtype=np.float64)
            return torch.from_numpy(np.array(np.broadcast_to(v, shape), dtype=np.float64, order="C")).to(dev)

        return pullback(J, field(a), field(c), mass_coef)


def _default_device(device):
    if device is not None:
        return torch.device(device)
    return torch.device(f"cuda:{torch.cuda.current_device()}")


class Mapping(_MappingBase):
    """A mapping given by two NumPy callables of the ``meshgrid`` coordinates
    (``indexing='ij'``): ``F(*xi)`` returns the ``d`` physical coordinates and
    ``jac(*xi)`` the nested ``J[i][k] = ∂F_i/∂ξ_k``; entries may be scalars or arrays
    that broadcast to the grid."""

    def __init__(self, F, jac, ndim: int | None = None):
        if not callable(F) or not callable(jac):
            raise TypeError("F and jac must be callables of the meshgrid coordinates")
        self.F, self.jac, self.ndim = F, jac, ndim

    def _grids(self, points_per_axis):
        pts = [np.atleast_1d(np.asarray(p, dtype=np.float64)) for p in points_per_axis]
        if self.ndim is not None and len(pts) != self.ndim:
            raise ValueError(f"a {self.ndim}D mapping needs {self.ndim} point arrays")
        return np.meshgrid(*pts, indexing="ij")

    @staticmethod
    def _up(v, shape, dev):
        v = np.broadcast_to(np.asarray(v, dtype=np.float64), shape)
        return torch.from_numpy(np.array(v, dtype=np.float64, order="C")).to(dev)

    def physical(self, points_per_axis, device=None):
        grids = self._grids(points_per_axis)
        x = self.F(*grids)
        if len(x) != len(grids):
            raise ValueError(f"F returned {len(x)} coordinates on a {len(grids)}D grid")
        dev = _default_device(device)
        return [self._up(xi, grids[0].shape, dev) for xi in x]

    def jacobian(self, points_per_axis, device=None):
        grids = self._grids(points_per_axis)
        J = self.jac(*grids)
        d = len(grids)
        if len(J) != d or any(len(row) != d for row in J):
            raise ValueError(f"jac must return a {d} x {d} nested sequence")
        dev = _default_device(device)
        return [[self._up(J[i][k], grids[0].shape, dev) for k in range(d)] for i in range(d)]


class SplineMapping(_MappingBase):
    """An isogeometric mapping ``F_i = Σ_j coeffs[i]_j B_j``: ``coeffs`` are ``d``
    :class:`~poms_amd.stencil.StencilVector` of control-point coordinates on the space
    ``V`` of ``knots``.  Values and Jacobian at a tensor grid of points come from
    :class:`~poms_amd.field.PointGrid` (``d`` and ``d²`` evaluation launches)."""

    def __init__(self, V, knots, coeffs):
        if len(coeffs) != V.ndim or len(knots) != V.ndim:
            raise ValueError(f"a {V.ndim}D spline mapping needs {V.ndim} knot vectors and {V.ndim} "
                             "control-point vectors")
        self.space, self.knots, self.coeffs, self.ndim = V, [np.asarray(T, float) for T in knots], list(coeffs), V.ndim

    def _point_grid(self, points_per_axis, device):
        from .field import PointGrid
        if device is not None and torch.device(device) != torch.device(f"cuda:{self.space.device}"):
            raise ValueError(f"a spline mapping is evaluated on its space's device cuda:{self.space.device}")
        return PointGrid(self.space, self.knots, points_per_axis)

    def physical(self, points_per_axis, device=None):
        pg = self._point_grid(points_per_axis, device)
        return [pg.evaluate(cf) for cf in self.coeffs]

    def jacobian(self, points_per_axis, device=None):
        pg = self._point_grid(points_per_axis, device)
        d = self.ndim
        return [[pg.evaluate(self.coeffs[i], der=tuple(int(m == k) for m in range(d))) for k in range(d)]
                for i in range(d)]


class MappedDomain:
    """A tensor B-spline space on a mapped domain: the space ``V`` of ``knots``, a
    mapping and the Gauss quadrature of ``nquad`` points per element (default ``p+1``).

    ``a``, ``c``, ``f`` and ``u`` below are NumPy callables of the physical
    coordinates (or scalars / arrays of :attr:`quad_shape`)."""

    def __init__(self, V, knots, mapping, nquad: int | None = None):
        from .assembly import axis_tables
        if len(knots) != V.ndim:
            raise ValueError(f"{V.ndim}D space needs {V.ndim} knot vectors")
        self.space, self.mapping, self.nquad = V, mapping, nquad
        self.knots = [np.asarray(T, float) for T in knots]
        tabs = [axis_tables(T, V.pads[d], nquad) for d, T in enumerate(self.knots)]
        self.points = [t["points"].reshape(-1) for t in tabs]
        self._weights = [t["weights"].reshape(-1) for t in tabs]
        self.quad_shape = tuple(len(p) for p in self.points)
        self._dev = f"cuda:{V.device}"
        self._quad = self._wdet = self._x = None

    def pullback(self, a=None, c=None, mass_coef: float = 1.0):
        """``(G, gamma, det)`` at the quadrature points."""
        return self.mapping.pullback(self.points, a=a, c=c, mass_coef=mass_coef, device=self._dev)

    def operator(self, a=None, c=None, mass_coef: float = 1.0, matrix_free: bool = False, dirichlet=None,
                 robin=None):
        """``-∇·(a∇u) + c u`` on the physical domain, as the stored stencil or
        (``matrix_free``) a :class:`~poms_amd.matfree.MatrixFreeOperator`; ``dirichlet``:
        its constrained faces; ``robin``: ``{(axis, side): β}`` (or a ``RobinBC``), the Robin faces
        ``a ∂ₙu + β u = g`` of the physical boundary, β a scalar or a function of the physical
        coordinates (:mod:`poms_amd.boundary`)."""
        G, gamma, _ = self.pullback(a, c, mass_coef)
        rb = self.robin(robin) if robin is not None else None
        if matrix_free:
            from .matfree import MatrixFreeOperator
            return MatrixFreeOperator(self.space, self.knots, a=G, c=gamma, nquad=self.nquad, dirichlet=dirichlet,
                                      robin=rb)
        from .assembly import assemble_stencil
        return assemble_stencil(self.space, self.knots, a=G, c=gamma, nquad=self.nquad, dirichlet=dirichlet, robin=rb)

    def robin(self, robin):
        """The :class:`~poms_amd.boundary.RobinBC` of the domain: β and the face data as
        functions of the physical coordinates, the face integrals with the surface measure.
        A ``RobinBC`` is returned as it is."""
        from .boundary import RobinBC
        if isinstance(robin, RobinBC):
            return robin
        return RobinBC(self.space, self.knots, robin, mapping=self.mapping, nquad=self.nquad)

    def boundary_load(self, g, out=None):
        """``∫_Γ g φ_i ds`` over the faces of ``g = {(axis, side): data}`` on the physical
        boundary, added into ``out`` (default: a zero vector)."""
        return self.robin(None).load_vector(g, out)

    def dirichlet(self, faces):
        """The :class:`~poms_amd.boundary.DirichletBC` of the domain: boundary data as a
        function of the physical coordinates."""
        from .boundary import DirichletBC
        return DirichletBC(self.space, self.knots, faces, mapping=self.mapping)

    def _setup(self):
        if self._quad is None:
            from .field import QuadGrid
            self._quad = QuadGrid(self.space, self.knots, self.nquad)
            J = self.mapping.jacobian(self.points, self._dev)
            det = pullback(J)[2]
            w = None
            for d, wd in enumerate(self._weights):
                shp = [1] * len(self._weights)
                shp[d] = len(wd)
                t = torch.from_numpy(np.ascontiguousarray(wd)).to(self._dev).reshape(shp)
                w = t if w is None else w * t
            self._det, self._wdet = det, w * det
            self._x = [xi.cpu().numpy() for xi in self.mapping.physical(self.points, self._dev)]

    def _sample(self, f):
        v = np.asarray(f(*self._x) if callable(f) else f, dtype=np.float64)
        v = np.array(np.broadcast_to(v, self.quad_shape), dtype=np.float64, order="C")
        return torch.from_numpy(v).to(self._dev)

    def load_vector(self, f):
        """``b[i] = ∫_Ω f φ_i`` : :meth:`QuadGrid.load_vector` of ``(f∘F) det J``."""
        self._setup()
        return self._quad.load_vector(self._sample(f) * self._det)

    def l2_error(self, x, u) -> float:
        """``‖u_h − u‖`` in L2 of the physical domain (weights ``w det J``)."""
        self._setup()
        e = self._quad.evaluate(x) - self._sample(u)
        return math.sqrt(float((self._wdet * e * e).sum().item()))
