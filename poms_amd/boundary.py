"""Dirichlet (essential) boundary conditions on whole faces of the parameter cube.

On open knot vectors a face of the domain is one layer of coefficients: index 0 or
``n_d - 1`` on one axis.  ``faces`` is one ``(lo, hi)`` pair of bools per axis; the
constrained set C holds every coefficient whose index is 0 on an axis with ``lo`` or
``n_d - 1`` on an axis with ``hi``, and Π is the diagonal 0/1 projection onto the others
(a Kronecker product of per-axis projections).

* General forms (:class:`~poms_amd.stencil.StencilMatrix`,
  :class:`~poms_amd.matfree.MatrixFreeOperator`) apply
  ``A_D = Π A Π + (I − Π) D (I − Π)``, ``D = diag(A)``, to any input
  (``set_dirichlet``, a mask in the kernels; the stored coefficients stay those of A).
* Kronecker forms are built from constrained 1D factors
  (:func:`~poms_amd.splines.constrain_1d`, ``KronOperator.laplace(..., dirichlet=)``).
* :class:`DirichletBC` supplies what a solve with data ``u = g`` on C needs: the mask,
  the projection, the lift ``xg`` of ``g`` (Greville interpolation per face) and the
  right-hand side ``Π (b − A xg)``; the solution is ``xg + x`` with ``A_D x`` = that.

This module is the one place that reads the spellings of ``faces``.

Natural conditions with data live here too (:class:`RobinBC`): on a face ``(axis, side)``
the condition ``(G∇u)·n + β u = g`` adds the face mass ``S_ij = ∫_Γ β φ_i φ_j ds`` to the
operator and the face load ``∫_Γ g φ_i ds`` to the right-hand side (``β = 0``: inhomogeneous
Neumann, the right-hand side only).  Both are (d−1)-dimensional objects on the boundary layer
of coefficients, because on open knots the end function is 1 on the face and the others 0.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

from .splines import basis_funs_ders, find_span, greville

__all__ = ["normalize_faces", "faces_mask", "mask_faces", "constrained_mask", "constrain_dense",
           "check_unit_rows", "constrain_prolongation", "collocation_1d", "lift_host", "DirichletBC",
           "normalize_robin", "add_face_term", "RobinBC"]


def normalize_faces(faces, ndim: int):
    """``faces`` as a tuple of ``ndim`` ``(lo, hi)`` pairs of bools, or None when no face
    is constrained.  Accepted: ``None`` / ``False`` (none), ``True`` / ``"all"`` (every
    face), or a sequence of ``ndim`` pairs."""
    if faces is None or faces is False:
        return None
    if faces is True or (isinstance(faces, str) and faces == "all"):
        return tuple((True, True) for _ in range(ndim))
    if isinstance(faces, str):
        raise ValueError(f"dirichlet: unknown spelling {faces!r} (None, False, True, 'all' or one (lo, hi) pair per axis)")
    try:
        pairs = list(faces)
    except TypeError:
        raise ValueError(f"dirichlet: cannot read {faces!r} as one (lo, hi) pair per axis") from None
    if len(pairs) != ndim:
        raise ValueError(f"dirichlet: need one (lo, hi) pair per axis, {ndim} here, got {len(pairs)}")
    out = []
    for d, pr in enumerate(pairs):
        if isinstance(pr, (str, bytes)) or not hasattr(pr, "__len__") or len(pr) != 2:
            raise ValueError(f"dirichlet: axis {d}: expected a (lo, hi) pair, got {pr!r}")
        lo, hi = pr
        if not all(isinstance(v, (bool, np.bool_)) or v in (0, 1) for v in (lo, hi)):
            raise ValueError(f"dirichlet: axis {d}: lo and hi must be bools, got {pr!r}")
        out.append((bool(lo), bool(hi)))
    return tuple(out) if any(lo or hi for lo, hi in out) else None


def faces_mask(faces, ndim: int) -> int:
    """The bitmask of ``poms_op_set_dirichlet``: bit ``2 d + side`` in the operator's axes."""
    f = normalize_faces(faces, ndim)
    if f is None:
        return 0
    return sum((1 << (2 * d)) * lo + (1 << (2 * d + 1)) * hi for d, (lo, hi) in enumerate(f))


def mask_faces(mask: int, ndim: int):
    """:func:`faces_mask`'s inverse (None for 0)."""
    return normalize_faces([(bool(mask >> (2 * d) & 1), bool(mask >> (2 * d + 1) & 1)) for d in range(ndim)], ndim)


def constrained_mask(shape: Sequence[int], faces) -> np.ndarray:
    """Bool array of the grid's shape, True on C."""
    nd = len(shape)
    f = normalize_faces(faces, nd)
    m = np.zeros(tuple(shape), dtype=bool)
    if f is None:
        return m
    for d, (lo, hi) in enumerate(f):
        idx = [slice(None)] * nd
        if lo:
            idx[d] = 0
            m[tuple(idx)] = True
        if hi:
            idx[d] = shape[d] - 1
            m[tuple(idx)] = True
    return m


def constrain_dense(A: np.ndarray, shape: Sequence[int], faces) -> np.ndarray:
    """``Π A Π + (I − Π) diag(A) (I − Π)`` of a dense matrix on the grid ``shape``."""
    c = constrained_mask(shape, faces).reshape(-1)
    A = np.asarray(A, dtype=np.float64)
    free = (~c).astype(np.float64)
    return free[:, None] * A * free[None, :] + np.diag(np.where(c, np.diag(A), 0.0))


def check_unit_rows(P: Sequence[np.ndarray], faces) -> None:
    """For every constrained side the boundary row of the 1D prolongation ``P[d]`` must be
    the unit vector of the boundary column (true of knot insertion on open knots).  Then
    ``Π_f P Π_c = P Π_c`` and the Galerkin product of the constrained operator is the
    constrained Galerkin product.  Raises ``ValueError`` otherwise."""
    f = normalize_faces(faces, len(P))
    if f is None:
        return
    for d, (lo, hi) in enumerate(f):
        Pd = np.asarray(P[d])
        for on, r, c, name in ((lo, 0, 0, "first"), (hi, Pd.shape[0] - 1, Pd.shape[1] - 1, "last")):
            if not on:
                continue
            e = np.zeros(Pd.shape[1])
            e[c] = 1.0
            if not np.array_equal(Pd[r], e):
                raise ValueError(f"dirichlet: axis {d}: the {name} row of the prolongation is not the unit vector of "
                                 f"the {name} column, so the constrained face is not preserved between the levels")


def constrain_prolongation(P: np.ndarray, lo: bool, hi: bool) -> np.ndarray:
    """``P Π_c``: the columns of the constrained coarse functions zeroed, so restricted
    residuals and prolonged corrections vanish on C."""
    Pt = np.array(P, dtype=np.float64, order="C")
    if lo:
        Pt[:, 0] = 0.0
    if hi:
        Pt[:, -1] = 0.0
    return Pt


def collocation_1d(T: np.ndarray, p: int, pts: np.ndarray) -> np.ndarray:
    """``C[i, j] = B_j(pts[i])`` for the B-splines of degree ``p`` on ``T``."""
    T = np.asarray(T, dtype=np.float64)
    n = len(T) - p - 1
    Cm = np.zeros((len(pts), n))
    for i, x in enumerate(pts):
        s = find_span(T, p, float(x))
        Cm[i, s - p:s + 1] = basis_funs_ders(T, p, float(x), s, 0)[0]
    return Cm


def lift_host(knots, degrees, faces, g, physical=None) -> np.ndarray:
    """Coefficients of the lift of ``g``, as an array of the grid's shape: zero on the
    free coefficients; on each constrained face the coefficients of the tensor-product
    interpolant of ``g`` at the face's Greville points (1D collocation matrices per face
    axis, solved here).  ``g``: a scalar or a NumPy callable of the ``meshgrid``
    coordinates (``indexing='ij'``) -- the parameter coordinates, or what
    ``physical(points_per_axis)`` makes of them.  The faces are taken in the order axis 0
    lo, axis 0 hi, axis 1 lo, …, later ones overwriting earlier ones on shared edges and
    corners; the values agree there up to rounding, because the first and last Greville
    points are the end points, where one basis function equals 1."""
    nd = len(knots)
    f = normalize_faces(faces, nd)
    knots = [np.asarray(T, dtype=np.float64) for T in knots]
    shape = tuple(len(T) - p - 1 for T, p in zip(knots, degrees))
    out = np.zeros(shape)
    if f is None:
        return out
    grev = [greville(T, p) for T, p in zip(knots, degrees)]
    cinv = [None] * nd   # inverse collocation matrix per axis, formed on first use

    def solve_axis(vals, e, axis):
        if cinv[e] is None:
            cinv[e] = np.linalg.inv(collocation_1d(knots[e], degrees[e], grev[e]))
        return np.moveaxis(np.tensordot(cinv[e], vals, axes=(1, axis)), 0, axis)

    for d, (lo, hi) in enumerate(f):
        for on, idx in ((lo, 0), (hi, shape[d] - 1)):
            if not on:
                continue
            pts = [np.array([grev[e][idx]]) if e == d else grev[e] for e in range(nd)]
            fshape = tuple(len(p) for p in pts)
            if callable(g):
                coords = np.meshgrid(*pts, indexing="ij") if physical is None else physical(pts)
                vals = np.array(np.broadcast_to(np.asarray(g(*coords), dtype=np.float64), fshape))
            else:
                vals = np.full(fshape, float(g))
            for e in range(nd):
                if e != d:
                    vals = solve_axis(vals, e, e)
            sl = [slice(None)] * nd
            sl[d] = idx
            out[tuple(sl)] = np.take(vals, 0, axis=d)
    return out


class DirichletBC:
    """Boundary data on the constrained faces of the space ``V`` of ``knots``.

    ``faces``: see :func:`normalize_faces`.  ``mapping``: a mapping of
    :mod:`poms_amd.geometry`; ``g`` in :meth:`lift` is then a function of the physical
    coordinates."""

    def __init__(self, V, knots, faces, mapping=None):
        if len(knots) != V.ndim:
            raise ValueError(f"{V.ndim}D space needs {V.ndim} knot vectors")
        if V.is_distributed or V.is_cart:
            raise NotImplementedError("dirichlet: distributed (slab / Cart) spaces are not supported")
        self.space, self.mapping = V, mapping
        self.knots = [np.asarray(T, dtype=np.float64) for T in knots]
        self.faces = normalize_faces(faces, V.ndim)
        self._mask = None

    def mask(self):
        """Device bool tensor of the grid's shape, True on C."""
        import torch
        if self._mask is None:
            m = constrained_mask(self.space.npts, self.faces)
            self._mask = torch.from_numpy(m).to(f"cuda:{self.space.device}")
        return self._mask

    def project(self, v):
        """Zero C in place (elementwise torch: a set-up path)."""
        V = self.space
        V.interior(v._data).masked_fill_(self.mask(), 0.0)
        v._mark_written()
        return v

    def lift(self, g):
        """The lift ``xg`` as a :class:`~poms_amd.stencil.StencilVector` (:func:`lift_host`)."""
        V = self.space
        phys = None
        if self.mapping is not None:
            dev = f"cuda:{V.device}"
            phys = lambda pts: [x.cpu().numpy() for x in self.mapping.physical(pts, dev)]
        return V.zeros().from_numpy(lift_host(self.knots, V.pads, self.faces, g, phys))

    def homogenize(self, A, b, xg):
        """``Π (b − A xg)`` with ``A`` applied unconstrained: a general form has its mask
        cleared around one ``dot``; a Kronecker operator must be the one built without
        ``dirichlet``."""
        faces = getattr(A, "dirichlet", None)
        if faces is not None and A.form not in ("stencil", "matfree"):
            raise ValueError("homogenize needs the Kronecker operator built without dirichlet (its constrained factors "
                             "do not apply A)")
        if faces is not None:
            A.set_dirichlet(None)
        try:
            r = A.residual(b, xg)
        finally:
            if faces is not None:
                A.set_dirichlet(faces)
        return self.project(r)


def normalize_robin(robin, ndim: int) -> dict:
    """``{(axis, side): value}`` with the faces in the order axis 0 lo, axis 0 hi, axis 1 lo, …
    (``side`` 0: index 0, 1: index ``n_axis − 1``, the numbering of ``poms_op_set_dirichlet``'s
    bits); None or an empty dict gives ``{}``."""
    if robin is None:
        return {}
    if not isinstance(robin, dict):
        raise ValueError(f"robin: expected a dict {{(axis, side): value}}, got {type(robin).__name__}")
    out = {}
    for key, val in robin.items():
        try:
            axis, side = key
        except (TypeError, ValueError):
            raise ValueError(f"robin: a face is an (axis, side) pair, got {key!r}") from None
        if not (isinstance(axis, (int, np.integer)) and 0 <= axis < ndim) or side not in (0, 1):
            raise ValueError(f"robin: face {key!r}: axis must be 0 .. {ndim - 1} and side 0 or 1")
        out[(int(axis), int(side))] = val
    return dict(sorted(out.items()))


def add_face_term(A, face, S: np.ndarray) -> None:
    """Add the face stencil ``S`` (:meth:`RobinBC.mass`) of ``face`` to a general form
    (``poms_op_add_face_term``): a stored stencil takes it into its coefficients, a
    matrix-free operator keeps it beside its quadrature form.  Host copies of what changed
    (the stencil's ``_data``, the matrix-free diagonal, the Chebyshev bound) are dropped."""
    import ctypes as C

    from . import _lib
    if getattr(A, "form", None) not in ("stencil", "matfree"):
        raise NotImplementedError("robin: a Kronecker operator takes its face terms through its factors: build it "
                                  "with KronOperator.laplace(..., robin=)")
    axis, side = face
    S = np.ascontiguousarray(S, dtype=np.float64)
    if S.ndim != 4:
        raise ValueError(f"robin: a face stencil has four dimensions (m_a, m_b, 2p_a+1, 2p_b+1), got shape {S.shape}")
    h = A._h   # (a stencil edited on the host is uploaded first)
    m = (C.c_int64 * 2)(S.shape[0], S.shape[1])
    half = (C.c_int * 2)((S.shape[2] - 1) // 2, (S.shape[3] - 1) // 2)
    try:
        _lib.call("poms_op_add_face_term", h, int(axis), int(side), S.ctypes.data_as(C.c_void_p), m, half)
    except _lib.PomsError as e:
        raise ValueError(str(e)) from None
    if A.form == "stencil":
        A._host = None   # (fetched again from the device on the next host-side access)
    else:
        A._diag = None
    A._lmax_est = None
    A._face_terms.append(((int(axis), int(side)), S))


class RobinBC:
    """Robin and inhomogeneous Neumann conditions ``(G∇u)·n + β u = g`` on whole faces of the
    space ``V`` of ``knots``.

    ``robin``: ``{(axis, side): β}``, ``β`` a scalar or a NumPy callable of the face's
    ``meshgrid`` coordinates (``indexing='ij'``): the d−1 parameter coordinates of the face's
    axes, or the d physical coordinates when a ``mapping`` of :mod:`poms_amd.geometry` is
    given.  The face terms are integrated with ``nquad`` Gauss points per element (default
    ``p+1``) times the surface Jacobian of the mapping (1 without one)."""

    def __init__(self, V, knots, robin, mapping=None, nquad: int | None = None):
        from .assembly import axis_tables
        if len(knots) != V.ndim:
            raise ValueError(f"{V.ndim}D space needs {V.ndim} knot vectors")
        if V.ndim not in (2, 3):
            raise ValueError("robin: face terms are implemented for 2D and 3D spaces")
        if V.is_distributed or V.is_cart or tuple(V.local_npts) != tuple(V.npts):
            raise NotImplementedError("robin: distributed (slab / Cart) spaces are not supported")
        self.space, self.mapping, self.nquad = V, mapping, nquad
        self.knots = [np.asarray(T, dtype=np.float64) for T in knots]
        self.robin = normalize_robin(robin, V.ndim)
        self._tabs = [axis_tables(T, V.pads[d], nquad) for d, T in enumerate(self.knots)]
        self._dev = f"cuda:{V.device}"
        self._quad = {}   # per normal axis: the face space and its QuadGrid (3D)

    def _face(self, face):
        (axis, side), = normalize_robin({face: 0.0}, self.space.ndim)
        return axis, side

    def face_points(self, face):
        """Per-axis 1D point arrays of the face's quadrature grid: the Gauss points on the
        face's axes, the single end point on the normal axis."""
        axis, side = self._face(face)
        T, p = self.knots[axis], self.space.pads[axis]
        end = T[p] if side == 0 else T[len(T) - p - 1]
        return [np.array([end]) if d == axis else t["points"].reshape(-1) for d, t in enumerate(self._tabs)]

    def _surface(self, face):
        """The surface Jacobian on the face's quadrature grid (device tensor), or None for 1."""
        if self.mapping is None:
            return None
        from .geometry import surface_measure
        axis, _ = self._face(face)
        return surface_measure(self.mapping.jacobian(self.face_points(face), self._dev), axis).squeeze(axis).contiguous()

    def _weights(self, face) -> np.ndarray:
        axis, _ = self._face(face)
        w = np.ones(())
        for d, t in enumerate(self._tabs):
            if d != axis:
                w = np.multiply.outer(w, t["weights"].reshape(-1))
        return w

    def measure(self, face, weights: bool = True):
        """``w·ds`` on the face's quadrature grid (its d−1 axes in increasing order): the Gauss
        weights of the face's axes times the surface Jacobian, a device tensor.  Every face
        integral of this class is a sum over it.  ``weights=False``: ``ds`` alone, for the
        device paths whose kernels apply the Gauss weights themselves."""
        import torch
        ds = self._surface(face)
        if not weights:
            shape = tuple(len(q) for d, q in enumerate(self.face_points(face)) if d != self._face(face)[0])
            return torch.ones(shape, dtype=torch.float64, device=self._dev) if ds is None else ds
        w = torch.from_numpy(np.ascontiguousarray(self._weights(face))).to(self._dev)
        return w if ds is None else w * ds

    def _sample(self, face, f) -> np.ndarray:
        """``f`` on the face's quadrature grid: a scalar, or a callable of the d−1 parameter
        coordinates of the face (of the d physical coordinates under a mapping)."""
        axis, _ = self._face(face)
        pts = self.face_points(face)
        shape = tuple(len(q) for d, q in enumerate(pts) if d != axis)
        if not callable(f):
            if np.ndim(f) != 0:
                raise ValueError("robin: β and g are scalars or callables of the face's coordinates")
            return np.full(shape, float(f))
        if self.mapping is None:
            coords = np.meshgrid(*[q for d, q in enumerate(pts) if d != axis], indexing="ij")
        else:
            coords = [np.squeeze(x.cpu().numpy(), axis=axis) for x in self.mapping.physical(pts, self._dev)]
        return np.array(np.broadcast_to(np.asarray(f(*coords), dtype=np.float64), shape), order="C")

    def _face_space(self, face):
        """The 2D space of a 3D problem's face and its quadrature grid (shared by both sides)."""
        from .field import QuadGrid
        from .stencil import StencilVectorSpace
        axis, _ = self._face(face)
        if axis not in self._quad:
            V = self.space
            ax = [d for d in range(V.ndim) if d != axis]
            Vf = StencilVectorSpace([V.npts[d] for d in ax], [V.pads[d] for d in ax], device=V.device)
            kn = [self.knots[d] for d in ax]
            self._quad[axis] = (Vf, kn, QuadGrid(Vf, kn, self.nquad))
        return self._quad[axis]

    def _weighted(self, face, f) -> np.ndarray:
        """``f`` times :meth:`measure` on the face's quadrature grid, on the host: ``f w ds`` for
        the 1D face of a 2D problem, summed on the host; ``f ds`` in 3D, where
        ``assemble_stencil`` and ``QuadGrid.load_vector`` on the face space apply ``w``."""
        return self._sample(face, f) * self.measure(face, weights=self.space.ndim == 2).cpu().numpy()

    def mass(self, face, beta=None) -> np.ndarray:
        """The face stencil ``S[i_a, i_b, k_a, k_b] = ∫_Γ β φ_i φ_(i+k−p) ds`` over the face's two
        axes in increasing order: float64 ``(m_a, m_b, 2p_a+1, 2p_b+1)``, interior rows only, C
        order, couplings to columns outside the grid exact zeros; a 2D operator has ``m_a = 1``,
        ``p_a = 0``.  In 3D it is :func:`~poms_amd.assembly.assemble_stencil` on the 2D face
        space with ``a = 0``, ``c = β ds``; the 1D face of a 2D problem is formed on the host
        from :func:`~poms_amd.assembly.axis_tables`.  ``beta``: default the face's own."""
        axis, side = self._face(face)
        if beta is None:
            beta = self.robin[(axis, side)]
        c = self._weighted((axis, side), beta)
        if self.space.ndim == 3:
            from .assembly import assemble_stencil
            Vf, kn, _ = self._face_space((axis, side))
            Sf = assemble_stencil(Vf, kn, a=0.0, c=c, nquad=self.nquad)
            return np.ascontiguousarray(Sf._data[tuple(slice(p, p + n) for p, n in zip(Vf.pads, Vf.npts))])
        t = self._tabs[1 - axis]
        p, n, nq = t["p"], t["n"], t["nq"]
        cw = c.reshape(t["nel"], nq)                         # β w ds
        S = np.zeros((1, n, 1, 2 * p + 1))
        for e in range(t["nel"]):
            B = t["basis"][e, :, :, 0]                       # (nq, p+1)
            El = np.einsum("q,qi,qj->ij", cw[e], B, B)       # the element's (p+1) x (p+1) block
            f0 = int(t["first"][e])
            for li in range(p + 1):
                S[0, f0 + li, 0, p - li:2 * p + 1 - li] += El[li]
        return S

    def apply(self, A):
        """Add every face's term to a :class:`~poms_amd.stencil.StencilMatrix` or a
        :class:`~poms_amd.matfree.MatrixFreeOperator` on this space: ``A`` becomes ``A + S``
        (calling it twice adds twice).  Returns ``A``."""
        if tuple(A.space.npts) != tuple(self.space.npts) or tuple(A.space.pads) != tuple(self.space.pads):
            raise ValueError("robin: the operator does not live on this space")
        for face in self.robin:
            add_face_term(A, face, self.mass(face))
        return A

    def load_vector(self, g, out=None):
        """Add the face loads ``∫_Γ g φ_i ds`` into ``out`` (default: a zero vector).  ``g``:
        ``{(axis, side): data}``, each a scalar or a callable as ``β``; it may name faces that
        are absent from ``robin`` (pure Neumann faces).  The loads are added into the boundary
        planes of ``out``, views of its interior (elementwise torch: a set-up path)."""
        import torch
        V = self.space
        g = normalize_robin(g, V.ndim)
        if out is None:
            out = V.zeros()
        inner = V.interior(out._data)
        for (axis, side), gf in g.items():
            v = self._weighted((axis, side), gf)
            if V.ndim == 3:
                Vf, _, quad = self._face_space((axis, side))
                load = Vf.interior(quad.load_vector(v)._data)
            else:
                t = self._tabs[1 - axis]
                vw = v.reshape(t["nel"], t["nq"])            # g w ds
                host = np.zeros(t["n"])
                for e in range(t["nel"]):
                    f0 = int(t["first"][e])
                    host[f0:f0 + t["p"] + 1] += vw[e] @ t["basis"][e, :, :, 0]
                load = torch.from_numpy(host).to(self._dev)
            idx = [slice(None)] * V.ndim
            idx[axis] = 0 if side == 0 else V.npts[axis] - 1
            inner[tuple(idx)] += load
        out._mark_written()
        return out
