"""On-device quadrature assembly of B-spline stencil operators.

The reference assembles ``-Δu + u`` element by element in Python
(`sources/matrix_assembler.py:84-179`, ``assembly_2d``: 222 s on one process for
the slides' grid, `sources/scalability.py:10`).  Here the host builds only the 1D
tables of each axis -- elements (non-empty knot spans), Gauss points and weights,
the ``p+1`` local B-splines and their derivatives at those points (Cox-de Boor,
:func:`poms_amd.splines.basis_funs_ders`) -- and ``poms_op_assemble_stencil``
forms every stencil coefficient on the device, one thread per (row, offset):

    M[i, j] = Σ_e Σ_q w_q (c(x_q) φ_i φ_j + a(x_q) ∇φ_i·∇φ_j)

With ``a = c = 1`` this is ``assembly_2d``'s operator (pinned by its golden
stencils); variable ``a``/``c`` (callables on the quadrature grid, or arrays of
its shape) give operators that are not Kronecker sums, applied by the
general-stencil kernel.

``a`` may also be a full symmetric *tensor* ``G`` at the quadrature points
(``poms_op_assemble_stencil_tensor``), the operator of a mapped domain or of
anisotropic diffusion,

    M[i, j] = Σ_e Σ_q w_q (c φ_i φ_j + ∇φ_iᵀ G ∇φ_j)

given as ``d(d+1)/2`` component planes, the upper triangle in row-major order
(3D: 00 01 02 11 12 22; 2D: 00 01 11): an array or a float64 device tensor of shape
``(ncomp,) + quad_shape``.  One more dimension than the quadrature grid is what
tells it from a scalar field.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .splines import basis_funs_ders, find_span
from .stencil import StencilMatrix, StencilVectorSpace


def axis_tables(T: np.ndarray, p: int, nquad: int | None = None) -> dict:
    """1D element tables of knot vector ``T`` (degree ``p``, ``nquad`` Gauss points,
    default ``p+1`` -- the reference's ``quad_order``)."""
    T = np.asarray(T, dtype=np.float64)
    n = len(T) - p - 1
    nq = p + 1 if nquad is None else int(nquad)
    xg, wg = np.polynomial.legendre.leggauss(nq)
    spans = [s for s in range(p, n) if T[s + 1] > T[s]]
    nel = len(spans)
    basis = np.zeros((nel, nq, p + 1, 2))
    weights = np.zeros((nel, nq))
    points = np.zeros((nel, nq))
    first = np.array([s - p for s in spans], dtype=np.int32)
    for e, s in enumerate(spans):
        a, b = T[s], T[s + 1]
        half = 0.5 * (b - a)
        for g in range(nq):
            x = a + half * (xg[g] + 1.0)
            points[e, g] = x
            weights[e, g] = half * wg[g]
            D = basis_funs_ders(T, p, x, s, 1)
            basis[e, g, :, 0] = D[0]
            basis[e, g, :, 1] = D[1]
    es = np.full(n, nel, dtype=np.int32)
    ee = np.full(n, -1, dtype=np.int32)
    for e, f in enumerate(first):
        for i in range(f, f + p + 1):
            es[i] = min(es[i], e)
            ee[i] = max(ee[i], e)
    return dict(n=n, p=p, nel=nel, nq=nq, first=first, es=es, ee=ee, basis=basis, weights=weights, points=points)


def point_tables(T: np.ndarray, p: int, pts) -> dict:
    """1D tables of the B-splines at arbitrary points: ``pts`` is a non-decreasing
    array in ``[T[p], T[n]]`` (repeats allowed).  ``first[q] = find_span - p`` is the
    first non-zero basis function at point ``q`` (the right end point falls in the
    last non-empty span, as :func:`find_span` puts it) and ``basis[q, a, 0:2]`` the
    value and first derivative of function ``first[q] + a``."""
    T = np.asarray(T, dtype=np.float64)
    pts = np.atleast_1d(np.asarray(pts, dtype=np.float64))
    n = len(T) - p - 1
    if pts.ndim != 1 or pts.size < 1:
        raise ValueError("points must be a non-empty 1D array")
    if np.any(np.diff(pts) < 0):
        raise ValueError("points must be non-decreasing")
    if pts[0] < T[p] or pts[-1] > T[n]:
        raise ValueError(f"points outside the domain [{T[p]}, {T[n]}]")
    Q = pts.size
    first = np.zeros(Q, dtype=np.int32)
    basis = np.zeros((Q, p + 1, 2))
    for q, x in enumerate(pts):
        s = find_span(T, p, x)
        first[q] = s - p
        D = basis_funs_ders(T, p, x, s, 1)
        basis[q, :, 0] = D[0]
        basis[q, :, 1] = D[1]
    return dict(n=n, p=p, Q=Q, points=pts.copy(), weights=None, first=first, basis=basis)


def support_ranges(first: np.ndarray, p: int, n: int):
    """Per basis function ``i`` the contiguous range ``[qlo[i], qhi[i])`` of the points
    ``q`` with ``first[q] <= i <= first[q] + p`` (``first`` non-decreasing); empty
    ranges have ``qlo == qhi``."""
    first = np.asarray(first, dtype=np.int64)
    i = np.arange(n)
    qlo = np.searchsorted(first, i - p, side="left").astype(np.int32)
    qhi = np.searchsorted(first, i, side="right").astype(np.int32)
    return qlo, np.maximum(qhi, qlo)


def quad_point_tables(T: np.ndarray, p: int, nquad: int | None = None) -> dict:
    """:func:`axis_tables` flattened to one row per quadrature point (``Q = nel nq``
    points in element order), with the support ranges the gather-form load vector
    needs: basis function ``i`` is non-zero exactly at points ``qlo[i] .. qhi[i]-1``."""
    t = axis_tables(T, p, nquad)
    Q = t["nel"] * t["nq"]
    first = np.repeat(t["first"], t["nq"]).astype(np.int32)
    qlo, qhi = support_ranges(first, p, t["n"])
    return dict(n=t["n"], p=p, Q=Q, nel=t["nel"], nq=t["nq"], points=t["points"].reshape(Q).copy(),
                weights=t["weights"].reshape(Q).copy(), first=first,
                basis=t["basis"].reshape(Q, p + 1, 2).copy(), qlo=qlo, qhi=qhi)


def _coef_field(f, tabs, device):
    if f is None:
        return None
    if callable(f):
        grids = np.meshgrid(*[t["points"].reshape(-1) for t in tabs], indexing="ij")
        vals = np.asarray(f(*grids), dtype=np.float64)
    else:
        vals = np.asarray(f, dtype=np.float64)
    shape = tuple(t["nel"] * t["nq"] for t in tabs)
    vals = np.broadcast_to(vals, shape)
    return torch.from_numpy(np.array(vals, dtype=np.float64, order="C")).to(device)


def used_in_place(f: torch.Tensor, shape, device, what: str = "coefficient tensor") -> torch.Tensor:
    """A device tensor an operator reads without a copy, after the checks: float64, of
    ``shape``, on ``device``, contiguous."""
    if f.dtype != torch.float64:
        raise TypeError(f"{what} must be float64, got {f.dtype}")
    if tuple(f.shape) != tuple(shape):
        raise ValueError(f"{what} has shape {tuple(f.shape)}, the quadrature grid {tuple(shape)}")
    if f.device != torch.device(device):
        raise ValueError(f"{what} lives on {f.device}, the space on {device}")
    if not f.is_contiguous():
        raise ValueError(f"{what} must be contiguous (C order)")
    return f


def _device_field(f, tabs, device):
    """A scalar field that is already a device tensor, used in place."""
    return used_in_place(f, tuple(t["nel"] * t["nq"] for t in tabs), device)


def tensor_ncomp(ndim: int) -> int:
    """Components of a symmetric ``ndim`` x ``ndim`` tensor coefficient."""
    return ndim * (ndim + 1) // 2


def split_coef(f, tabs):
    """``(values, is_tensor)``: a callable is sampled once at the quadrature points
    (``meshgrid``, ``indexing='ij'``); what has one dimension more than the quadrature
    grid is a tensor coefficient, anything else a scalar field."""
    if f is None:
        return None, False
    if callable(f):
        f = f(*np.meshgrid(*[t["points"].reshape(-1) for t in tabs], indexing="ij"))
    ndim = f.dim() if isinstance(f, torch.Tensor) else np.ndim(f)
    return f, ndim == len(tabs) + 1


def tensor_coef(g, tabs, device):
    """A tensor coefficient as the contiguous float64 device array of shape
    ``(ncomp,) + quad_shape`` the operators read: a float64 device tensor of that shape
    is used in place, an array is uploaded."""
    qshape = tuple(t["nel"] * t["nq"] for t in tabs)
    ncomp = tensor_ncomp(len(tabs))
    want = (ncomp,) + qshape
    got = tuple(g.shape) if isinstance(g, torch.Tensor) else np.shape(g)
    if len(got) != len(want) or got[1:] != qshape:
        raise ValueError(f"tensor coefficient has shape {got}, the quadrature grid needs {want}")
    if got[0] != ncomp:
        raise ValueError(f"tensor coefficient has {got[0]} components (shape {got}), a {len(tabs)}D operator "
                         f"needs ncomp = {ncomp}: the upper triangle in row-major order")
    if isinstance(g, torch.Tensor):
        return used_in_place(g, want, device, "tensor coefficient")
    return torch.from_numpy(np.array(g, dtype=np.float64, order="C")).to(device)


def quadrature_args(V: StencilVectorSpace, knots, nquad: int | None = None):
    """``(tabs, args, keep)``: every axis's :func:`axis_tables`, checked against the space; the
    constructors' arguments after the layout (``nel, nq, p, first, es, ee, basis, weights, nglob``,
    three entries each, unused leading axes empty); the arrays the pointers refer to."""
    nd = V.ndim
    if len(knots) != nd:
        raise ValueError(f"{nd}D space needs {nd} knot vectors")
    tabs = [axis_tables(np.asarray(T, float), V.pads[d], nquad) for d, T in enumerate(knots)]
    for d, t in enumerate(tabs):
        if t["n"] != V.npts[d]:
            raise ValueError(f"axis {d}: knots give {t['n']} basis functions, space has {V.npts[d]}")
    lead, keep = 3 - nd, []

    def pointers(key, dtype):
        arrs = [np.ascontiguousarray(t[key], dtype=dtype) for t in tabs]
        keep.extend(arrs)
        return (C.c_void_p * 3)(*([None] * lead + [a.ctypes.data for a in arrs]))

    ints = lambda key: (C.c_int * 3)(*([0] * lead + [int(t[key]) for t in tabs]))
    nglob = (C.c_int64 * 3)(*([1] * lead + [int(t["n"]) for t in tabs]))
    args = (ints("nel"), ints("nq"), ints("p"), pointers("first", np.int32), pointers("es", np.int32),
            pointers("ee", np.int32), pointers("basis", np.float64), pointers("weights", np.float64), nglob)
    return tabs, args, keep


def assemble_stencil(V: StencilVectorSpace, knots, a=None, c=None, mass_coef: float = 1.0,
                     nquad: int | None = None, dirichlet=None, robin=None) -> StencilMatrix:
    """``-∇·(a ∇u) + c u`` on the tensor space of ``knots`` (one knot vector per axis,
    degree = the space's pads), assembled on the device.  ``a``/``c``: None (1 and
    ``mass_coef``), a callable of the quadrature-point coordinates (``meshgrid``,
    ``indexing='ij'``) or an array of the quadrature grid's shape.  ``a`` may be a
    tensor coefficient: an array, a float64 device tensor, or a callable returning
    either, of shape ``(ncomp,) + quad_shape`` (see the module's text).  ``dirichlet``:
    constrained faces, passed to ``set_dirichlet`` (the assembled coefficients are those
    of the unconstrained operator).  ``robin``: ``{(axis, side): β}`` or a
    :class:`~poms_amd.boundary.RobinBC` of this space (which knows a mapping): the face
    masses are added into the stored coefficients, which are then those of ``A + S``."""
    nd = V.ndim
    if robin is not None:   # (refused before anything is assembled)
        from .boundary import RobinBC
        if not isinstance(robin, RobinBC):
            robin = RobinBC(V, knots, robin, nquad=nquad)
    if dirichlet is not None:   # (refused before anything is assembled)
        from .boundary import normalize_faces
        if normalize_faces(dirichlet, nd) is not None and (V.is_distributed or V.is_cart):
            raise NotImplementedError("dirichlet: distributed (slab / Cart) spaces are not supported")
    tabs, tables, _keep = quadrature_args(V, knots, nquad)
    dev = f"cuda:{V.device}"
    avals, tensor = split_coef(a, tabs)
    aq = tensor_coef(avals, tabs, dev) if tensor else _coef_field(avals, tabs, dev)
    cq = _device_field(c, tabs, dev) if isinstance(c, torch.Tensor) and c.is_cuda else _coef_field(c, tabs, dev)
    h = C.c_void_p()
    tail = (None if cq is None else C.c_void_p(cq.data_ptr()), float(mass_coef),
            int(V.starts[0]) if nd == 3 else 0, C.byref(h))
    if tensor:
        _lib.call("poms_op_assemble_stencil_tensor", V.ctx, nd, C.byref(V.layout), *tables,
                  C.c_void_p(aq.data_ptr()), tensor_ncomp(nd), *tail)
    else:
        _lib.call("poms_op_assemble_stencil", V.ctx, nd, C.byref(V.layout), *tables,
                  None if aq is None else C.c_void_p(aq.data_ptr()), *tail)
    A = StencilMatrix._from_handle(V, h)
    if robin is not None:
        robin.apply(A)
    if dirichlet is not None:
        A.set_dirichlet(dirichlet)
    return A
