"""Spline fields on tensor point grids: from a function ``f`` to the load vector ``b``,
and from a coefficient vector ``x`` back to the function ``u_h`` it stands for.

The solvers of this package work on ``A x = b``; the reference's drivers take
``b[i] = 1`` (`sources/mg_jac.py:57-62`) and never look at ``u_h``.  This module adds,
on the device (``csrc/spline_field.hip``, three sum-factorised 1D passes each):

* ``grid.evaluate(x)``      -- ``u_h`` (or a first derivative) at every point of a
  tensor grid: the quadrature grid of the space (:class:`QuadGrid`) or any
  tensor grid of points (:class:`PointGrid`);
* ``grid.load_vector(f)``   -- ``b[i] = ∫ f B_i`` by Gauss quadrature;
* ``grid.l2_error(x, u)``   -- ``‖u_h − u‖`` in L2, fused (the point values are
  never stored), and ``grid.h1_seminorm_error(x, grad_u)``.

``f`` / ``u`` are a scalar, an array or tensor of the grid's shape, or a callable of
one broadcastable device tensor per axis (``(Q0,1,1), (1,Q1,1), (1,1,Q2)`` in 3D) that
returns a device tensor.  Grids larger than ``chunk_bytes`` are walked in axis-0
slices, so a callable never materialises the whole grid.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Sequence

import numpy as np
import torch

from . import _lib
from . import runtime as rt
from .assembly import point_tables, quad_point_tables, support_ranges
from .stencil import StencilVector, StencilVectorSpace

F64 = torch.float64
DEFAULT_CHUNK_BYTES = 256 << 20


class _TensorGrid:
    """Per-axis tables of a tensor grid of points, uploaded once (``poms_field_create``)."""

    def __init__(self, V: StencilVectorSpace, tabs: Sequence[dict], chunk_bytes: int):
        if V.is_distributed or tuple(V.local_npts) != tuple(V.npts):
            raise NotImplementedError("spline fields are implemented for undistributed spaces "
                                      "(the axis-0 tables would have to follow the slabs)")
        if len(tabs) != V.ndim:
            raise ValueError(f"{V.ndim}D space needs {V.ndim} knot vectors")
        for d, t in enumerate(tabs):
            if t["n"] != V.npts[d] or t["p"] != V.pads[d]:
                raise ValueError(f"axis {d}: tables of {t['n']} functions of degree {t['p']}, space has "
                                 f"{V.npts[d]} of degree {V.pads[d]}")
        self.space = V
        self.ndim = V.ndim
        self.shape = tuple(int(t["Q"]) for t in tabs)
        self.points = [np.array(t["points"], dtype=np.float64) for t in tabs]
        has_w = all(t.get("weights") is not None for t in tabs)
        self.weights = [np.array(t["weights"], dtype=np.float64) for t in tabs] if has_w else None
        lead = 3 - self.ndim
        self._shape3 = (1,) * lead + self.shape
        row_bytes = 8 * self._shape3[1] * self._shape3[2]
        self.chunk_q0 = int(max(1, min(self._shape3[0], int(chunk_bytes) // row_bytes)))
        self._dev = f"cuda:{V.device}"
        self._pts_dev = None

        keep = []

        def arr3(key, dtype, dummy):
            out = (C.c_void_p * 3)()
            for k in range(3):
                a = dummy if k < lead else tabs[k - lead][key]
                a = np.ascontiguousarray(a, dtype=dtype)
                keep.append(a)
                out[k] = a.ctypes.data
            return out

        npts = (C.c_int64 * 3)(*self._shape3)
        pp = (C.c_int * 3)(*([0] * lead + [int(t["p"]) for t in tabs]))
        ranges = has_w
        if ranges:
            for t in tabs:
                if "qlo" not in t:
                    t["qlo"], t["qhi"] = support_ranges(t["first"], t["p"], t["n"])
        h = C.c_void_p()
        _lib.call("poms_field_create", V.ctx, self.ndim, C.byref(V.layout), npts, pp,
                  arr3("first", np.int32, [0]), arr3("basis", np.float64, [1.0, 0.0]),
                  arr3("weights", np.float64, [1.0]) if has_w else None,
                  arr3("qlo", np.int32, [0]) if ranges else None, arr3("qhi", np.int32, [1]) if ranges else None,
                  self.chunk_q0, C.byref(h))
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.lib.poms_field_destroy(h)
            except Exception:
                pass
            self._h = None

    # -- helpers -------------------------------------------------------------------
    def _chunks(self):
        Q0 = self._shape3[0]
        return [(b, min(b + self.chunk_q0, Q0)) for b in range(0, Q0, self.chunk_q0)]

    def _der3(self, der):
        if der is None:
            der = (0,) * self.ndim
        der = tuple(int(v) for v in der)
        if len(der) != self.ndim or any(v not in (0, 1) for v in der):
            raise ValueError(f"der needs {self.ndim} entries of 0 (value) or 1 (first derivative), got {der}")
        return (C.c_int * 3)(*((0,) * (3 - self.ndim) + der))

    def _check_x(self, x):
        V = self.space
        if not isinstance(x, StencilVector) or (x.space is not V and (
                x.space.local_npts, x.space.pads, x.space.pitch, x.space.shift, x.space.device)
                != (V.local_npts, V.pads, V.pitch, V.shift, V.device)):
            raise TypeError("x must be a StencilVector of the grid's space")

    def _axis_points(self, b, e):
        """The points of axis-0 slice [b, e) as one broadcastable device tensor per axis."""
        if self._pts_dev is None:
            self._pts_dev = [torch.from_numpy(p).to(self._dev) for p in self.points]
        out = []
        for d, p in enumerate(self._pts_dev):
            if d == 0 and self.ndim == 3:
                p = p[b:e]
            shp = [1] * self.ndim
            shp[d] = p.numel()
            out.append(p.reshape(shp))
        return out

    def _prepare(self, f, what):
        """Validate a field argument before any launch; returns ``chunk(b, e)`` giving the
        contiguous device block of the axis-0 slice (leading unit axes dropped)."""
        if callable(f):
            def chunk(b, e):
                v = torch.as_tensor(f(*self._axis_points(b, e)), dtype=F64, device=self._dev)
                return torch.broadcast_to(v, self._slice_shape(b, e)).contiguous()
            return chunk
        if isinstance(f, (int, float, np.floating, np.integer)):
            return lambda b, e: torch.full(self._slice_shape(b, e), float(f), dtype=F64, device=self._dev)
        t = f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f, dtype=np.float64))
        if tuple(t.shape) != self.shape:
            raise ValueError(f"{what} has shape {tuple(t.shape)}, the grid has {self.shape}")
        t = t.to(device=self._dev, dtype=F64)
        if self.ndim == 3:
            return lambda b, e: t[b:e].contiguous()
        t = t.contiguous()
        return lambda b, e: t

    def _slice_shape(self, b, e):
        return (e - b,) + self.shape[1:] if self.ndim == 3 else self.shape

    # -- evaluation ------------------------------------------------------------------
    def evaluate(self, x: StencilVector, der=None, out: torch.Tensor | None = None) -> torch.Tensor:
        """``u_h`` of the coefficients ``x`` at every point (``der[d] = 1``: the first
        derivative along axis ``d``), a device tensor of ``.shape``."""
        self._check_x(x)
        d3 = self._der3(der)
        if out is None:
            out = torch.empty(self.shape, dtype=F64, device=self._dev)
        elif tuple(out.shape) != self.shape or out.dtype != F64 or not out.is_contiguous() or not out.is_cuda:
            raise ValueError(f"out must be a contiguous float64 device tensor of shape {self.shape}")
        row = self._shape3[1] * self._shape3[2]
        st = rt.stream_handle()
        for b, e in self._chunks():
            _lib.call("poms_field_eval", self._h, rt.ptr(x._data), d3, b, e,
                      C.c_void_p(out.data_ptr() + 8 * b * row), st)
        return out

    def _need_weights(self, what):
        if self.weights is None:
            raise ValueError(f"{what} needs quadrature weights: use a QuadGrid")

    def sq_error(self, x: StencilVector, u=None, der=None) -> torch.Tensor:
        """``Σ_q w_q (u_h(q) − u(q))²`` as a device tensor of shape (1,) (no host read)."""
        self._need_weights("the error")
        self._check_x(x)
        d3 = self._der3(der)
        get = None if u is None else self._prepare(u, "u")
        acc = torch.zeros(1, dtype=F64, device=self._dev)
        st = rt.stream_handle()
        for b, e in self._chunks():
            ub = None if get is None else get(b, e)
            _lib.call("poms_field_error", self._h, rt.ptr(x._data), d3, None if ub is None else rt.ptr(ub),
                      b, e, rt.ptr(acc), st)
        return acc

    def l2_error(self, x: StencilVector, u=None, der=None) -> float:
        """``‖u_h − u‖`` in L2 by the grid's quadrature (``u=None``: ``‖u_h‖``); with
        ``der`` the same for a first derivative."""
        return math.sqrt(float(self.sq_error(x, u, der).item()))

    def h1_seminorm_error(self, x: StencilVector, grad_u) -> float:
        """``|u_h − u|_{H1}``: ``grad_u[d]`` is the derivative of ``u`` along axis ``d``."""
        if len(grad_u) != self.ndim:
            raise ValueError(f"grad_u needs {self.ndim} components")
        tot = None
        for d in range(self.ndim):
            s = self.sq_error(x, grad_u[d], tuple(int(k == d) for k in range(self.ndim)))
            tot = s if tot is None else tot + s
        return math.sqrt(float(tot.item()))

    def load_vector(self, f, out: StencilVector | None = None) -> StencilVector:
        """``b[i] = Σ_q w_q B_i(q) f(q)``, the right-hand side of ``f`` (gather form:
        bitwise reproducible for a given chunking)."""
        self._need_weights("load_vector")
        get = self._prepare(f, "f")
        if out is None:
            out = self.space.zeros()
        else:
            self._check_x(out)
        st = rt.stream_handle()
        for k, (b, e) in enumerate(self._chunks()):
            fb = get(b, e)
            _lib.call("poms_field_load", self._h, rt.ptr(fb), b, e, int(k > 0), rt.ptr(out._data), st)
        out._mark_written()
        return out


def _check_knots(V, knots):
    if len(knots) != V.ndim:
        raise ValueError(f"{V.ndim}D space needs {V.ndim} knot vectors")


class QuadGrid(_TensorGrid):
    """The Gauss quadrature grid of a tensor B-spline space: ``nquad`` points (default
    ``p+1``) in every non-empty knot span, ``shape[d] = nel_d · nquad`` points per axis."""

    def __init__(self, V: StencilVectorSpace, knots, nquad: int | None = None,
                 chunk_bytes: int = DEFAULT_CHUNK_BYTES):
        _check_knots(V, knots)
        super().__init__(V, [quad_point_tables(np.asarray(T, float), V.pads[d], nquad) for d, T in enumerate(knots)],
                         chunk_bytes)


class PointGrid(_TensorGrid):
    """A tensor grid of arbitrary points (one non-decreasing 1D array per axis) to
    evaluate on; it has no weights, so no load vector and no error."""

    def __init__(self, V: StencilVectorSpace, knots, points, chunk_bytes: int = DEFAULT_CHUNK_BYTES):
        _check_knots(V, knots)
        if len(points) != V.ndim:
            raise ValueError(f"{V.ndim}D space needs {V.ndim} point arrays")
        super().__init__(V, [point_tables(np.asarray(T, float), V.pads[d], points[d]) for d, T in enumerate(knots)],
                         chunk_bytes)


def assemble_rhs(V, knots, f, nquad: int | None = None) -> StencilVector:
    """Load vector of ``f`` on the space of ``knots`` (see :meth:`QuadGrid.load_vector`)."""
    return QuadGrid(V, knots, nquad).load_vector(f)


def evaluate(V, knots, x, points, der=None) -> torch.Tensor:
    """``u_h`` of ``x`` on the tensor grid of ``points`` (see :meth:`PointGrid.evaluate`)."""
    return PointGrid(V, knots, points).evaluate(x, der)


def l2_error(V, knots, x, u, nquad: int | None = None) -> float:
    """``‖u_h − u‖`` in L2 (see :meth:`QuadGrid.l2_error`)."""
    return QuadGrid(V, knots, nquad).l2_error(x, u)


def evaluate_at(V, knots, x, pos, der=None) -> torch.Tensor:
    """``u_h`` of ``x`` at the scattered points ``pos``, a ``(ndim, N)`` device tensor
    (see :meth:`poms_amd.points.SplinePoints.evaluate`)."""
    from .points import SplinePoints
    return SplinePoints(V, knots).evaluate(x, pos, der)


def deposit(V, knots, pos, w=None) -> StencilVector:
    """Load vector ``b[i] = Σ_k w_k B_i(x_k)`` of point sources at ``pos``
    (see :meth:`poms_amd.points.SplinePoints.deposit`)."""
    from .points import SplinePoints
    return SplinePoints(V, knots).deposit(pos, w)
