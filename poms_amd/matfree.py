"""Matrix-free variable-coefficient operator and its V-cycle.

``-∇·(a∇u) + c u`` on a tensor B-spline space applied without a stored matrix
(``csrc/matfree.hip``, ``poms_op_create_matfree``):

    (A x)_i = Σ_q w_q [ c(q) u_h(q) φ_i(q) + a(q) ∇u_h(q)·∇φ_i(q) ]

is an evaluation at the quadrature points, a pointwise scaling and a load-vector
contraction, fused in one kernel.  It is the operator the reference assembles in
``assembly_2d`` (`sources/matrix_assembler.py:84-179`); its cycle
(`sources/mg_jac.py:84-119`) needs the fine operator only as ``A.dot``, its diagonal and
the residual.  Where :func:`~poms_amd.assembly.assemble_stencil` stores ``(2p+1)^d``
coefficients per row (2744 B/DOF in 3D at p = 3) this form holds the two coefficient
arrays at the quadrature points and an 8 B/DOF diagonal.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .assembly import (_coef_field, assemble_stencil, axis_tables, quadrature_args, split_coef, tensor_coef,
                       tensor_ncomp, used_in_place)
from .boundary import add_face_term
from .mg import GalerkinVCycle, uniform_hierarchy
from .stencil import KronOperator, StencilVectorSpace


def _coef_arg(f, tabs, device):
    """A coefficient as the device array the operator borrows: None stays None; a
    float64 device tensor of the quadrature grid's shape is used in place; a scalar, an
    array or a callable goes through :func:`assemble_stencil`'s preparation."""
    shape = tuple(t["nel"] * t["nq"] for t in tabs)
    if f is None:
        return None
    if isinstance(f, torch.Tensor):
        return used_in_place(f, shape, device)
    if not callable(f):
        got = np.shape(f)
        if got != () and got != shape:
            raise ValueError(f"coefficient array has shape {got}, the quadrature grid {shape}")
    return _coef_field(f, tabs, device)


def _diffusion_arg(a, tabs, device):
    """``(array, is_tensor)`` of the argument ``a``: a tensor coefficient (one dimension
    more than the quadrature grid, :func:`~poms_amd.assembly.tensor_coef`) or what
    :func:`_coef_arg` makes of a scalar field."""
    vals, tensor = split_coef(a, tabs)
    if tensor:
        return tensor_coef(vals, tabs, device), True
    if callable(a):
        return _coef_field(vals, tabs, device), False
    return _coef_arg(a, tabs, device), False


class MatrixFreeOperator(KronOperator):
    """``-∇·(a∇u) + c u`` on the tensor space of ``knots`` (degree = the space's pads,
    1…3; ``nquad`` 1…5 Gauss points per element, default ``p+1``), applied matrix-free.

    ``a`` / ``c``: what :func:`~poms_amd.assembly.assemble_stencil` accepts (None for 1
    and ``mass_coef``, a scalar, an array of the quadrature grid's shape
    (:attr:`quad_shape`), a NumPy callable of the ``meshgrid`` coordinates), or a
    float64 device tensor of that shape, which is used in place without a copy: the
    operator keeps a reference, and later changes to the tensor change the operator
    (but not its diagonal, formed once at creation).

    ``a`` may be a tensor coefficient ``G`` (``-∇·(G∇u) + c u``, a mapped domain or
    anisotropic diffusion, ``poms_op_create_matfree_tensor``): an array, a float64
    device tensor (used in place) or a callable returning either, of shape
    ``(ncomp,) + quad_shape`` with the ``d(d+1)/2`` components of the upper triangle in
    row-major order; one dimension more than the quadrature grid tells it from a
    scalar field (:attr:`tensor` is then True).

    ``dot``, ``residual``, ``dot_inner``, ``jacobi_sweep`` and ``diag_scale`` run the
    kernel's epilogues; ``pcg``, ``damped_jacobi``, ``jacobi`` and ``crl`` take the
    operator unchanged.  :meth:`assemble` gives the stored stencil of the same
    arguments for cross-checks.  ``dirichlet`` / :meth:`set_dirichlet`: constrained faces
    (:mod:`poms_amd.boundary`); the stored diagonal stays that of the unconstrained
    operator.  ``robin``: ``{(axis, side): β}`` or a :class:`~poms_amd.boundary.RobinBC` of the
    space: the face masses ``S`` are kept beside the quadrature form and applied by the
    kernel's ``FACE`` builds, and the stored diagonal is that of ``A + S``."""

    def __init__(self, V: StencilVectorSpace, knots, a=None, c=None, mass_coef: float = 1.0,
                 nquad: int | None = None, dirichlet=None, robin=None):
        if V.is_cart or V.is_distributed or tuple(V.local_npts) != tuple(V.npts):
            raise NotImplementedError("matrix-free operators are implemented for undistributed spaces "
                                      "(no slab or Cart decomposition)")
        nd = V.ndim
        if nd not in (2, 3):
            raise ValueError("matrix-free operators are 2D or 3D")
        tabs, tables, _keep = quadrature_args(V, knots, nquad)
        self._init_base(V, "matfree")
        self._h = C.c_void_p()
        self.knots = [np.asarray(T, float).copy() for T in knots]
        self.nquad, self.mass_coef = nquad, float(mass_coef)
        self._args = (a, c)
        self.quad_shape = tuple(t["nel"] * t["nq"] for t in tabs)
        dev = f"cuda:{V.device}"
        # the arrays the handle borrows live as long as this object
        (self._aq, self.tensor), self._cq = _diffusion_arg(a, tabs, dev), _coef_arg(c, tabs, dev)
        self._diag = None
        tail = (None if self._cq is None else C.c_void_p(self._cq.data_ptr()), self.mass_coef, C.byref(self._h))
        try:
            if self.tensor:
                _lib.call("poms_op_create_matfree_tensor", V.ctx, nd, C.byref(V.layout), *tables,
                          C.c_void_p(self._aq.data_ptr()), tensor_ncomp(nd), *tail)
            else:
                _lib.call("poms_op_create_matfree", V.ctx, nd, C.byref(V.layout), *tables,
                          None if self._aq is None else C.c_void_p(self._aq.data_ptr()), *tail)
        except _lib.PomsError as e:
            raise ValueError(str(e)) from None
        if robin is not None:
            from .boundary import RobinBC
            (robin if isinstance(robin, RobinBC) else RobinBC(V, self.knots, robin, nquad=nquad)).apply(self)
        if dirichlet is not None:
            self.set_dirichlet(dirichlet)

    def diagonal(self) -> torch.Tensor:
        """diag(A) of the interior rows as a device tensor of the grid's shape (the
        stored diagonal ``Σ_q w (c φ_i² + a |∇φ_i|²)`` the Jacobi epilogue divides by)."""
        if self._diag is None:
            V = self.space
            host = np.empty(V.npts)
            _lib.call("poms_op_diagonal", self._h, host.ctypes.data_as(C.c_void_p))
            self._diag = torch.from_numpy(host).to(f"cuda:{V.device}")
        return self._diag

    def device_bytes(self) -> int:
        """Bytes of device memory the operator holds (coefficient arrays, diagonal)."""
        n = int(np.prod(self.space.npts)) * 8
        for t in (self._aq, self._cq):
            if t is not None:
                n += t.numel() * 8
        return n

    def assemble(self):
        """The stored stencil :func:`~poms_amd.assembly.assemble_stencil` forms from the
        same arguments (for cross-checks and host-side views)."""
        a, c = self._args
        to_np = lambda f: f.cpu().numpy() if isinstance(f, torch.Tensor) else f
        # (a tensor coefficient goes on as the device array the operator holds)
        B = assemble_stencil(self.space, self.knots, a=self._aq if self.tensor else to_np(a), c=to_np(c),
                             mass_coef=self.mass_coef, nquad=self.nquad)
        for face, S in self._face_terms:   # (the same face terms, before the mask)
            add_face_term(B, face, S)
        if self.dirichlet is not None:
            B.set_dirichlet(self.dirichlet)
        return B

    def _no_matrix(self, what):
        raise NotImplementedError(f"a matrix-free operator stores no coefficients: {what} is not available; "
                                  "use .assemble() for the stored stencil of the same arguments")

    def tosparse(self):
        self._no_matrix("tosparse()")

    def tocsr(self):
        self._no_matrix("tocsr()")

    def toarray(self):
        self._no_matrix("toarray()")

    def __getitem__(self, key):
        self._no_matrix("element access")

    def diagonal_axes(self):
        raise NotImplementedError("a matrix-free operator has no per-axis factors; use .diagonal()")


class MatrixFreeVCycle(GalerkinVCycle):
    """:class:`~poms_amd.mg.GalerkinVCycle`'s cycle with a matrix-free finest level:
    ``ops[0]`` is a :class:`MatrixFreeOperator`, ``ops[1]`` the stencil assembled on
    level 1's knots, ``ops[l ≥ 2] = galerkin_stencil(ops[l-1], P[l-1])``, and the
    coarsest level is inverted densely.  The sequence of a level is the base's
    ``_level``, unchanged.

    Level 1 is a *rediscretisation*, not a Galerkin product: it equals ``PᵀA₀P``
    exactly when ``a`` and ``c`` are integrated exactly on both levels (polynomials of
    degree ≤ 1 per axis at ``nquad = p+1``), and to quadrature accuracy otherwise.
    Below level 1 the coarse operators are Galerkin products of it.

    ``A``: the finest operator; ``P[l]``: the 1D prolongations from level ``l+1`` to
    ``l``; ``A1``: the level-1 :class:`~poms_amd.stencil.StencilMatrix` (on the space
    of ``P[0]``'s columns)."""

    def __init__(self, A: MatrixFreeOperator, P, A1, *, tol: float = 1e-6, maxiters=None, **smoother_kw):
        if tuple(A1.space.npts) != tuple(np.shape(p)[1] for p in P[0]):
            raise ValueError("the level-1 operator does not live on the columns of P[0]")
        self._A1 = A1
        super().__init__(A, P, tol=tol, maxiters=maxiters, **smoother_kw)

    def _coarse_op(self, l: int):
        return self._A1 if l == 0 else super()._coarse_op(l)

    @classmethod
    def uniform(cls, p: int, ncells_fine: int, ncells_coarsest: int = 8, ndim: int = 3, *, a=None, c=None,
                mass_coef: float = 1.0, nquad: int | None = None, device=None, tol: float = 1e-6, maxiters=None,
                mapping=None, dirichlet=None, robin=None, **smoother_kw):
        """Dyadic uniform hierarchy, as :meth:`GalerkinVCycle.uniform`.  ``a`` / ``c``:
        None, scalars or callables (they are sampled on two quadrature grids, the
        finest level's and level 1's).  ``mapping``: the operator of the mapped domain
        (:mod:`poms_amd.geometry`), its tensor sampled on those two grids; ``a`` / ``c``
        are then functions of the physical coordinates.  ``robin``: ``{(axis, side): β}``, β a
        scalar or a callable (:class:`~poms_amd.boundary.RobinBC`), sampled on both levels too:
        level 1 is rediscretised with the same ``robin`` on its own knots.  ``smoother_kw``:
        ``smoother``, ``cheby_degree``, ``cheby_ratio``, ``cheby_safety`` of
        :class:`~poms_amd.mg.GalerkinVCycle`."""
        from .boundary import RobinBC
        for f in (a, c):
            if f is not None and not callable(f) and np.ndim(f) != 0:
                raise ValueError("a / c must be None, scalars or callables here: they are sampled on two grids")
        cells, knots, P1, V = uniform_hierarchy(p, ncells_fine, ncells_coarsest, ndim, device)
        a1, c1 = a, c
        if mapping is not None:
            pull = lambda T: mapping.pullback([axis_tables(T, p, nquad)["points"].reshape(-1)] * ndim, a=a, c=c,
                                              mass_coef=mass_coef, device=f"cuda:{V.device}")[:2]
            (a, c), (a1, c1) = pull(knots[0]), pull(knots[1])
        V1 = StencilVectorSpace([len(knots[1]) - p - 1] * ndim, [p] * ndim, device=V.device, align=True)
        r0 = r1 = None
        if robin:
            r0 = RobinBC(V, [knots[0]] * ndim, robin, mapping=mapping, nquad=nquad)
            r1 = RobinBC(V1, [knots[1]] * ndim, robin, mapping=mapping, nquad=nquad)
        A = MatrixFreeOperator(V, [knots[0]] * ndim, a=a, c=c, mass_coef=mass_coef, nquad=nquad, dirichlet=dirichlet,
                               robin=r0)
        A1 = assemble_stencil(V1, [knots[1]] * ndim, a=a1, c=c1, mass_coef=mass_coef, nquad=nquad, robin=r1)
        mg = cls(A, [[P1l] * ndim for P1l in P1], A1, tol=tol, maxiters=maxiters, **smoother_kw)
        mg.p, mg.ndim, mg.cells, mg.knots, mg.P1 = int(p), int(ndim), cells, knots, P1
        return mg
