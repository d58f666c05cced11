"""Two-level B-spline multigrid V-cycle (`sources/mg_jac.py`), on the device.

Set-up (host, once) follows `sources/mg_jac.py:25-81`:
coarse knots ``Tc``, fine knots ``Tf``, inserted knots
``Ts = knots_to_insert(Tf, nf, p, Tc, nc, p)``, fine space on
``T = sort(Tc ∪ Ts)``, operator ``-Δu + u``, ``P1 = matrix_multi_stages(Ts,
nc, p, Tc)``, ``R1 = P1^T``, Galerkin ``Ac = R Af P``.  Because every factor
is a Kronecker product, ``Ac = Σ_t ⊗_d (P1^T F_{t,d} P1)`` exactly; it is
factorised on the host (the reference's ``splu``) and its inverse applied on
the device.

Cycle (`sources/mg_jac.py:84-119`):
    xf, info_pre = pcg(Af, damped_jacobi, bf, tol, maxiter)     # pre-smoothing
    rc = R (bf - Af xf) (+ all-reduce over slabs)                 # residual -> restriction, fused
    xc = Ac^{-1} rc                                               # coarse solve
    xf = xf + P xc ; ghost exchange                               # correction
    xf2, info_pos = pcg(Af, damped_jacobi, bf, x0=xf, tol, maxiter)  # post-smoothing

``post_smoother="glt"`` runs `sources/mg_glt.py:113-123` instead: the post-smoother
is ``pcg_glt(Af, M1, M2, bf, x0=xf, tol, maxiter=p+1)``, preconditioned by the
Kronecker direct solve with the cardinal-spline collocation matrices
(``collocation_cardinal_splines(p, n)`` per axis, `sources/mg_glt.py:115-118`).

Grid convention: ``ncells_fine`` / ``ncells_coarse`` count CELLS; the knot
vectors have ``n = N + p`` basis functions.  (The reference passes ``nc = 8``
as a number of basis functions to ``make_open_knots``; with a uniform fine
grid of 512 cells that would make the union knot vector non-uniform, so the
benchmark nests an 8-cell coarse grid instead.  Both conventions are
supported through ``knots_coarse`` / ``knots_fine``.)
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import scipy.linalg as sla
import torch

from . import _lib
from . import runtime as rt
from .boundary import check_unit_rows, constrain_dense, constrain_prolongation, normalize_faces
from .multilevels import KronTransfer, knots_to_insert
from .solvers import (_cached_lmax, chebyshev, chebyshev_work, damped_jacobi, defer_x_count, pcg,
                      pcg_kron)
from .splines import (array_to_mat_stencil, assemble_1d, band_to_dense, collocation_cardinal_splines,
                      matrix_multi_stages, uniform_knots)
from .stencil import F64, KronOperator, StencilVector, StencilVectorSpace


def two_level_setup_1d(p: int, Tf: np.ndarray, Tc: np.ndarray):
    """1D pieces of the two-level hierarchy: fine knots T, inserted knots Ts, P1 (nf x nc)."""
    nf = len(Tf) - p - 1
    nc = len(Tc) - p - 1
    Ts = knots_to_insert(Tf, nf, p, Tc, nc, p)
    T = np.sort(np.concatenate([Tc, Ts]))
    P1 = matrix_multi_stages(Ts, nc, p, Tc)
    return T, Ts, P1


def galerkin_coarse_dense(Mc, Kc, ndim: int, mass_coef: float = 1.0) -> np.ndarray:
    """Dense ``Ac = c Mc⊗Mc(⊗Mc) + Σ_d (Kc on axis d, Mc elsewhere)``; ``Mc`` / ``Kc``: one
    matrix for every axis, or a list of one per axis."""
    def kr(ms):
        out = ms[0]
        for m in ms[1:]:
            out = np.kron(out, m)
        return out

    Mc = list(Mc) if isinstance(Mc, (list, tuple)) else [Mc] * ndim
    Kc = list(Kc) if isinstance(Kc, (list, tuple)) else [Kc] * ndim
    A = mass_coef * kr(Mc)
    for d in range(ndim):
        A = A + kr([Kc[e] if e == d else Mc[e] for e in range(ndim)])
    return A


def dyadic_cells(ncells_fine: int, ncells_coarsest: int) -> list:
    """Cells per axis of every level: ``ncells_fine`` halved while it is even and the
    half is not below ``ncells_coarsest``."""
    if ncells_fine < ncells_coarsest or ncells_coarsest < 1:
        raise ValueError("need ncells_fine >= ncells_coarsest >= 1")
    cells = [int(ncells_fine)]
    while cells[-1] % 2 == 0 and (half := cells[-1] // 2) >= ncells_coarsest:
        cells.append(half)
    if len(cells) < 2:
        raise ValueError("the hierarchy needs at least two levels (even cell counts)")
    return cells


def uniform_hierarchy(p: int, ncells_fine: int, ncells_coarsest: int, ndim: int, device=None):
    """``(cells, knots, P1, V)`` of the dyadic uniform hierarchy: the cells and knots of
    every level, the 1D prolongations between them, and the finest level's space."""
    cells = dyadic_cells(ncells_fine, ncells_coarsest)
    knots = [uniform_knots(p, N) for N in cells]
    P1 = [two_level_setup_1d(p, knots[l], knots[l + 1])[2] for l in range(len(cells) - 1)]
    V = StencilVectorSpace([len(knots[0]) - p - 1] * ndim, [p] * ndim, device=device, align=True)
    return cells, knots, P1, V


def _constrained_P(P, faces):
    """The per-axis prolongations the transfers of a constrained hierarchy are built from:
    ``P_d Π_cd`` after :func:`~poms_amd.boundary.check_unit_rows` (``P`` itself without faces)."""
    if faces is None:
        return list(P)
    check_unit_rows(P, faces)
    return [constrain_prolongation(Pd, lo, hi) for Pd, (lo, hi) in zip(P, faces)]


def _kron_dirichlet(dirichlet, ndim: int, dist, post_smoother: str = "jacobi"):
    """The faces of a Kronecker V-cycle, after the combinations it does not implement."""
    faces = normalize_faces(dirichlet, ndim)
    if faces is not None and dist is not None:
        raise NotImplementedError("dirichlet: distributed (slab / Cart) V-cycles are not supported")
    if faces is not None and post_smoother == "glt":
        raise NotImplementedError("dirichlet: the GLT post-smoother is not supported")
    return faces


def _smoother_counts(maxiters, nlevels: int) -> list:
    out = [10] * (nlevels - 1) if maxiters is None else [int(m) for m in maxiters]
    if len(out) != nlevels - 1:
        raise ValueError(f"maxiters needs {nlevels - 1} entries")
    return out


def _check_smoother(smoother: str, dist=None, post_smoother: str = "jacobi") -> str:
    """The smoother's name, after the combinations the Chebyshev smoother does not implement."""
    if smoother not in ("jacobi", "chebyshev"):
        raise ValueError("smoother must be 'jacobi' (pcg with damped Jacobi, mg_jac.py) or 'chebyshev'")
    if smoother == "chebyshev" and dist is not None:
        raise ValueError("smoother='chebyshev': distributed (slab / Cart) V-cycles are not supported")
    if smoother == "chebyshev" and post_smoother == "glt":
        raise ValueError("smoother='chebyshev': the GLT post-smoother is not supported")
    return smoother


class _VCycle:
    """What the V-cycles share: the sequence of one level, the right-hand side of ones and
    the dense solve on the coarsest level.  A constructor sets ``tol`` and, per level with
    a coarser one below it, ``ops``, ``spaces``, ``transfers``, ``fused`` (residual ->
    restriction in one pass) and ``maxiters``, then calls :meth:`_set_coarse` and, for a
    smoother other than the default, :meth:`_set_smoother`.

    ``smoother="chebyshev"`` replaces both ``pcg(A_l, damped_jacobi, b_l)`` calls of a level
    by :func:`~poms_amd.solvers.chebyshev` of degree ``cheby_degree`` (an int, or one per
    level) over ``[cheby_safety lmax / cheby_ratio, cheby_safety lmax]``, lmax(D^-1 A_l)
    estimated once at construction.  The same polynomial runs before and after the coarse
    correction and there are no stop tests, so the cycle from zero is a fixed symmetric
    linear operator: :meth:`preconditioner` hands it to ``solvers.pcg``."""

    glt = None   # level 0's post-smoother factors where it is pcg_kron (TwoLevelVCycle)
    smoother = "jacobi"

    def _set_smoother(self, smoother: str, cheby_degree=10, cheby_ratio: float = 30.0,
                      cheby_safety: float = 1.1) -> None:
        self.smoother = smoother
        if smoother != "chebyshev":
            return
        L = len(self.transfers)
        degs = [int(cheby_degree)] * L if np.ndim(cheby_degree) == 0 else [int(d) for d in cheby_degree]
        if len(degs) != L or min(degs) < 1:
            raise ValueError(f"cheby_degree needs one integer >= 1, or {L} of them")
        self.cheby_degrees, self.cheby_ratio, self.cheby_safety = degs, float(cheby_ratio), float(cheby_safety)
        self.cheby_lmax = [_cached_lmax(A) for A in self.ops[:L]]
        self._cheby_work = [chebyshev_work(A) for A in self.ops[:L]]

    def preconditioner(self):
        """``psolve`` for :func:`~poms_amd.solvers.pcg`: one cycle from zero on ``r``.  A
        legitimate CG preconditioner with ``smoother="chebyshev"`` only (a pcg-smoothed
        cycle is not a fixed linear operator)."""
        return lambda A, r: self.cycle(r)[0]

    def _set_coarse(self, Ac: np.ndarray) -> None:
        """The coarsest level from its dense operator: the inverse (the reference's
        ``splu``) applied on the device, and the coarse vectors of every level."""
        self.Ac = Ac
        Ainv = sla.lu_solve(sla.lu_factor(Ac), np.eye(Ac.shape[0]))
        dev = f"cuda:{self.space.device}"
        self.Ainv = torch.from_numpy(np.ascontiguousarray(Ainv)).to(dev)
        self.rcs = [torch.empty(tr.ncoarse, dtype=F64, device=dev) for tr in self.transfers]
        self.xc = torch.empty(Ac.shape[0], dtype=F64, device=dev)
        self.infos = [None] * len(self.transfers)

    @property
    def nlevels(self) -> int:
        return len(self.transfers) + 1

    @property
    def ndof(self) -> int:
        return self.space.dimension

    @property
    def space(self) -> StencilVectorSpace:
        return self.spaces[0]

    @property
    def A(self) -> KronOperator:
        return self.ops[0]

    def rhs_ones(self) -> StencilVector:
        """``bf[i] = 1`` on every owned coefficient (`sources/mg_jac.py:57-62`)."""
        b = self.space.empty()
        _lib.call("poms_vec_fill", self.space.ctx, C.byref(self.space.layout), 1.0, rt.ptr(b._data),
                  rt.stream_handle())
        b._mark_written()
        b.update_ghost_regions()
        return b

    def coarse_solve(self, rc: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        _lib.call("poms_dense_matvec", self.space.ctx, rc.numel(), rt.ptr(self.Ainv), rt.ptr(rc),
                  rt.ptr(out), rt.stream_handle())
        return out

    def _level(self, l: int, b: StencilVector, x0: StencilVector | None) -> StencilVector:
        A, tr, n = self.ops[l], self.transfers[l], self.maxiters[l]
        cheby = self.smoother == "chebyshev"
        if cheby:
            ckw = dict(degree=self.cheby_degrees[l], lmax=self.cheby_lmax[l], ratio=self.cheby_ratio,
                       safety=self.cheby_safety, work=self._cheby_work[l])
            x, ipre = chebyshev(A, b, x0=x0, **ckw)
        else:
            # (_skip_tail: a smoother call's last iteration ends at x and r.r, see solvers.pcg)
            # (_defer_x: x brought up to date once per call where that pays, see solvers.defer_x_count)
            dx = defer_x_count(A, self.spaces[l], n)
            x, ipre = pcg(A, damped_jacobi, b, x0=x0, tol=self.tol, maxiter=n, _skip_tail=True, _defer_x=dx,
                          _fold_r=True)
        if self.fused[l]:
            rc = tr.resid_restrict(A, b, x, out=self.rcs[l])
        else:
            rc = tr.restrict(A.residual(b, x), out=self.rcs[l])
        if l + 1 == len(self.transfers):
            ec = self.coarse_solve(rc, self.xc)
        else:
            Vc = self.spaces[l + 1]
            bc = Vc.empty()
            Vc.interior(bc._data).copy_(rc.view(Vc.local_npts))
            bc._mark_written()
            bc.update_ghost_regions()
            ecv = self._level(l + 1, bc, None)
            ec = Vc.interior(ecv._data).contiguous().view(-1)
        tr.prolong_add(ec, x)
        x.update_ghost_regions()
        if cheby:
            # (the same polynomial as before the correction, continued in the level's buffers;
            # level 0's result leaves them, so that the caller owns what it gets)
            x, ipos = chebyshev(A, b, x0=x, _x0_owned=True, **ckw)
            if l == 0:
                x = x.copy()
        elif l == 0 and self.glt is not None:
            x, ipos = pcg_kron(A, self.glt, b, x0=x, tol=self.tol, maxiter=self.p + 1, _skip_tail=True)
        else:
            # (x is this cycle's own temporary, never the caller's x0: iterate in its buffer, no copy)
            x, ipos = pcg(A, damped_jacobi, b, x0=x, tol=self.tol, maxiter=n, _x0_owned=True, _skip_tail=True,
                          _defer_x=dx, _fold_r=True)
        if self.infos[l] is None:
            self.infos[l] = (ipre, ipos)
        return x

    def cycle(self, b: StencilVector, x0: StencilVector | None = None):
        """One V-cycle from level 0; returns ``(x, infos)``, ``infos[l] = (info_pre,
        info_post)`` of level l's first visit in this cycle."""
        self.infos = [None] * len(self.transfers)
        x = self._level(0, b, x0)
        return x, list(self.infos)


class TwoLevelVCycle(_VCycle):
    """Two-level V-cycle on an ``ndim``-D tensor B-spline space of degree ``p``."""

    def __init__(self, p: int, ncells_fine: int, ncells_coarse: int = 8, ndim: int = 3, *,
                 dist=None, mass_coef: float = 1.0, device=None, knots_fine=None, knots_coarse=None,
                 tol: float = 1e-6, maxiter: int = 10, chunk: int = 0, align: bool = True,
                 post_smoother: str = "jacobi", fused_restrict: bool | None = None, dirichlet=None,
                 smoother: str = "jacobi", cheby_degree=10, cheby_ratio: float = 30.0, cheby_safety: float = 1.1):
        self.p, self.ndim = int(p), int(ndim)
        if post_smoother not in ("jacobi", "glt"):
            raise ValueError("post_smoother must be 'jacobi' (mg_jac.py) or 'glt' (mg_glt.py)")
        _check_smoother(smoother, dist, post_smoother)
        self.post_smoother = post_smoother
        # Dirichlet faces: constrained 1D factors on both levels, transfers from P Π_c, and
        # the coarse factors constrain(P^T F P) (not (PΠ)^T F~ (PΠ), which is singular)
        self.dirichlet = faces = _kron_dirichlet(dirichlet, ndim, dist, post_smoother)
        Tc = uniform_knots(p, ncells_coarse) if knots_coarse is None else np.asarray(knots_coarse, float)
        Tf = uniform_knots(p, ncells_fine) if knots_fine is None else np.asarray(knots_fine, float)
        T, Ts, P1 = two_level_setup_1d(p, Tf, Tc)
        self.Tc, self.Tf, self.T, self.Ts, self.P1 = Tc, Tf, T, Ts, P1
        self.n = n = len(T) - p - 1
        self.M1d, self.K1d = M, K = assemble_1d(T, p)
        # line-aligned rows (pitch a multiple of 16 doubles): the v5 operator kernel
        # then stores whole 128-B lines only
        V = StencilVectorSpace([n] * ndim, [p] * ndim, dist=dist, device=device, align=align)
        A = KronOperator.laplace(V, [M] * ndim, [K] * ndim, mass_coef=mass_coef, dirichlet=faces)
        if chunk:
            A.set_chunk(chunk)
        self.spaces, self.ops, self.transfers = [V], [A], [KronTransfer(V, _constrained_P([P1] * ndim, faces))]
        # residual -> restriction in one pass over x and b (KronTransfer.resid_restrict);
        # False: the residual vector and the restriction, as the reference computes them.
        # None: fused in 3D (515^3: 0.70 ms against 0.92 for the pair), not in 2D, where
        # the passes are latency-bound (1027^2: 44.8 against 42.5 us)
        if fused_restrict is None:   # (POMS_FUSED_RESTRICT: 0 never, all in every dimension)
            fr = os.environ.get("POMS_FUSED_RESTRICT", "1")
            fused_restrict = fr == "all" or (ndim == 3 and fr != "0")
        self.fused = [bool(fused_restrict) and self.transfer.set_operator(A)]
        Md, Kd = band_to_dense(M), band_to_dense(K)
        Mc, Kc = [P1.T @ Md @ P1] * ndim, [P1.T @ Kd @ P1] * ndim
        if faces is not None:
            Mc = [constrain_dense(m, m.shape[:1], [f]) for m, f in zip(Mc, faces)]
            Kc = [constrain_dense(k, k.shape[:1], [f]) for k, f in zip(Kc, faces)]
        self._set_coarse(galerkin_coarse_dense(Mc, Kc, ndim, mass_coef))
        self.tol, self.maxiters = tol, [maxiter]
        if post_smoother == "glt":
            Cm = array_to_mat_stencil(n, p, collocation_cardinal_splines(p, n))
            self.glt = [Cm] * ndim
        self._set_smoother(smoother, cheby_degree, cheby_ratio, cheby_safety)

    # the one level's entries of the base's lists, under the names of `sources/mg_jac.py`
    transfer = property(lambda self: self.transfers[0])
    rc = property(lambda self: self.rcs[0])
    maxiter = property(lambda self: self.maxiters[0], lambda self, m: self.maxiters.__setitem__(0, m))
    fused_restrict = property(lambda self: self.fused[0], lambda self, f: self.fused.__setitem__(0, bool(f)))

    def cycle(self, bf: StencilVector, x0: StencilVector | None = None):
        """One V-cycle; returns ``(xf2, info_pre, info_pos)``."""
        self.infos = [None]
        return (self._level(0, bf, x0),) + self.infos[0]


class MultilevelVCycle(_VCycle):
    """V-cycle over a hierarchy of nested uniform B-spline spaces (SURVEY §8f
    rank 1: the reference's two-level cycle `sources/mg_jac.py:84-119` applied
    recursively, with every level's operator, smoothing and transfers on the
    device and a dense device solve on the coarsest level).

    Level 0 has ``ncells_fine`` cells per axis; each coarser level halves the
    cells (dyadic knot insertion, ``P1 = matrix_multi_stages``) down to
    ``ncells_coarsest``.  Level operators are assembled on their own knots; for
    nested spaces with exact quadrature that IS the Galerkin product R A P of
    the reference (pinned by tests/test_splines.py and the oracle parity test).
    Each level is smoothed by ``pcg(A_l, damped_jacobi, b_l, tol, maxiters[l])``
    before and after the coarse correction, as the reference smooths its fine
    level.  With ``dist`` the finest level is slab-decomposed; the restriction
    to level 1 is all-reduced and the coarser levels are replicated on every
    rank (their work is 1/8, 1/64, ... of the finest level's).
    """

    def __init__(self, p: int, ncells_fine: int, ncells_coarsest: int = 8, ndim: int = 3, *,
                 dist=None, mass_coef: float = 1.0, device=None, tol: float = 1e-6, maxiters=None,
                 align: bool = True, chunk: int = 0, fused_restrict: bool | None = None, dirichlet=None,
                 smoother: str = "jacobi", cheby_degree=10, cheby_ratio: float = 30.0, cheby_safety: float = 1.1):
        _check_smoother(smoother, dist)
        self.cells = cells = dyadic_cells(ncells_fine, ncells_coarsest)
        self.dirichlet = faces = _kron_dirichlet(dirichlet, ndim, dist)   # (as TwoLevelVCycle)
        self.p, self.ndim, self.tol = int(p), int(ndim), tol
        L = len(cells)
        self.maxiters = _smoother_counts(maxiters, L)
        self.knots = knots = [uniform_knots(p, N) for N in cells]
        self.P1 = [two_level_setup_1d(p, knots[l], knots[l + 1])[2] for l in range(L - 1)]
        self.M1d, self.K1d = (list(f) for f in zip(*[assemble_1d(T, p) for T in knots]))
        self.spaces, self.ops, self.transfers = [], [], []
        for l in range(L - 1):
            V = StencilVectorSpace([len(knots[l]) - p - 1] * ndim, [p] * ndim, dist=dist if l == 0 else None,
                                   device=device, align=align)
            A = KronOperator.laplace(V, [self.M1d[l]] * ndim, [self.K1d[l]] * ndim, mass_coef=mass_coef,
                                     dirichlet=faces)
            if chunk:
                A.set_chunk(chunk)
            self.spaces.append(V)
            self.ops.append(A)
            self.transfers.append(KronTransfer(V, _constrained_P([self.P1[l]] * ndim, faces)))
        # fused residual -> restriction where the transfer is dense (coarse extents <= 32);
        # None: in 3D (as TwoLevelVCycle)
        if fused_restrict is None:
            fused_restrict = ndim == 3
        self.fused = [bool(fused_restrict) and tr.set_operator(A) for tr, A in zip(self.transfers, self.ops)]
        # coarsest level: its operator assembled on its knots (= Galerkin, nested)
        Mc, Kc = [band_to_dense(self.M1d[-1])] * ndim, [band_to_dense(self.K1d[-1])] * ndim
        if faces is not None:
            Mc = [constrain_dense(m, m.shape[:1], [f]) for m, f in zip(Mc, faces)]
            Kc = [constrain_dense(k, k.shape[:1], [f]) for k, f in zip(Kc, faces)]
        self._set_coarse(galerkin_coarse_dense(Mc, Kc, ndim, mass_coef))
        self._set_smoother(smoother, cheby_degree, cheby_ratio, cheby_safety)


class GalerkinVCycle(_VCycle):
    """V-cycle for a general (variable-coefficient) stencil operator with Galerkin
    coarse operators, as the reference builds its own (`sources/mg_jac.py:80-81`,
    ``Ac = R Af P`` of the assembled matrix): ``ops[l+1] = P_l^T ops[l] P_l`` formed on
    the device (:func:`~poms_amd.multilevels.galerkin_stencil`), every level smoothed
    by ``pcg(A_l, damped_jacobi, b_l, tol, maxiters[l])`` before and after the coarse
    correction (the base's ``_level`` sequence; residual and restriction are
    two launches, there is no fused pass for stencils) and a dense solve on the
    coarsest level.

    ``A``: the finest :class:`~poms_amd.stencil.StencilMatrix`; ``P[l]``: the list of
    1D prolongations, one per axis, from level ``l+1`` to level ``l``.

    A constrained ``A`` (``A.dirichlet``) constrains the hierarchy: every coarse operator
    gets the same faces, the transfers are built from ``P Π_c`` and the coarsest inverse
    from the constrained dense matrix.  The Galerkin products still run on the stored
    coefficients with the full ``P``: where the boundary rows of ``P`` are unit vectors
    (checked), ``Π_c (PᵀAP) Π_c = (PΠ_c)ᵀ (Π_f A Π_f) (PΠ_c)``.
    """

    def __init__(self, A, P, *, tol: float = 1e-6, maxiters=None, smoother: str = "jacobi", cheby_degree=10,
                 cheby_ratio: float = 30.0, cheby_safety: float = 1.1):
        if len(P) < 1:
            raise ValueError("the hierarchy needs at least two levels")
        _check_smoother(smoother)
        self.tol = tol
        self.maxiters = _smoother_counts(maxiters, len(P) + 1)
        self.P = [[np.ascontiguousarray(p, dtype=np.float64) for p in Pl] for Pl in P]
        self.ops, self.spaces, self.transfers = [A], [A.space], []
        self.dirichlet = faces = A.dirichlet
        for l in range(len(P)):
            Pt = _constrained_P(self.P[l], faces)
            Ac = self._coarse_op(l)
            if Ac.dirichlet != faces:
                Ac.set_dirichlet(faces)
            self.transfers.append(KronTransfer(self.spaces[l], Pt))
            self.ops.append(Ac)
            self.spaces.append(Ac.space)
        self.fused = [False] * len(P)
        # coarsest level: its Galerkin operator, inverted densely
        self._set_coarse(self.ops[-1].toarray())
        self._set_smoother(smoother, cheby_degree, cheby_ratio, cheby_safety)

    def _coarse_op(self, l: int):
        """Level ``l+1``'s operator from level ``l``'s (subclasses may rediscretise)."""
        from .multilevels import galerkin_stencil
        return galerkin_stencil(self.ops[l], self.P[l])

    @classmethod
    def uniform(cls, p: int, ncells_fine: int, ncells_coarsest: int = 8, ndim: int = 3, *, a=None, c=None,
                mass_coef: float = 1.0, device=None, tol: float = 1e-6, maxiters=None, mapping=None,
                dirichlet=None, robin=None, **smoother_kw):
        """Dyadic uniform hierarchy (as :class:`MultilevelVCycle`'s) under
        ``-∇·(a∇u) + c u`` assembled on the finest knots by
        :func:`~poms_amd.assembly.assemble_stencil`.  ``mapping`` (a
        :class:`~poms_amd.geometry.Mapping` or ``SplineMapping``): the operator of the
        mapped domain, its tensor sampled on the finest quadrature grid (``a`` / ``c``
        are then functions of the physical coordinates).  ``robin``: ``{(axis, side): β}``, β a
        scalar or a callable (:class:`~poms_amd.boundary.RobinBC`), sampled on the finest level
        only: the coarse operators are Galerkin products of the stored ``A + S``.
        ``smoother_kw``: ``smoother``, ``cheby_degree``, ``cheby_ratio``, ``cheby_safety`` of the
        constructor."""
        from .assembly import assemble_stencil, axis_tables
        from .boundary import RobinBC
        _check_smoother(smoother_kw.get("smoother", "jacobi"))
        cells, knots, P1, V = uniform_hierarchy(p, ncells_fine, ncells_coarsest, ndim, device)
        if mapping is not None:
            pts = axis_tables(knots[0], p)["points"].reshape(-1)
            a, c, _ = mapping.pullback([pts] * ndim, a=a, c=c, mass_coef=mass_coef, device=f"cuda:{V.device}")
        rb = RobinBC(V, [knots[0]] * ndim, robin, mapping=mapping) if robin else None
        A = assemble_stencil(V, [knots[0]] * ndim, a=a, c=c, mass_coef=mass_coef, dirichlet=dirichlet, robin=rb)
        mg = cls(A, [[P1l] * ndim for P1l in P1], tol=tol, maxiters=maxiters, **smoother_kw)
        mg.p, mg.ndim, mg.cells, mg.knots, mg.P1 = int(p), int(ndim), cells, knots, P1
        return mg

