"""Generalised eigenproblems ``A x = λ B x`` on the device: LOBPCG over block vector algebra.

* :func:`block_gram` -- the Gram matrix ``Xᵀ Y`` of two lists of vectors in one pass
  (``poms_block_gram``: 4 x 4 register tiles, ordered reduction, the same bits every call);
* :func:`block_combine` -- linear combinations ``out_j = Σ_i C[i, j] in_i`` of a list of
  vectors in one pass (``poms_block_combine``: every input read once for all outputs);
* :func:`rayleigh_ritz` -- the small dense eigenproblem of a basis, on the host (NumPy /
  SciPy only: it needs no device);
* :func:`lobpcg` -- Knyazev's locally optimal block preconditioned conjugate gradient method
  for the ``k`` lowest eigenpairs, with any ``pcg`` preconditioner (``solvers.jacobi``,
  ``vc.preconditioner()``).

The reference has no eigensolver; the operators, mass matrices and preconditioners are
the ones it solves ``A u = f`` with.
"""
from __future__ import annotations

import numpy as np

EPS = 2.0 ** -52
BLOCK_MAX = 24          # POMS_BLOCK_MAX: vectors per list of a block operation
COMBINE_MAX_OUT = 16    # outputs of one poms_block_combine

#: :func:`lobpcg` drops ``P`` from the basis for an iteration (a *restart*: ``S = [X W]``)
#: when the Gram matrix ``SᵀBS`` of ``S = [X W P]``, scaled to a unit diagonal, has a
#: condition number above this, or is not numerically positive definite.  The Ritz values
#: of a basis of condition κ carry a relative error of about κ EPS of the largest one;
#: 1e8 keeps that below 1e-8 and is reached only where ``P`` has become a combination of
#: ``X`` and ``W`` to half the working precision, i.e. when it no longer adds a direction.
RESTART_COND = 1e8


class GramNotPositiveDefinite(np.linalg.LinAlgError):
    """:func:`rayleigh_ritz`: the Gram matrix ``H`` of the basis is not numerically positive
    definite (scaled to a unit diagonal, its smallest eigenvalue is at most ``n EPS`` times
    its largest): the basis vectors are linearly dependent to working precision."""


def rayleigh_ritz(G, H, m):
    """The ``m`` lowest Ritz pairs of a basis ``S`` from ``G = SᵀAS`` and ``H = SᵀBS``
    (symmetric ``n x n``, ``H`` positive definite): ``(theta, C, cond)`` with ``theta`` the
    ``m`` lowest eigenvalues of ``G c = θ H c`` in ascending order, ``C`` (``n x m``) their
    eigenvectors, ``CᵀHC = I``, in terms of the *unscaled* basis, and ``cond`` the condition
    number of ``D H D``, ``D = diag(H)^-½``.

    Both matrices are scaled by ``D`` first (the Ritz values do not depend on the lengths of
    the basis vectors; the conditioning of the small problem does), symmetrised, and handed
    to ``scipy.linalg.eigh(D G D, D H D)``.  Raises :class:`GramNotPositiveDefinite` when
    ``D H D`` is not numerically positive definite (or ``diag(H)`` is not positive)."""
    import scipy.linalg as sla
    G = np.asarray(G, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64)
    n = G.shape[0]
    if G.shape != (n, n) or H.shape != (n, n) or not 1 <= int(m) <= n:
        raise ValueError(f"rayleigh_ritz: G and H must be n x n and 1 <= m <= n, got {G.shape}, {H.shape}, m = {m}")
    h = np.diag(H)
    if not np.all(np.isfinite(G)) or not np.all(np.isfinite(H)) or not np.all(h > 0.0):
        raise GramNotPositiveDefinite("rayleigh_ritz: diag(H) is not positive (or an entry is not finite)")
    d = 1.0 / np.sqrt(h)
    Gs = d[:, None] * G * d[None, :]
    Hs = d[:, None] * H * d[None, :]
    Gs = 0.5 * (Gs + Gs.T)
    Hs = 0.5 * (Hs + Hs.T)
    w = np.linalg.eigvalsh(Hs)
    if not w[0] > n * EPS * w[-1]:
        raise GramNotPositiveDefinite(
            f"rayleigh_ritz: the scaled Gram matrix is not positive definite (eigenvalues {w[0]:.3e} .. {w[-1]:.3e})")
    cond = float(w[-1] / w[0])
    try:
        theta, Z = sla.eigh(Gs, Hs)
    except np.linalg.LinAlgError as exc:   # (the Cholesky factorisation of Hs broke down)
        raise GramNotPositiveDefinite(f"rayleigh_ritz: {exc}") from exc
    m = int(m)
    return theta[:m].copy(), d[:, None] * Z[:, :m], cond


# ---- block operations on the device ----------------------------------------------------

def _space_of(vectors, what):
    from .stencil import StencilVector
    vectors = list(vectors)
    if not vectors or not all(isinstance(v, StencilVector) for v in vectors):
        raise TypeError(f"{what}: a non-empty list of StencilVector")
    V = vectors[0].space
    if any(v.space is not V for v in vectors):
        raise ValueError(f"{what}: the vectors must belong to one StencilVectorSpace")
    return vectors, V


def _ptrs(vectors):
    import ctypes as C
    return (C.c_void_p * len(vectors))(*[v._data.data_ptr() for v in vectors])


def block_gram(xs, ys, symmetric=False, out=None):
    """``G[i, j] = xs[i] . ys[j]`` as a device tensor of shape ``(len(xs), len(ys))``, at most
    24 vectors per list, all of one (undistributed) space.  One pass: each vector is read
    once per 4 x 4 tile of ``G`` it belongs to, and two calls give the same bits.
    ``symmetric=True`` (equally long lists): the caller asserts ``G = Gᵀ`` (``ys = xs``, or
    ``ys[j] = A xs[j]`` with ``A`` symmetric); only the tiles on or above the diagonal are
    computed and the rest is mirrored, so ``G`` equals its transpose bitwise.  ``out``: a
    contiguous float64 device tensor of that shape to write into."""
    import ctypes as C
    import torch
    from . import _lib, runtime as rt
    xs, V = _space_of(xs, "block_gram")
    ys, Vy = _space_of(ys, "block_gram")
    if Vy is not V:
        raise ValueError("block_gram: the vectors must belong to one StencilVectorSpace")
    if V.dist is not None:
        raise NotImplementedError("block_gram: distributed (slab / Cart) spaces are not supported")
    if out is None:
        out = torch.empty((len(xs), len(ys)), dtype=torch.float64, device=xs[0]._data.device)
    elif out.shape != (len(xs), len(ys)) or out.dtype != torch.float64 or not out.is_contiguous():
        raise ValueError("block_gram: out must be a contiguous float64 tensor of shape (len(xs), len(ys))")
    _lib.call("poms_block_gram", V.ctx, C.byref(V.layout), len(xs), _ptrs(xs), len(ys), _ptrs(ys),
              1 if symmetric else 0, rt.ptr(out), rt.stream_handle())
    return out


def block_combine(ins, C, outs):
    """``outs[j] = Σ_i C[i, j] ins[i]`` (interior; at most 24 inputs and 16 outputs of one
    undistributed space).  ``C``: ``len(ins) x len(outs)``, a host array or a float64 device
    tensor.  Per element ``C[0, j] ins[0]`` first, then one fma per further input in order;
    every input is read once for all outputs.  No output may be an input or another output.
    Returns ``outs``."""
    import ctypes as Ct
    import torch
    from . import _lib, runtime as rt
    ins, V = _space_of(ins, "block_combine")
    outs, Vo = _space_of(outs, "block_combine")
    if Vo is not V:
        raise ValueError("block_combine: the vectors must belong to one StencilVectorSpace")
    if V.dist is not None:
        raise NotImplementedError("block_combine: distributed (slab / Cart) spaces are not supported")
    if not isinstance(C, torch.Tensor):
        C = torch.from_numpy(np.ascontiguousarray(np.asarray(C, dtype=np.float64)))
    if tuple(C.shape) != (len(ins), len(outs)):
        raise ValueError(f"block_combine: C must be {len(ins)} x {len(outs)}, got {tuple(C.shape)}")
    C = C.to(device=ins[0]._data.device, dtype=torch.float64).contiguous()
    _lib.call("poms_block_combine", V.ctx, Ct.byref(V.layout), len(ins), _ptrs(ins), len(outs), _ptrs(outs),
              rt.ptr(C), rt.stream_handle())
    for o in outs:
        o._mark_written()
    return outs


# ---- LOBPCG ------------------------------------------------------------------------------

def _check_k(k):
    if int(k) != k or k < 1:
        raise ValueError(f"lobpcg: k must be an integer >= 1, got {k}")
    if 3 * k > BLOCK_MAX:
        raise ValueError(f"lobpcg: the basis [X W P] of 3 k vectors must fit one block operation "
                         f"(3 k <= {BLOCK_MAX}), got k = {k}")
    return int(k)


def residual_norms(theta, raa, rbb, rrr):
    """LOBPCG's relative residuals ``‖r_j‖ / (‖A x_j‖ + |θ_j| ‖B x_j‖)`` from the squared norms
    (Gram diagonals) ``raa = ‖A x_j‖²``, ``rbb = ‖B x_j‖²``, ``rrr = ‖r_j‖²``."""
    den = np.sqrt(np.maximum(raa, 0.0)) + np.abs(theta) * np.sqrt(np.maximum(rbb, 0.0))
    return np.sqrt(np.maximum(rrr, 0.0)) / den


def ritz_step(G, H, k, have_p):
    """One Rayleigh-Ritz step of :func:`lobpcg` on the Gram matrices of ``S = [X W P]``
    (``3k x 3k``; ``2k x 2k`` without ``P``): ``(theta, C, cond, restarted)``.  With ``P`` in
    the basis and its ``H`` not positive definite or of condition above
    :data:`RESTART_COND`, the step is repeated on ``[X W]`` (``C`` then has zero rows for
    ``P``) and ``restarted`` is True."""
    n = G.shape[0]
    if have_p:
        try:
            theta, C, cond = rayleigh_ritz(G, H, k)
            if cond <= RESTART_COND:
                return theta, C, cond, False
        except GramNotPositiveDefinite:
            pass
        theta, C2, cond = rayleigh_ritz(G[:2 * k, :2 * k], H[:2 * k, :2 * k], k)
        C = np.zeros((n, k))
        C[:2 * k] = C2
        return theta, C, cond, True
    theta, C, cond = rayleigh_ritz(G, H, k)
    return theta, C, cond, False


def lobpcg(A, B=None, k=4, X0=None, precond=None, project=None, tol=1e-8, maxiter=100, seed=0):
    """The ``k`` lowest eigenpairs of ``A x = λ B x`` by LOBPCG: ``(lam, X, info)``.

    ``A``, ``B``: symmetric positive definite operators of one undistributed space (any
    :class:`~poms_amd.stencil.KronOperator`: Kronecker, stored stencil, matrix-free);
    ``B=None`` is the identity, and nothing is stored twice for ``B X``.  ``precond``:
    ``pcg``'s ``psolve``, ``(A, r) -> StencilVector`` (``solvers.jacobi``,
    ``vc.preconditioner()``); None: ``W = R``.  ``project``: a callable applied in place to
    every start vector and every preconditioned residual (``DirichletBC.project`` keeps the
    iteration in the constrained subspace).  ``X0``: ``k`` start vectors (not modified);
    default ``np.random.default_rng(seed).standard_normal`` over the interior in C order,
    one draw per vector in turn.

    The first step is Rayleigh-Ritz on ``X0``.  Then per iteration: ``R = A X - B X diag(θ)``
    and the relative residuals ``‖r_j‖ / (‖A x_j‖ + |θ_j| ‖B x_j‖)`` from Gram diagonals (stop
    when all are ``<= tol``); ``W = precond(R)``, projected; ``A W`` and ``B W``; the Gram
    matrices ``SᵀAS`` and ``SᵀBS`` of ``S = [X W P]`` (two :func:`block_gram` calls, one copy to
    the host, one synchronisation); :func:`rayleigh_ritz`; new ``X, P, A X, A P, B X, B P``
    as combinations of ``S``, ``A S``, ``B S`` (three :func:`block_combine` calls into a
    second set of buffers, then a swap).  When ``SᵀBS`` is ill-conditioned (see
    :data:`RESTART_COND`) or not positive definite the iteration runs without ``P``
    (``S = [X W]``) and counts a restart.  All ``k`` vectors stay active: there is no locking.

    ``lam``: NumPy array, ascending.  ``X``: ``k`` B-orthonormal vectors.  ``info``:
    ``niter`` (iterations that updated ``X``), ``converged`` (bool per vector), ``res`` (the
    relative residuals of the returned pairs), ``history`` (θ per iteration, ``history[0]``
    from ``X0``), ``restarts``, ``cond`` (of the last Rayleigh-Ritz's scaled ``H``).

    Working set: about ``15 k`` vectors (two sets of ``X, P, AX, AP, BX, BP`` and ``W, AW,
    BW``; ``10 k`` with ``B=None``), beside what ``precond`` allocates.  Raises ``ValueError``
    for ``k < 1``, ``3 k > 24`` or operators of different spaces and ``NotImplementedError``
    for a distributed (slab / Cart) space, before anything is allocated."""
    k = _check_k(k)
    V = getattr(A, "space", None)
    if V is None or not hasattr(A, "dot"):
        raise TypeError("lobpcg: A must be a poms_amd operator (KronOperator, StencilMatrix, MatrixFreeOperator)")
    if B is not None and getattr(B, "space", None) is not V:
        raise ValueError("lobpcg: A and B must act on the same StencilVectorSpace")
    if V.dist is not None:
        raise NotImplementedError("lobpcg: distributed (slab / Cart) spaces are not supported")
    if X0 is not None:
        X0, V0 = _space_of(X0, "lobpcg: X0")
        if len(X0) != k or V0 is not V:
            raise ValueError(f"lobpcg: X0 must be {k} vectors of the operators' space")
    import torch

    def apply(Op, xs, outs):
        for x, y in zip(xs, outs):
            x.update_ghost_regions()
            Op.dot(x, out=y)

    fresh = lambda: [V.empty() for _ in range(k)]
    # the start block, its images, and the first Rayleigh-Ritz
    X = fresh()
    if X0 is None:
        rng = np.random.default_rng(seed)
        for x in X:
            x.from_numpy(rng.standard_normal(int(np.prod(V.npts))).reshape(V.npts))
    else:
        for x, x0 in zip(X, X0):
            x.assign(x0)
    if project is not None:
        for x in X:
            project(x)
    AX, P, AP = fresh(), fresh(), fresh()
    Xn, AXn, Pn, APn = fresh(), fresh(), fresh(), fresh()
    W, AW = fresh(), fresh()
    if B is not None:
        BX, BP, BXn, BPn, BW = fresh(), fresh(), fresh(), fresh(), fresh()
    else:
        BX, BP, BXn, BPn, BW = X, P, Xn, Pn, W
    apply(A, X, AX)
    if B is not None:
        apply(B, X, BX)
    dev = X[0]._data.device
    small = torch.empty((2, 3 * k, 3 * k), dtype=torch.float64, device=dev)

    def grams(S, AS, BS):
        n = len(S)
        g = small.view(-1)[:2 * n * n].view(2, n, n)
        block_gram(S, AS, symmetric=True, out=g[0])
        block_gram(S, BS, symmetric=True, out=g[1])
        h = g.cpu().numpy()   # one copy, one synchronisation
        return h[0], h[1]

    def combine3(S, AS, BS, C, outs, aouts, bouts):
        Cd = torch.from_numpy(np.ascontiguousarray(C)).to(dev)
        block_combine(S, Cd, outs)
        block_combine(AS, Cd, aouts)
        if B is not None:
            block_combine(BS, Cd, bouts)

    G, H = grams(X, AX, BX)
    theta, C, cond, _ = ritz_step(G, H, k, False)
    combine3(X, AX, BX, C, Xn, AXn, BXn)
    X, Xn, AX, AXn = Xn, X, AXn, AX
    if B is not None:
        BX, BXn = BXn, BX
    else:
        BX, BXn = X, Xn
    history = [theta.copy()]
    restarts, niter, have_p = 0, 0, False
    eye = np.eye(k)
    nrm = torch.empty((3 * k, 3 * k), dtype=torch.float64, device=dev)
    while True:
        # R = A X - B X diag(theta), into W's buffers; the residual norms from the diagonal of
        # one Gram call on [R AX BX]
        block_combine(AX + BX, np.vstack([eye, -np.diag(theta)]), W)
        T = W + AX + BX
        d = np.diag(block_gram(T, T, symmetric=True, out=nrm).cpu().numpy())
        res = residual_norms(theta, d[k:2 * k], d[2 * k:], d[:k])
        if np.all(res <= tol) or niter >= maxiter:
            break
        if precond is not None:
            for w in W:
                s = precond(A, w)
                if s is w:
                    raise RuntimeError("lobpcg: precond returned its input buffer")
                w.assign(s)
        if project is not None:
            for w in W:
                project(w)
        apply(A, W, AW)
        if B is not None:
            apply(B, W, BW)
        S, AS, BS = X + W, AX + AW, BX + BW
        if have_p:
            S, AS, BS = S + P, AS + AP, BS + BP
        G, H = grams(S, AS, BS)
        theta, C, cond, restarted = ritz_step(G, H, k, have_p)
        restarts += int(restarted)
        Cp = C.copy()
        Cp[:k] = 0.0
        combine3(S, AS, BS, np.hstack([C, Cp]), Xn + Pn, AXn + APn, BXn + BPn)
        X, Xn, P, Pn, AX, AXn, AP, APn = Xn, X, Pn, P, AXn, AX, APn, AP
        if B is not None:
            BX, BXn, BP, BPn = BXn, BX, BPn, BP
        else:
            BX, BP, BXn, BPn = X, P, Xn, Pn
        have_p = True
        niter += 1
        history.append(theta.copy())
    info = {"niter": niter, "converged": res <= tol, "res": res, "history": history, "restarts": restarts,
            "cond": cond}
    return theta.copy(), X, info
