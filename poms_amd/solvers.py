"""Krylov solver and smoothers of the V-cycle, with the reference's API.

Signatures, defaults, return conventions and stopping rules are those of
`sources/solvers.py`:

* ``pcg(A, psolve, b, x0=None, tol=1e-6, maxiter=100, verbose=False) -> (x, info)``
  (`sources/solvers.py:69-135`), ``info = {'niter', 'success', 'res_norm'}``;
  the stop test ``r.r < tol * ||r0||`` mixes squared and unsquared norms
  exactly as the reference does (:87, :113).
* ``damped_jacobi(A, b, x0=None, tol=1e-6, maxiter=10, verbose=False) -> x``
  (:167-235), omega = 2/3, stop when ``dr.dr < tol**2`` *after* the update.
* ``jacobi(A, b) -> x`` (:139-163).
* ``crl(A, b, x0=None, tol=1e-5, maxiter=1000, verbose=False) -> (x, info)``
  (:3-65): conjugate residual, stop when ``s.r < tol**2`` before the update.
* ``pcg_glt(A, M1, M2, b, x0=None, tol=1e-6, maxiter=100, verbose=False) -> (x, info)``
  (:239-306): the same PCG with the Kronecker direct solve
  ``kron_solve_par(M2, M1, r)`` as preconditioner (:258, :290), factorised once
  per (M2, M1) pair (``poms_amd.kron_solve``); :func:`pcg_kron` is its n-D form.

Differences that do not change results:
* the reference's discarded ``s = A.dot(r)`` (:109) is not computed;
* with ``_skip_tail`` (the V-cycles' smoother calls) neither are ``psolve``, ``s.r``,
  ``beta`` and ``p`` of iteration ``k == maxiter`` (:117-124), which nothing reads;
* with ``_defer_x`` (the 3D V-cycles' smoother calls) ``x += alpha p`` of several
  iterations runs as one pass over their kept ``p`` (the same fma per term: the same bits);
* the per-element Python loop ``dr = omega*r/A[i,i,0,0]`` (:211-213) and the
  surrounding ``r = b - A.dot(x)``, ``x = x + dr``, ``dr.dot(dr)`` are one
  fused HIP kernel; the first sweep from ``x0 = None`` uses ``A.0 = 0``
  exactly and launches the diagonal scaling alone;
* with ``tol == 0`` the norms that can never stop the iteration are not
  computed (no host synchronisation);
* inside ``pcg`` with this module's ``damped_jacobi`` as ``psolve``, ``s.dot(r)``
  is accumulated by the final smoothing sweep (``poms_op_jacobi_sweep_dot``);
* ``q = A.dot(p)`` and ``p.dot(q)`` come from one pass (``poms_op_apply_dot``);
* from ``x0 = None`` sweeps 1 and 2 run as one pass over ``b``
  (``poms_op_jacobi_from_zero``); if the reference would stop after sweep 1,
  ``x1`` is formed separately and returned.

Inputs must be :mod:`poms_amd.stencil` device objects; there is no CPU path.
"""
from __future__ import annotations

import os
from math import sqrt

from .stencil import KronOperator, StencilVector

OMEGA = 2.0 / 3.0


def _check(A, b):
    if not isinstance(A, KronOperator) or not isinstance(b, StencilVector):
        raise TypeError("poms_amd solvers take a poms_amd.stencil.KronOperator and StencilVector "
                        "(device-resident); there is no CPU fallback")
    n = A.shape[0]
    assert A.shape == (n, n)
    assert b.shape == (n,)


def _print_header(title):
    print(title)
    print("+---------+---------------------+")
    print("+ Iter. # | L2-norm of residual |")
    print("+---------+---------------------+")


def _tail_skipped(skip_tail) -> bool:
    """``_skip_tail`` unless POMS_PCG_TAIL=1 asks for the reference's full last iteration
    (read per call: an A/B of both in one process)."""
    return bool(skip_tail) and os.environ.get("POMS_PCG_TAIL", "0") != "1"


def pcg(A, psolve, b, x0=None, tol=1e-6, maxiter=100, verbose=False, *, _x0_owned=False, _skip_tail=False,
        _defer_x=0, _fold_r=False):
    """Preconditioned conjugate gradient (`sources/solvers.py:69-135`).

    ``_skip_tail`` (internal: the V-cycles' smoother calls): iteration ``k == maxiter``
    ends after ``x += alpha p`` and ``r.r``.  The reference goes on to ``s = psolve(A, r)``,
    ``s.r``, ``beta`` and ``p = s + beta p`` (`sources/solvers.py:117-124`), leaves the
    loop and returns ``x`` and ``info`` without reading any of them: the same result,
    one preconditioner call less.

    ``_x0_owned`` (internal: the V-cycle's own temporaries) lets the native loop
    iterate in x0's buffer instead of a copy of it -- the reference copies x0
    (`sources/solvers.py:82`); a caller that never reads x0 again loses nothing.

    ``_defer_x`` (internal: the 3D V-cycles' smoother calls, see :func:`defer_x_count`):
    the number of extra ``p`` buffers the native loop may keep, so that ``x += alpha p``
    runs as one pass per that many iterations instead of one per iteration -- the same
    fma per term, the same ``x`` and ``info``; one more vector of memory per buffer.
    ``POMS_PCG_DEFER_X=<n>`` (read per call) replaces a non-zero count, 0 turns it off.

    ``_fold_r`` (internal: the V-cycles' smoother calls; with ``_skip_tail`` and ``_defer_x`` on
    the native loop only): where ``A.rjacobi0_supported``, ``r -= alpha q`` is formed inside the
    preconditioner call's first launch instead of a pass of its own, and the stop test is
    decided from that launch's ``r . r`` unless it falls within a guard band of rounding
    errors around the threshold, where the r update's own sum is formed and decides -- the
    same ``x`` and ``info``; one more vector of memory.  ``POMS_PCG_RFOLD=0`` (read per call)
    keeps the two launches."""
    _check(A, b)
    V = b.space
    skip_tail = _tail_skipped(_skip_tail)
    if (psolve is damped_jacobi and not verbose and V.lazy_reductions and A.apply_dot_supported
            and A.fused_dot_supported):
        if _native_ok(A, V):
            return _pcg_native(A, b, x0, tol, maxiter, _x0_owned, skip_tail, _defer_x, bool(_fold_r))
        return _pcg_device(A, b, x0, tol, maxiter, skip_tail)
    ctx, lay = V.ctx, V.layout
    if x0 is None:
        x = V.zeros()
        r = V.empty().assign(b)          # r = b - A.0 = b exactly
    else:
        assert x0.shape == (A.shape[0],)
        x = x0.copy()
        r = A.residual(b, x)

    nrmr0 = sqrt(r.dot(r))
    s, sr = _psolve_dot(A, psolve, r)
    p = s
    q = V.empty()

    if verbose:
        _print_header("CG solver:")
        template = "| {:7d} | {:19.2e} |"

    k = 0
    nrmr = nrmr0 * nrmr0
    fused_pq = A.apply_dot_supported
    for k in range(1, maxiter + 1):
        if fused_pq:
            pq = A.dot_inner(p, q)       # q = A p and p.q in one pass
        else:
            A.dot(p, out=q)
            pq = p.dot(q)
        alpha = sr / pq
        if skip_tail and k == maxiter:              # what follows would be discarded
            import torch
            a_dev = torch.tensor([alpha], dtype=x._data.dtype, device=x._data.device)
            nrmr = V.global_dot(float(_pcg_final_update_dev(V, a_dev, x, p, r, q, local=True).item()))
            if nrmr < tol * nrmr0:
                x.assign(r)                         # (x as the early-stop update below rounds it)
                k -= 1
            elif verbose:
                print(template.format(k, sqrt(nrmr)))
            break
        nrmr = _pcg_r_update(V, alpha, r, q)        # r -= alpha q ; r.r
        if nrmr < tol * nrmr0:
            _vec(V, "poms_vec_axpby", 1.0, x, alpha, p, x)   # x += alpha p
            k -= 1
            break
        srold = sr
        s, sr = _psolve_dot(A, psolve, r)
        beta = sr / srold
        if p is s:
            raise RuntimeError("psolve returned its input buffer")
        _pcg_xp_update(V, alpha, beta, x, p, s)     # x += alpha p ; p = s + beta p  (old p, one pass)
        if verbose:
            print(template.format(k, sqrt(nrmr)))

    if verbose:
        print("+---------+---------------------+")
    info = {"niter": k, "success": nrmr < tol * nrmr0, "res_norm": sqrt(nrmr)}
    return x, info


def _pcg_device(A, b, x0, tol, maxiter, skip_tail=False):
    """pcg with damped_jacobi as psolve, scalars on the device.

    Same iterates and stopping rule as the host loop above (`sources/solvers.py:69-135`).
    alpha = s.r / p.q and beta = s.r / s.r_old are device tensors read by the
    update kernels (``poms_*_dev``); the host reads only r.r for the stop test,
    and only after the next preconditioner call is queued, so the device never
    idles waiting for the host.  If the test fires, that queued psolve(r) is
    discarded (the reference stops before computing it: results are identical).
    """
    import torch
    V = b.space
    if x0 is None:
        x = V.zeros()
        r = V.empty().assign(b)
    else:
        assert x0.shape == (A.shape[0],)
        x = x0.copy()
        r = A.residual(b, x)
    nrmr0 = sqrt(r.dot(r))
    s, sr = _damped_jacobi(A, r, want_dot=True, device_dot=True)
    if sr is None:
        sr = s.dot_device(r)
    p = s
    q = V.empty()
    k = 0
    nrmr = nrmr0 * nrmr0
    for k in range(1, maxiter + 1):
        pq = A.dot_inner(p, q, device=True)
        alpha = sr / pq
        if skip_tail and k == maxiter:                  # what follows would be discarded
            nrmr = V.lazy_value(_pcg_final_update_dev(V, alpha, x, p, r, q)).value()
            if nrmr < tol * nrmr0:
                x.assign(r)                             # (x as the early-stop update below rounds it)
                k -= 1
            break
        nrm_dev = _pcg_r_update_dev(V, alpha, r, q)     # r -= alpha q ; r.r (device)
        pending = V.lazy_value(nrm_dev)
        srold = sr
        s_next, sr = _damped_jacobi(A, r, want_dot=True, device_dot=True)   # queued before the read
        if sr is None:
            sr = s_next.dot_device(r)
        nrmr = pending.value()
        if nrmr < tol * nrmr0:
            _vec_dev(V, "poms_vec_axpby_dev", torch.cat([torch.ones_like(alpha), alpha]), x, p, x)
            k -= 1
            break
        beta = sr / srold
        _pcg_xp_update_dev(V, torch.cat([alpha, beta]), x, p, s_next)
    info = {"niter": k, "success": nrmr < tol * nrmr0, "res_norm": sqrt(nrmr)}
    return x, info


def _native_ok(A, V) -> bool:
    """The whole pcg + damped-Jacobi loop runs in C (poms_pcg_jacobi) unless disabled
    (POMS_NATIVE_PCG=0), the space is a Cart block (its ghost exchange is the torch
    transport's) or a distributed space has no native communicator."""
    import os
    if os.environ.get("POMS_NATIVE_PCG", "1") == "0" or V.is_cart:
        return False
    return not V.is_distributed or V.dist.native is not None


def defer_x_count(A, V, maxiter) -> int:
    """The ``_defer_x`` a V-cycle passes to its smoother calls: ``min(maxiter, 10)`` p
    buffers on a 3D single-rank space whose pcg runs natively, else 0.  (In 2D the vectors
    live in the cache, the loop is latency-bound and beta is folded: nothing to gain.)"""
    if V.ndim != 3 or V.is_distributed or not _native_ok(A, V):
        return 0
    return max(0, min(int(maxiter), 10))


def _defer_buffers(A, V, n):
    """``n`` p buffers for the deferred x updates, allocated lazily, once, beside
    ``A._pcg_work`` (every smoother call on A shares them); [] when ``n`` < 2, when
    ``POMS_PCG_DEFER_X`` says 0, or when the allocation fails (said once)."""
    e = os.environ.get("POMS_PCG_DEFER_X", "")
    if n and e != "":
        n = int(e)
    if n < 2 or getattr(A, "_pcg_defer_failed", False):
        return []
    n = min(n, 15)
    bufs = getattr(A, "_pcg_pbufs", None)
    if bufs is None or (bufs and bufs[0].space is not V):
        bufs = A._pcg_pbufs = []
    try:
        while len(bufs) < n:
            bufs.append(V.empty())
    except RuntimeError as exc:   # (torch.cuda.OutOfMemoryError is one)
        import warnings
        A._pcg_pbufs = []
        A._pcg_defer_failed = True
        warnings.warn(f"pcg: no memory for {n} deferred-x buffers ({exc.__class__.__name__}); "
                      "x is updated every iteration instead", RuntimeWarning)
        return []
    return bufs[:n]


def _pcg_native(A, b, x0, tol, maxiter, x0_owned=False, skip_tail=False, defer_x=0, fold_r=False):
    """pcg(A, damped_jacobi, b, x0, tol, maxiter) as one C call (``poms_pcg_jacobi``):
    the launches, device scalars and stop tests of :func:`_pcg_device`, bitwise the
    same iterates, without a Python round trip per launch."""
    import ctypes as C
    from . import _lib, runtime as rt
    V = b.space
    work = getattr(A, "_pcg_work", None)
    if work is None or work[0].space is not V:
        work = A._pcg_work = [V.empty() for _ in range(5)]
    # (x0 = None: the C loop zero-fills x's interior; empty() zeroes only the ghosts,
    # instead of a second full-storage fill)
    x = (V.empty() if os.environ.get("POMS_PCG_X_EMPTY", "1") != "0" else V.zeros()) if x0 is None else (x0 if x0_owned else x0.copy())
    if x0 is not None:
        assert x0.shape == (A.shape[0],)
    d = V.dist if V.is_distributed else None
    opts = _lib.PcgOpts(float(tol), int(maxiter), 1e-6, 10, OMEGA,
                        -1 if d is None or d.prev is None else int(d.prev),
                        -1 if d is None or d.next is None else int(d.next), 1 if skip_tail else 0)
    pbufs = _defer_buffers(A, V, int(defer_x)) if d is None else []
    if pbufs:
        pptrs = (C.c_void_p * len(pbufs))(*[w._data.data_ptr() for w in pbufs])
        opts.n_pbuf, opts.pbuf = len(pbufs), pptrs
    opts.fold_r = 1 if fold_r else 0
    info = _lib.PcgInfo()
    ptrs = (C.c_void_p * 5)(*[w._data.data_ptr() for w in work])
    _lib.call("poms_pcg_jacobi", A._h, d.native.h if d is not None else None,
              C.byref(opts), rt.ptr(b._data), rt.ptr(x._data), 0 if x0 is None else 1, ptrs, C.byref(info),
              rt.stream_handle())
    x._mark_written()
    for w in work + pbufs:
        w._mark_written()
    A._calls += 1
    return x, {"niter": info.niter, "success": bool(info.success), "res_norm": info.res_norm}


def _vec_dev(V, name, ab, xv, yv, zv):
    from . import _lib, runtime as rt
    import ctypes as C
    _lib.call(name, V.ctx, C.byref(V.layout), rt.ptr(ab), rt.ptr(xv._data), rt.ptr(yv._data), rt.ptr(zv._data),
              rt.stream_handle())
    zv._mark_written()


def _pcg_r_update_dev(V, alpha, r, q):
    from . import _lib, runtime as rt
    import ctypes as C
    buf = V.scalar_buffer()
    _lib.call("poms_pcg_r_update_dev", V.ctx, C.byref(V.layout), rt.ptr(alpha), rt.ptr(r._data), rt.ptr(q._data),
              rt.ptr(buf), rt.stream_handle())
    r._mark_written()
    return V.device_sum(buf[0:1])


def _pcg_final_update_dev(V, alpha, x, p, r, q, local=False):
    """x += alpha p and (r - alpha q).(r - alpha q) (device; ``local``: this rank's part).
    r - alpha q is not kept: r takes x as pcg's early-stop update would have rounded it
    (``poms_pcg_final_update_dev``), for the caller whose stop test fires on the sum."""
    from . import _lib, runtime as rt
    import ctypes as C
    buf = V.scalar_buffer()
    _lib.call("poms_pcg_final_update_dev", V.ctx, C.byref(V.layout), rt.ptr(alpha), rt.ptr(x._data), rt.ptr(p._data),
              rt.ptr(r._data), rt.ptr(q._data), rt.ptr(buf), rt.stream_handle())
    x._mark_written()
    r._mark_written()
    return buf[0:1] if local else V.device_sum(buf[0:1])


def _pcg_xp_update_dev(V, ab, x, p, s):
    from . import _lib, runtime as rt
    import ctypes as C
    _lib.call("poms_pcg_xp_update_dev", V.ctx, C.byref(V.layout), rt.ptr(ab), rt.ptr(x._data), rt.ptr(p._data),
              rt.ptr(s._data), rt.stream_handle())
    x._mark_written()
    p._mark_written()


def _psolve_dot(A, psolve, r):
    """``s = psolve(A, r)`` and ``s.dot(r)``; for this module's damped_jacobi the dot is
    accumulated by the last smoothing sweep itself (same values, one pass less)."""
    if psolve is damped_jacobi and A.fused_dot_supported:
        s, sr = _damped_jacobi(A, r, want_dot=True)
        if sr is not None:
            return s, sr
        return s, s.dot(r)
    s = psolve(A, r)
    return s, s.dot(r)


def _vec(V, name, a, xv, b, yv, zv):
    from . import _lib, runtime as rt
    import ctypes as C
    _lib.call(name, V.ctx, C.byref(V.layout), float(a), rt.ptr(xv._data), float(b), rt.ptr(yv._data),
              rt.ptr(zv._data), rt.stream_handle())
    zv._mark_written()


def _pcg_r_update(V, alpha, r, q) -> float:
    from . import _lib, runtime as rt
    import ctypes as C
    buf = V.scalar_buffer()
    _lib.call("poms_pcg_r_update", V.ctx, C.byref(V.layout), float(alpha), rt.ptr(r._data), rt.ptr(q._data),
              rt.ptr(buf), rt.stream_handle())
    r._mark_written()
    return V.global_dot(float(buf[0].item()))


def _pcg_xp_update(V, alpha, beta, x, p, s):
    from . import _lib, runtime as rt
    import ctypes as C
    _lib.call("poms_pcg_xp_update", V.ctx, C.byref(V.layout), float(alpha), float(beta), rt.ptr(x._data),
              rt.ptr(p._data), rt.ptr(s._data), rt.stream_handle())
    x._mark_written()
    p._mark_written()


def _pcg_update(V, alpha, x, p, r, q) -> float:
    from . import _lib, runtime as rt
    import ctypes as C
    buf = V.scalar_buffer()
    _lib.call("poms_pcg_update", V.ctx, C.byref(V.layout), float(alpha), rt.ptr(x._data), rt.ptr(p._data),
              rt.ptr(r._data), rt.ptr(q._data), rt.ptr(buf), rt.stream_handle())
    x._mark_written()
    r._mark_written()
    return V.global_dot(float(buf[0].item()))


def jacobi(A, b):
    """Point Jacobi ``x = b / diag(A)`` (`sources/solvers.py:139-163`)."""
    _check(A, b)
    x = b.space.empty()
    A.diag_scale(b, x, 1.0, want_norm=False)
    x.update_ghost_regions()
    return x


def damped_jacobi(A, b, x0=None, tol=1e-6, maxiter=10, verbose=False):
    """Weighted Jacobi, omega = 2/3 (`sources/solvers.py:167-235`); returns x."""
    return _damped_jacobi(A, b, x0, tol, maxiter, verbose)[0]


def _damped_jacobi(A, b, x0=None, tol=1e-6, maxiter=10, verbose=False, want_dot=False, device_dot=False):
    """damped_jacobi; with ``want_dot`` also returns ``x.b`` accumulated by the final
    sweep (None when the last sweep was not a full sweep); ``device_dot`` returns it
    as a device tensor and skips the last sweep's norm (it cannot change the result)."""
    _check(A, b)
    V = b.space
    omega = OMEGA
    tol_sqr = tol ** 2
    need = tol_sqr > 0.0 or verbose
    if verbose:
        _print_header("Damped Jacobi method:")
        template = "| {:7d} | {:19.2e} |"

    # Norms are read one sweep late: sweep k is queued before the host waits for
    # ||dr_{k-1}||^2 (copied to pinned memory), so the GPU never idles on the stop
    # test.  If sweep k-1 met it, x_{k-1} is returned -- sweep k wrote the other
    # buffer -- exactly the reference's result (`sources/solvers.py:219-222`).
    lazy = need and not verbose and V.lazy_reductions
    pending = None                      # (LazyScalar of sweep k-1, buffer holding x_{k-1})

    def settle(pend):
        if len(pend) == 3:          # sweeps 1 and 2 from zero: (norms, x2 buffer, b)
            lz, xbuf, rhs = pend
            if lz.value(0) < tol_sqr:
                x1 = V.empty()
                A.diag_scale(rhs, x1, omega)
                return True, x1
            return lz.value(1) < tol_sqr, xbuf
        lz, xbuf = pend
        return lz.value() < tol_sqr, xbuf

    k0 = 1
    if x0 is None and maxiter >= 2 and not verbose and not (want_dot and maxiter == 2) \
            and A.from_zero_supported:
        # k = 1, 2 from x = 0 in one pass over b (x1 = omega b / diag is formed on the fly)
        x = V.empty()
        res = A.jacobi_from_zero(b, x, omega, want_norm=need, lazy=lazy)
        if lazy:
            pending = (res, x, b)
        elif need:
            n1, n2 = res
            if n1 < tol_sqr:        # the reference stops after sweep 1: return x1 itself
                x1 = V.empty()
                A.diag_scale(b, x1, omega)
                return x1, None
            if n2 < tol_sqr:
                return x, None
        k0 = 3
    elif x0 is None:
        if maxiter < 1:
            return V.zeros(), None
        # k = 1 from x = 0:  r = b - A.0 = b,  dr = omega b / diag,  x = dr
        x = V.empty()
        nrmr = A.diag_scale(b, x, omega, want_norm=need, lazy=lazy)
        if lazy:
            pending = (nrmr, x)
        else:
            if need and nrmr < tol_sqr:
                if verbose:
                    print("+---------+---------------------+")
                return x, None
            if verbose:
                print(template.format(1, sqrt(nrmr)))
        k0 = 2
    else:
        assert x0.shape == (A.shape[0],)
        x = x0.copy()

    dot = None
    if maxiter >= k0:
        xn = V.empty()
        for k in range(k0, maxiter + 1):
            if want_dot and k == maxiter and device_dot and lazy:
                # the last sweep's stop test cannot change the result: no norm, dot on device
                nrmr, dot = A.jacobi_sweep(b, x, xn, omega, want_norm=False, want_dot=True, device_dot=True)
            elif want_dot and k == maxiter:   # the last sweep also forms x_out . b
                nrmr, dot = A.jacobi_sweep(b, x, xn, omega, want_norm=need, want_dot=True)
            else:
                nrmr = A.jacobi_sweep(b, x, xn, omega, want_norm=need, lazy=lazy)
            if pending is not None:         # stop test of the previous sweep
                done, xprev = settle(pending)
                pending = None
                if done:
                    return xprev, None
            x, xn = xn, x
            if want_dot and k == maxiter and device_dot and lazy:
                break
            if lazy and not (want_dot and k == maxiter):
                pending = (nrmr, x)
                continue
            if need and nrmr < tol_sqr:
                break
            if verbose:
                print(template.format(k, sqrt(nrmr)))
    if pending is not None and len(pending) == 3:
        # maxiter == 2 from zero: the loop never ran, so sweep 1's stop test is still
        # open -- if it fired, the reference returns x1 (`sources/solvers.py:219-222`)
        done, xprev = settle(pending)
        return xprev, None
    if pending is not None and not device_dot:   # the last sweep's test cannot change the result
        pending[0].value()
    if verbose:
        print("+---------+---------------------+")
    return x, dot


def pcg_kron(A, factors, b, x0=None, tol=1e-6, maxiter=100, verbose=False, *, _skip_tail=False):
    """PCG preconditioned by ``X = (F0^-1 ⊗ F1^-1 [⊗ F2^-1]) R`` (``factors[d]`` acts on
    axis ``d``): the body of `sources/solvers.py:239-306` for any dimension."""
    from .kron_solve import solver_for
    ks = solver_for(b.space, tuple(factors))
    return pcg(A, lambda _A, r: ks.solve(r), b, x0=x0, tol=tol, maxiter=maxiter, verbose=verbose,
               _skip_tail=_skip_tail)


def pcg_glt(A, M1, M2, b, x0=None, tol=1e-6, maxiter=100, verbose=False, *, _skip_tail=False):
    """GLT-preconditioned CG (`sources/solvers.py:239-306`).  As the reference, the
    preconditioner is ``kron_solve_par(M2, M1, r)`` (:258, :290): M2 acts on axis 0."""
    if b.space.ndim != 2:
        raise ValueError("pcg_glt is the 2D solver of the reference; use pcg_kron for other dimensions")
    return pcg_kron(A, (M2, M1), b, x0=x0, tol=tol, maxiter=maxiter, verbose=verbose, _skip_tail=_skip_tail)


def crl(A, b, x0=None, tol=1e-5, maxiter=1000, verbose=False):
    """Conjugate residual method (`sources/solvers.py:3-65`): device vectors, the
    operator's fused residual / apply kernels, in-place vector updates."""
    _check(A, b)
    V = b.space
    if x0 is None:
        x = V.zeros()
        r = V.empty().assign(b)          # b - A.0 = b exactly
    else:
        assert x0.shape == (A.shape[0],)
        x = x0.copy()
        r = A.residual(b, x)
    p = r.copy()
    q = A.dot(p)
    s = q.copy()
    sr = s.dot(r)
    tol_sqr = tol ** 2
    if verbose:
        _print_header("CG solver:")
        template = "| {:7d} | {:19.2e} |"
    k = 0
    for k in range(1, maxiter + 1):
        if sr < tol_sqr:
            k -= 1
            break
        alpha = sr / q.dot(q)
        x.axpby_(alpha, p, 1.0)          # x = x + alpha p
        r.axpby_(-alpha, q, 1.0)         # r = r - alpha q
        A.dot(r, out=s)
        srold = sr
        sr = s.dot(r)
        beta = sr / srold
        p.axpby_(1.0, r, beta)           # p = r + beta p
        q.axpby_(1.0, s, beta)           # q = s + beta q
        if verbose:
            print(template.format(k, sqrt(sr)))
    if verbose:
        print("+---------+---------------------+")
    info = {"niter": k, "success": sr < tol_sqr, "res_norm": sqrt(sr)}
    return x, info


# ---- Chebyshev-Jacobi: a polynomial smoother without inner products ------------------
# Replaces the smoothing calls `pcg(Af, damped_jacobi, bf, ...)` of the reference's cycle
# (`sources/mg_jac.py:88,104`) where D^-1 A has eigenvalues beyond 2/omega = 3 (B-splines
# at p = 3 in 2D, from p = 2 in 3D) and plain damped Jacobi is no contraction.

def chebyshev_coefficients(lmin, lmax, degree):
    """``(alpha, beta)``, two lists of ``degree`` floats, of the three-term recurrence

        x_{k+1} = x_k + beta_k (x_k - x_{k-1}) + alpha_k D^-1 (b - A x_k),  k = 0 .. degree-1

    whose error polynomial is the Chebyshev polynomial of [lmin, lmax] scaled to 1 at 0:
    on a scalar operator lam with b = 0, x_0 = 1 it gives
    ``x_k = T_k((theta - lam)/delta) / T_k(sigma)``.  theta = (lmax + lmin)/2,
    delta = (lmax - lmin)/2, sigma = theta/delta; alpha_0 = 1/theta, beta_0 = 0,
    rho_0 = 1/sigma; rho_k = 1/(2 sigma - rho_{k-1}), alpha_k = 2 rho_k/delta,
    beta_k = rho_k rho_{k-1}."""
    lmin, lmax = float(lmin), float(lmax)
    if not (0.0 < lmin < lmax):
        raise ValueError(f"chebyshev_coefficients: need 0 < lmin < lmax, got [{lmin}, {lmax}]")
    if int(degree) != degree or degree < 1:
        raise ValueError(f"chebyshev_coefficients: degree must be an integer >= 1, got {degree}")
    theta, delta = (lmax + lmin) / 2.0, (lmax - lmin) / 2.0
    sigma = theta / delta
    alpha, beta, rho = [1.0 / theta], [0.0], 1.0 / sigma
    for _ in range(1, int(degree)):
        rho_new = 1.0 / (2.0 * sigma - rho)
        alpha.append(2.0 * rho_new / delta)
        beta.append(rho_new * rho)
        rho = rho_new
    return alpha, beta


def estimate_lmax(A, iters=10, seed=0):
    """The largest Ritz value of ``iters`` Lanczos steps for ``A v = lambda D v``,
    D = diag(A): an estimate of lambda_max(D^-1 A) from below (never above it in exact
    arithmetic; within 1.5 % after 10 steps on the B-spline operators of DESIGN §3.17).

    The start vector is ``np.random.default_rng(seed).standard_normal(n)`` over the
    interior in C order.  The steps run ``A.dot``, ``diag_scale``, ``dot`` and ``axpby_``
    on the device; the coefficients are read on the host every step (a set-up path) and
    the small tridiagonal matrix is solved there."""
    import numpy as np
    import torch
    if not isinstance(A, KronOperator):
        raise TypeError("estimate_lmax takes a poms_amd.stencil.KronOperator")
    if iters < 1:
        raise ValueError("estimate_lmax: iters must be >= 1")
    V = A.space
    z = np.random.default_rng(seed).standard_normal(int(np.prod(V.npts))).reshape(V.npts)
    v = V.zeros().from_numpy(z)
    # u = D v: the diagonal from one diag_scale of ones (1/diag), the only elementwise
    # product of the estimate
    u, w = V.zeros(), V.empty()
    V.interior(u._data).fill_(1.0)
    A.diag_scale(u, w, 1.0)
    V.interior(u._data).copy_(V.interior(v._data) / V.interior(w._data))
    u._mark_written()
    nrm = sqrt(u.dot(v))
    u *= 1.0 / nrm
    v *= 1.0 / nrm
    up, r = V.zeros(), V.empty()
    al, be, b = [], [], 0.0
    for j in range(int(iters)):
        v.update_ghost_regions()
        A.dot(v, out=r)
        a = r.dot(v)
        al.append(a)
        if j + 1 == iters:
            break
        r.axpby_(-a, u, 1.0)             # r = A v - a u - b u_prev  (D-orthogonal to v, v_prev)
        if b != 0.0:
            r.axpby_(-b, up, 1.0)
        A.diag_scale(r, w, 1.0)          # w = D^-1 r
        b2 = r.dot(w)                    # ||w||_D^2
        if not b2 > (1e-14 * abs(a)) ** 2:
            break                        # an invariant subspace: the Ritz values are exact
        b = sqrt(b2)
        be.append(b)
        up, u, r = u, r, up              # u_prev <- u, u <- r / b (r's old buffer is reused)
        u *= 1.0 / b
        v.axpby_(1.0 / b, w, 0.0)        # v <- w / b
    T = np.diag(al) + np.diag(be[:len(al) - 1], 1) + np.diag(be[:len(al) - 1], -1)
    return float(np.linalg.eigvalsh(T)[-1])


def _cached_lmax(A):
    """``estimate_lmax(A)`` with its defaults, kept on the operator until it changes."""
    if getattr(A, "_lmax_est", None) is None:
        A._lmax_est = estimate_lmax(A)
    return A._lmax_est


def chebyshev_work(A):
    """The buffers one :func:`chebyshev` call on ``A`` ping-pongs: two where the step is
    one launch, three where it is composed (``A.cheby_supported``)."""
    return [A.space.empty() for _ in range(2 if A.cheby_supported else 3)]


def chebyshev(A, b, x0=None, degree=10, lmax=None, ratio=30.0, safety=1.1, work=None, *, _x0_owned=False):
    """``degree`` steps of the Chebyshev iteration on D^-1 A over the interval
    ``[safety lmax / ratio, safety lmax]``; returns ``(x, info)``,
    ``info = {"niter": degree, "lmin":, "lmax":}`` (the interval).  There is no residual
    norm and no stop test: the call is a fixed chain of launches -- a fixed polynomial in
    D^-1 A applied to ``b - A x0``, so a cycle smoothed with it is a fixed linear operator.

    ``lmax=None``: :func:`estimate_lmax`, cached on the operator (dropped when its
    Dirichlet faces or coefficients change).  ratio 30 and safety 1.1 are the customary
    defaults of other libraries.  From ``x0=None`` the first step is
    ``diag_scale(b, x, alpha_0)``.  ``work`` (:func:`chebyshev_work`: vectors of
    ``V.empty()``, whose ghosts are zero) supplies the buffers, and the call then allocates
    nothing; the returned ``x`` is one of them (or ``x0``'s buffer with ``_x0_owned``, the
    V-cycle's own temporaries)."""
    _check(A, b)
    V = b.space
    if lmax is None:
        lmax = _cached_lmax(A)
    hi = float(safety) * float(lmax)
    lo = hi / float(ratio)
    alpha, beta = chebyshev_coefficients(lo, hi, degree)
    fused = A.cheby_supported
    if work is None:
        work = chebyshev_work(A)
    if x0 is not None:
        assert x0.shape == (A.shape[0],)
    # the buffers free to write: all of work, but for an owned x0 that is one of them (the
    # V-cycle's post-smoothing continues in the buffers its pre-smoothing ended in)
    free = [w for w in work if not (_x0_owned and w is x0)]
    if len(free) < (1 if _x0_owned and x0 is not None else 2) + (0 if fused else 1):
        raise ValueError(f"chebyshev: work needs {2 if fused else 3} vectors")
    if any(w is b or w is x0 for w in free):
        raise ValueError("chebyshev: work must not hold b or x0")
    t = None if fused else free.pop()
    if x0 is None:
        x, y = free[0], free[1]
        A.diag_scale(b, x, alpha[0])     # x_1 = alpha_0 D^-1 b  (A.0 = 0 exactly)
        if degree > 1:
            from . import _lib, runtime as rt
            import ctypes as C
            _lib.call("poms_vec_fill", V.ctx, C.byref(V.layout), 0.0, rt.ptr(y._data), rt.stream_handle())   # x_0
            y._mark_written()
    else:
        xin, y = (x0, free[0]) if _x0_owned else (free[1].assign(x0), free[0])
        xin.update_ghost_regions()
        A.cheby_step(b, xin, y, alpha[0], 0.0, work=t)
        x, y = y, xin
    for k in range(1, int(degree)):
        x.update_ghost_regions()
        A.cheby_step(b, x, y, alpha[k], beta[k], work=t)
        x, y = y, x
    return x, {"niter": int(degree), "lmin": lo, "lmax": hi}
