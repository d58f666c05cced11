"""pcg's p update formed inside the next apply + dot launch (``EPI_PAPPLYDOT``, ``POMS_PCG_PFOLD``).

With deferred x updates the native loop used to write ``p_next = s + beta p`` with the flat
``V_PUPD`` launch and read it straight back in the apply + dot.  Where v5's 16-wave tiles
run (3D, p <= 3, one rank) the loop now only forms beta, and the next apply + dot forms
``p_next`` in its LDS ring with ``V_PUPD``'s fma, stores the interior points and goes on as the
apply + dot of ``p_next``: the same tiles, the same partial slots.

Every comparison is the fused path against ``POMS_PCG_PFOLD=0`` (the two launches) in the same
process, ``torch.equal`` on the whole storage of ``x`` and ``==`` on ``info``: the arithmetic is
the same, so there is no tolerance.  Shapes (DOF extents): the smallest at which each
mechanism of the kernel can fail --

* (12, 19, 118), chunk 6: two chunks of axis 0 (their halo planes must not be stored), two
  row tiles, the second with 3 rows (waves without an output row still combine the rows
  they own), two column tiles (112 + 6 on the aligned layout), on both layouts (16-B and
  8-B stores);
* (9, 17, 20): one tile, one chunk, no row inside the Toeplitz interior;
* (11, 21, 13) at p = 2 (a 20-row x tile: the waves that own two rows are 0..3);
* p = 4 (8-wave tiles): keeps the two launches.
"""
import ctypes as C

import numpy as np
import pytest

from poms_amd.splines import assemble_1d, uniform_knots

pytestmark = pytest.mark.gpu

MAXITER = 7
BUFFERS = (2, 3, 7)   # buffer reuse before and after an x flush; as many buffers as iterations

# name -> (DOF per axis, p, align, chunk)
LAYOUTS = {
    "p3-two-chunks": ((12, 19, 118), 3, False, 6),
    "p3-two-chunks-aligned": ((12, 19, 118), 3, True, 6),
    "p3-one-tile": ((9, 17, 20), 3, False, 0),
    "p2": ((11, 21, 13), 2, False, 0),
}
FIRST = ("p3-two-chunks", "p3-two-chunks-aligned")

# (powers of A applied to a normal b, scale of x0) to look for the stop branches among (as
# test_gpu_pcg_defer.py: r.r of pcg need not fall from one iteration to the next)
CANDIDATES = [(0, 1.0), (1, 1.0), (2, 1.0), (2, 1e-3), (4, 1e-3)]


def _operator(shape, p, align, chunk):
    from poms_amd.stencil import KronOperator, StencilVectorSpace
    mats = [assemble_1d(uniform_knots(p, n - p), p) for n in shape]
    V = StencilVectorSpace(list(shape), [p] * len(shape), align=align)
    A = KronOperator.laplace(V, [m[0] for m in mats], [m[1] for m in mats])
    if chunk:
        A.set_chunk(chunk)
    return V, A


def _problem(shape, p, align, chunk, cand=CANDIDATES[0]):
    V, A = _operator(shape, p, align, chunk)
    rng = np.random.default_rng(1000 * shape[0] + 10 * p)
    power, xscale = cand
    bn = rng.standard_normal(shape)
    for _ in range(power):
        bn = A.dot(V.zeros().from_numpy(bn)).to_local_numpy()
    b = V.zeros().from_numpy(bn)
    xi = V.zeros().from_numpy(xscale * rng.standard_normal(shape))
    return V, A, b, xi


def _run(monkeypatch, A, b, xi, start, tol, maxiter, skip, nbuf, fused):
    """One pcg call with ``nbuf`` p buffers -> (x, info, fused launches)."""
    import torch
    from poms_amd import solvers
    monkeypatch.delenv("POMS_PCG_DEFER_X", raising=False)
    if fused:
        monkeypatch.delenv("POMS_PCG_PFOLD", raising=False)
    else:
        monkeypatch.setenv("POMS_PCG_PFOLD", "0")
    x0 = None if start == "none" else xi.copy() if start == "owned" else xi
    keep = xi._data.clone()
    n0 = A.papply_dot_count
    x, info = solvers.pcg(A, solvers.damped_jacobi, b, x0=x0, tol=tol, maxiter=maxiter, _skip_tail=skip,
                          _x0_owned=start == "owned", _defer_x=nbuf)
    assert torch.equal(xi._data, keep), "the caller's x0 was modified"
    return x, info, A.papply_dot_count - n0


def _same(got, ref, what):
    import torch
    assert torch.equal(got[0]._data, ref[0]._data), what
    assert got[1] == ref[1], (what, got[1], ref[1])
    assert ref[2] == 0, (what, "POMS_PCG_PFOLD=0 ran the fused launch")


def _stop_cases(monkeypatch, layout, start):
    """(problem, [(name, tol, maxiter)], jm, jl): no stop, a stop in the middle, a stop in
    iteration maxiter -- from r.r per iteration on the two-launch path (iteration j stops pcg
    when r.r_j < tol ||r0|| and no earlier one did)."""
    shape, p, align, chunk = LAYOUTS[layout]
    tried = []
    for cand in CANDIDATES:
        V, A, b, xi = _problem(shape, p, align, chunk, cand)
        nrm0 = _run(monkeypatch, A, b, xi, start, 0.0, 0, True, 3, False)[1]["res_norm"]
        rr = [_run(monkeypatch, A, b, xi, start, 0.0, j, True, 3, False)[1]["res_norm"] ** 2
              for j in range(1, MAXITER + 1)]
        firsts = [j for j in range(2, MAXITER + 1) if rr[j - 1] < (1.0 - 1e-6) * min(rr[:j - 1])]
        tried.append((cand, rr, firsts))
        if len(firsts) >= 2 and firsts[-1] >= 4:
            break
    else:
        pytest.fail(f"no candidate right-hand side reaches the stop branches: {tried}")
    tol_at = lambda j: 0.5 * (rr[j - 1] + min(rr[:j - 1])) / nrm0
    jl, jm = firsts[-1], min(firsts[:-1], key=lambda j: abs(j - 4))
    return (V, A, b, xi), [("none", 0.0, MAXITER), ("middle", tol_at(jm), MAXITER), ("last", tol_at(jl), jl)], jm, jl


@pytest.mark.parametrize("start", ["none", "given", "owned"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_folded_p_update_is_bitwise_neutral(gpu, monkeypatch, layout, start):
    """maxiter 7 with 2, 3 and 7 p buffers, with and without skip_tail, no stop, a stop in the
    middle and one in iteration maxiter (the last shows the flush of a remembered update
    and the update that is never needed)."""
    (V, A, b, xi), cases, jm, jl = _stop_cases(monkeypatch, layout, start)
    for name, tol, maxiter in cases:
        for skip in (False, True):
            for nbuf in BUFFERS:
                ref = _run(monkeypatch, A, b, xi, start, tol, maxiter, skip, nbuf, False)
                if name == "none":
                    assert ref[1]["niter"] == maxiter and not ref[1]["success"], ref[1]
                elif name == "middle":
                    assert ref[1]["success"] and ref[1]["niter"] == jm - 1 < maxiter - 1, ref[1]
                else:
                    assert ref[1]["success"] and ref[1]["niter"] == maxiter - 1 == jl - 1, ref[1]
                got = _run(monkeypatch, A, b, xi, start, tol, maxiter, skip, nbuf, True)
                _same(got, ref, (layout, start, name, skip, nbuf))
                # every p update but a last one no apply follows went into an apply + dot
                stop = maxiter if name == "none" else ref[1]["niter"] + 1   # the iteration the loop leaves in
                assert got[2] == stop - 1, (layout, start, name, skip, nbuf, got[2])


@pytest.mark.parametrize("layout", FIRST)
def test_p_buffers_hold_what_the_two_launches_left(gpu, monkeypatch, layout):
    """The loop runs out right after a p update (no skip_tail): the remembered update is
    flushed as the plain launch, and every p buffer, ghosts included, ends as before."""
    import torch
    shape, p, align, chunk = LAYOUTS[layout]
    V, A, b, xi = _problem(shape, p, align, chunk)
    for nbuf in BUFFERS:
        held = []
        for fused in (False, True):
            _run(monkeypatch, A, b, xi, "given", 0.0, 1, False, nbuf, fused)   # (allocates the buffers)
            for w in A._pcg_pbufs:
                V.interior(w._data).fill_(float("nan"))
            _run(monkeypatch, A, b, xi, "given", 0.0, MAXITER, False, nbuf, fused)
            held.append([w._data.clone() for w in A._pcg_pbufs[:nbuf]])
        for i, (a, c) in enumerate(zip(*held)):
            assert torch.equal(a, c), (layout, nbuf, i)
            assert torch.isfinite(a).all()


@pytest.mark.parametrize("layout", FIRST)
def test_scalar_kernel_paths_agree(gpu, monkeypatch, layout):
    """POMS_ALPHA_FOLD 0 and 1 and POMS_HOST_PARTIALS=0 (the paths the large grids take)."""
    shape, p, align, chunk = LAYOUTS[layout]
    V, A, b, xi = _problem(shape, p, align, chunk)
    for start in ("none", "given"):
        for skip in (False, True):
            ref = _run(monkeypatch, A, b, xi, start, 0.0, MAXITER, skip, 3, False)
            for env in ({"POMS_ALPHA_FOLD": "1"}, {"POMS_ALPHA_FOLD": "0"}, {"POMS_HOST_PARTIALS": "0"},
                        {"POMS_HOST_PARTIALS": "0", "POMS_ALPHA_FOLD": "0"}):
                with monkeypatch.context() as mp:
                    for k, v in env.items():
                        mp.setenv(k, v)
                    _same(_run(mp, A, b, xi, start, 0.0, MAXITER, skip, 3, False), ref, ("two launches", env))
                    got = _run(mp, A, b, xi, start, 0.0, MAXITER, skip, 3, True)
                    _same(got, ref, (layout, start, skip, env))
                    assert got[2] == MAXITER - 1


def test_p4_keeps_the_two_launches(gpu, monkeypatch):
    V, A, b, xi = _problem((11, 21, 13), 4, False, 0)
    ref = _run(monkeypatch, A, b, xi, "given", 0.0, MAXITER, True, 3, False)
    got = _run(monkeypatch, A, b, xi, "given", 0.0, MAXITER, True, 3, True)
    _same(got, ref, "p = 4")
    assert got[2] == 0, "p = 4 runs 8-wave tiles: no fused launch"
    w = [V.zeros() for _ in range(4)]
    assert not A.papply_dot_supported(*w)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_fused_launch_against_the_pair(gpu, layout):
    """The launch itself on random s, p and beta (every interior point non-zero): p_next, q and
    the sum of the dot's partials against V_PUPD followed by the apply + dot; the pads, ghost
    planes and dead pitch columns of p_next stay exactly zero."""
    import torch
    from poms_amd import _lib, runtime as rt
    shape, p, align, chunk = LAYOUTS[layout]
    V, A = _operator(shape, p, align, chunk)
    rng = np.random.default_rng(7)
    s = V.zeros().from_numpy(rng.standard_normal(shape))
    po = V.zeros().from_numpy(rng.standard_normal(shape))
    assert (s.to_local_numpy() != 0).all() and (po.to_local_numpy() != 0).all()
    ab = torch.tensor([0.0, float(rng.uniform(0.3, 1.7))], dtype=torch.float64, device=s._data.device)
    pn_ref, q_ref, pn, q = V.empty(), V.empty(), V.empty(), V.empty()
    for w in (pn_ref, q_ref, pn, q):
        V.interior(w._data).fill_(float("nan"))
    _lib.call("poms_pcg_p_update_dev", V.ctx, C.byref(V.layout), rt.ptr(ab), rt.ptr(s._data), rt.ptr(po._data),
              rt.ptr(pn_ref._data), rt.stream_handle())
    dot_ref = A.dot_inner(pn_ref, q_ref, device=True).clone()
    assert A.papply_dot_supported(s, po, pn, q)
    n0 = A.papply_dot_count
    dot = A.papply_dot(ab[1:2], s, po, pn, q)
    assert A.papply_dot_count == n0 + 1
    assert torch.isfinite(pn_ref._data).all() and torch.isfinite(q_ref._data).all()
    assert torch.equal(pn._data, pn_ref._data)
    assert torch.equal(q._data, q_ref._data)
    assert torch.equal(dot.reshape(-1), dot_ref.reshape(-1))
    st = pn._store.clone()
    V.interior(V.view(st)).zero_()
    assert not V.planes(st).any(), "p_next's ghosts or dead pitch columns were written"
    assert not V.view(st).any()


def test_whole_cycle_folded_against_not(gpu, monkeypatch):
    import torch
    from poms_amd.mg import TwoLevelVCycle
    mg = TwoLevelVCycle(3, 16, 4, ndim=3)
    b = mg.rhs_ones()
    monkeypatch.delenv("POMS_PCG_DEFER_X", raising=False)
    monkeypatch.setenv("POMS_PCG_PFOLD", "0")
    xr, pre_r, pos_r = mg.cycle(b)
    assert mg.A.papply_dot_count == 0
    monkeypatch.delenv("POMS_PCG_PFOLD")
    xd, pre_d, pos_d = mg.cycle(b)
    assert mg.A.papply_dot_count > 0
    assert torch.equal(xd._data, xr._data)
    assert pre_d == pre_r and pos_d == pos_r
