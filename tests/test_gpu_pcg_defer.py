"""pcg's deferred x updates (``_defer_x``): with extra p buffers the native loop writes
``p_{k+1}`` beside ``p_k`` and forms ``x = x0 + sum alpha_k p_k`` in one pass per flush, with
the per-iteration update's fma per term.

Every comparison is deferred against ``POMS_PCG_DEFER_X=0`` (the per-iteration updates) in
the same process, ``torch.equal`` on the whole storage of ``x`` and ``==`` on ``info``: the
fma chain is the same, so there is no tolerance.
"""
import numpy as np
import pytest

from poms_amd.splines import assemble_1d, uniform_knots

pytestmark = pytest.mark.gpu

MAXITER = 7
BUFFERS = (2, 3, 7, 10)   # a flush mid-loop, one on the last iteration, more buffers than iterations

# name -> (DOF per axis, p, align)
LAYOUTS = {
    "3d-p3": ((19, 17, 23), 3, False),
    "3d-p3-aligned": ((19, 17, 23), 3, True),
    "3d-p2": ((12, 21, 13), 2, False),
    "3d-p2-aligned": ((12, 21, 13), 2, True),
    "2d-p3": ((33, 29), 3, True),   # (the V-cycles leave 2D alone: the buffers forced on)
}


# (powers of A applied to a normal b, scale of x0) to look for the stop branches among:
# r.r of pcg need not fall from one iteration to the next -- on the p = 2 space it rises
# for a normal b -- and does where r0 is rich in the operator's upper spectrum
CANDIDATES = [(0, 1.0), (1, 1.0), (2, 1.0), (2, 1e-3), (4, 1e-3)]


def _problem(shape, p, align, cand=CANDIDATES[0]):
    from poms_amd.stencil import KronOperator, StencilVectorSpace
    mats = [assemble_1d(uniform_knots(p, n - p), p) for n in shape]
    V = StencilVectorSpace(list(shape), [p] * len(shape), align=align)
    A = KronOperator.laplace(V, [m[0] for m in mats], [m[1] for m in mats])
    rng = np.random.default_rng(1000 * shape[0] + 10 * p)
    power, xscale = cand
    bn = rng.standard_normal(shape)
    for _ in range(power):
        bn = A.dot(V.zeros().from_numpy(bn)).to_local_numpy()
    b = V.zeros().from_numpy(bn)
    xi = V.zeros().from_numpy(xscale * rng.standard_normal(shape))
    return V, A, b, xi


def _run(monkeypatch, A, b, xi, start, tol, maxiter, skip, nbuf):
    """One pcg call; nbuf = 0: POMS_PCG_DEFER_X=0 with buffers asked for (the reference)."""
    import torch
    from poms_amd import solvers
    if nbuf:
        monkeypatch.delenv("POMS_PCG_DEFER_X", raising=False)
    else:
        monkeypatch.setenv("POMS_PCG_DEFER_X", "0")
    x0 = None if start == "none" else xi.copy() if start == "owned" else xi
    keep = xi._data.clone()
    x, info = solvers.pcg(A, solvers.damped_jacobi, b, x0=x0, tol=tol, maxiter=maxiter, _skip_tail=skip,
                          _x0_owned=start == "owned", _defer_x=nbuf or 3)
    assert torch.equal(xi._data, keep), "the caller's x0 was modified"
    return x, info


def _same(got, ref, what):
    import torch
    assert torch.equal(got[0]._data, ref[0]._data), what
    assert got[1] == ref[1], (what, got[1], ref[1])


def _stop_cases(monkeypatch, shape, p, align, start):
    """(problem, [(name, tol, maxiter)], jm, jl) for the three stop branches, from r.r per
    iteration on the DEFER_X=0 path: iteration j stops pcg when r.r_j < tol ||r0|| and no
    earlier one did, so j needs r.r_j below every earlier r.r, and tol ||r0|| between the
    two.  The first candidate right-hand side with two such j, the last of them >= 4."""
    tried = []
    for cand in CANDIDATES:
        V, A, b, xi = _problem(shape, p, align, cand)
        nrm0 = _run(monkeypatch, A, b, xi, start, 0.0, 0, True, 0)[1]["res_norm"]
        rr = [_run(monkeypatch, A, b, xi, start, 0.0, j, True, 0)[1]["res_norm"] ** 2 for j in range(1, MAXITER + 1)]
        firsts = [j for j in range(2, MAXITER + 1) if rr[j - 1] < (1.0 - 1e-6) * min(rr[:j - 1])]
        tried.append((cand, rr, firsts))
        if len(firsts) >= 2 and firsts[-1] >= 4:
            break
    else:
        pytest.fail(f"no candidate right-hand side reaches the stop branches: {tried}")
    tol_at = lambda j: 0.5 * (rr[j - 1] + min(rr[:j - 1])) / nrm0
    jl, jm = firsts[-1], min(firsts[:-1], key=lambda j: abs(j - 4))   # (the middle: after a first flush)
    return (V, A, b, xi), [("none", 0.0, MAXITER), ("middle", tol_at(jm), MAXITER), ("last", tol_at(jl), jl)], jm, jl


@pytest.mark.parametrize("start", ["none", "given", "owned"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_deferred_x_is_bitwise_neutral(gpu, monkeypatch, layout, start):
    shape, p, align = LAYOUTS[layout]
    (V, A, b, xi), cases, jm, jl = _stop_cases(monkeypatch, shape, p, align, start)
    seen = set()
    for name, tol, maxiter in cases:
        for skip in (False, True):
            ref = _run(monkeypatch, A, b, xi, start, tol, maxiter, skip, 0)
            # the case is the branch it is named after
            if name == "none":
                assert ref[1]["niter"] == maxiter and not ref[1]["success"], ref[1]
            elif name == "middle":
                assert ref[1]["success"] and ref[1]["niter"] == jm - 1 < maxiter - 1, ref[1]
            else:
                assert ref[1]["success"] and ref[1]["niter"] == maxiter - 1 == jl - 1, ref[1]
            seen.add((name, skip))
            for nbuf in BUFFERS:
                got = _run(monkeypatch, A, b, xi, start, tol, maxiter, skip, nbuf)
                _same(got, ref, (layout, start, name, skip, nbuf))
    assert seen == {(n, s) for n in ("none", "middle", "last") for s in (False, True)}


def _poison(A, V):
    """NaN in the interior of every p buffer A holds (the ghosts stay zero)."""
    for w in A._pcg_pbufs:
        V.interior(w._data).fill_(float("nan"))


def test_deferred_path_runs_and_its_fallbacks_agree(gpu, monkeypatch):
    """The buffers are written where the loop defers; the device-reduced norm-only pass
    (POMS_HOST_PARTIALS=0) and the unfolded alpha / beta kernels (POMS_ALPHA_FOLD=0: the
    paths the large grids take) give the same bits."""
    import torch
    shape, p, align = LAYOUTS["3d-p3-aligned"]
    V, A, b, xi = _problem(shape, p, align)
    for start in ("none", "given"):
        for skip in (False, True):
            ref = _run(monkeypatch, A, b, xi, start, 0.0, MAXITER, skip, 0)
            for env in ({}, {"POMS_HOST_PARTIALS": "0"}, {"POMS_ALPHA_FOLD": "0"},
                        {"POMS_HOST_PARTIALS": "0", "POMS_ALPHA_FOLD": "0"}):
                with monkeypatch.context() as mp:
                    for k, v in env.items():
                        mp.setenv(k, v)
                    _same(_run(mp, A, b, xi, start, 0.0, MAXITER, skip, 0), ref, ("reference", env))
                    _run(mp, A, b, xi, start, 0.0, 1, skip, 3)   # (allocates the buffers)
                    _poison(A, V)
                    _same(_run(mp, A, b, xi, start, 0.0, MAXITER, skip, 3), ref, (start, skip, env))
                    for w in A._pcg_pbufs[:3]:
                        assert torch.isfinite(w._data).all(), "a p buffer the deferred loop did not write"


def test_deferred_x_on_a_stored_stencil_operator(gpu, monkeypatch):
    """A general-form operator: alpha and beta from the one-thread scalar kernel."""
    from poms_amd.assembly import assemble_stencil
    shape, p, align = LAYOUTS["3d-p2"]
    V, _, b, xi = _problem(shape, p, align)
    S = assemble_stencil(V, [uniform_knots(p, n - p) for n in shape], a=lambda x, y, z: 1.0 + x * y + z)
    for start in ("none", "given"):
        for skip in (False, True):
            ref = _run(monkeypatch, S, b, xi, start, 0.0, MAXITER, skip, 0)
            for nbuf in (2, 10):
                _same(_run(monkeypatch, S, b, xi, start, 0.0, MAXITER, skip, nbuf), ref, (start, skip, nbuf))


@pytest.mark.parametrize("graph", ["0", "1"])
def test_speculative_and_graph_modes_keep_the_old_path(gpu, monkeypatch, graph):
    import torch
    shape, p, align = LAYOUTS["3d-p3"]
    V, A, b, xi = _problem(shape, p, align)
    ref = _run(monkeypatch, A, b, xi, "given", 0.0, 3, True, 0)
    _run(monkeypatch, A, b, xi, "given", 0.0, 1, True, 3)
    monkeypatch.setenv("POMS_PCG_SPEC", "1")
    monkeypatch.setenv("POMS_PCG_GRAPH", graph)
    for _ in range(2):   # (graph mode: the capture, then a replay)
        _poison(A, V)
        _same(_run(monkeypatch, A, b, xi, "given", 0.0, 3, True, 3), ref, graph)
        assert all(torch.isnan(V.interior(w._data)).all() for w in A._pcg_pbufs), "a p buffer was written"


def test_whole_cycle_deferred_against_not(gpu, monkeypatch):
    import torch
    from poms_amd.mg import TwoLevelVCycle
    mg = TwoLevelVCycle(3, 16, 4, ndim=3)
    b = mg.rhs_ones()
    monkeypatch.setenv("POMS_PCG_DEFER_X", "0")
    xr, pre_r, pos_r = mg.cycle(b)
    assert not getattr(mg.A, "_pcg_pbufs", None)
    monkeypatch.delenv("POMS_PCG_DEFER_X")
    xd, pre_d, pos_d = mg.cycle(b)
    assert len(mg.A._pcg_pbufs) == 10   # min(maxiter, 10), shared by both smoother calls
    assert torch.equal(xd._data, xr._data)
    assert pre_d == pre_r and pos_d == pos_r


def test_2d_cycles_do_not_defer(gpu, monkeypatch):
    from poms_amd.mg import TwoLevelVCycle
    monkeypatch.delenv("POMS_PCG_DEFER_X", raising=False)
    mg = TwoLevelVCycle(3, 32, 8, ndim=2)
    mg.cycle(mg.rhs_ones())
    assert not getattr(mg.A, "_pcg_pbufs", None)
