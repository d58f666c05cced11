"""pcg's r update formed inside the first psolve launch (``EPI_RJACOBI0``, ``_fold_r``, ``POMS_PCG_RFOLD``).

On the deferred path the native loop used to write ``r -= alpha q`` with the flat ``V_RUPD``
launch and read ``r`` straight back as the right-hand side of the two sweeps from zero.  Where
those sweeps run v5's p = 3 16-wave build on one rank, the loop now starts the psolve with one
launch that forms ``r_new = r - alpha q`` in its LDS ring with ``V_RUPD``'s fma, stores the
interior points into the other of two r buffers and goes on as the two sweeps on ``r_new``.
``r . r`` comes back added in tile order; the loop decides the stop test from it only outside a
guard band around the threshold and forms ``V_RUPD``'s own sum from the stored ``r_new`` inside it.

Every comparison of the loop is ``_fold_r`` against ``POMS_PCG_RFOLD=0`` (the two launches) in
the same process, ``torch.equal`` on the whole storage of ``x`` and ``==`` on ``info``: no
tolerance.  The one bound is the launch's tile-order sum against the flat one: both add the
same m non-negative terms, each within gamma_m = m u / (1 - m u) of the exact sum (u = 2^-53),
so they differ by at most g = 4 m u of the flat sum, m the length of the flat range (whole
interior planes, pads included) -- the guard the loop derives.

Shapes (DOF extents), the smallest at which each mechanism of the kernel can fail --

* (12, 19, 118), chunk 6: two chunks of axis 0 (their halo planes must not be stored or summed),
  two row tiles, the second with 3 rows (waves without an output row of their own still combine
  and store the rows they own), two column tiles, on both layouts (16-B and 8-B stores);
* (9, 17, 20): one tile, one chunk, no row inside the Toeplitz interior
  (axes 1 and 2 share their cell width: the 16-wave build runs only where their rows agree);
* p = 2 and p = 4 spaces: keep the two launches.
"""
import numpy as np
import pytest

from poms_amd.splines import assemble_1d, uniform_knots

pytestmark = pytest.mark.gpu

MAXITER = 7
BUFFERS = (2, 3, 10)
OMEGA = 2.0 / 3.0

# name -> (DOF per axis, p, align, chunk)
LAYOUTS = {
    "p3-two-chunks": ((12, 19, 118), 3, False, 6),
    "p3-two-chunks-aligned": ((12, 19, 118), 3, True, 6),
    "p3-one-tile": ((9, 17, 20), 3, False, 0),
}
FIRST = ("p3-two-chunks", "p3-two-chunks-aligned")
OTHER_DEGREES = {"p2": ((11, 21, 13), 2, False, 0), "p4": ((11, 21, 13), 4, False, 0)}

# (powers of A applied to a normal b, scale of x0) to look for the stop branches among (as
# test_gpu_pcg_defer.py: r.r of pcg need not fall from one iteration to the next)
CANDIDATES = [(0, 1.0), (1, 1.0), (2, 1.0), (2, 1e-3), (4, 1e-3)]


def _factors(shape, p):
    """Mass and stiffness bands per axis.  The fused launch needs axes 1 and 2 to share their
    interior rows bitwise (one cell width on both), so where both axes are long enough the shorter
    one's bands are cut out of the longer one's: its first and last 2p rows, and its Toeplitz row
    between them -- the matrices of the same knots with fewer cells."""
    mats = [assemble_1d(uniform_knots(p, n - p), p) for n in shape]
    lo, hi = sorted((1, 2), key=lambda d: shape[d])
    if shape[lo] >= 4 * p and shape[lo] != shape[hi]:
        def cut(band):
            mid = band[band.shape[0] // 2]
            return np.concatenate([band[:2 * p], np.repeat(mid[None], shape[lo] - 4 * p, axis=0), band[-2 * p:]])
        mats[lo] = tuple(cut(band) for band in mats[hi])
    return mats


def _operator(shape, p, align, chunk):
    from poms_amd.stencil import KronOperator, StencilVectorSpace
    mats = _factors(shape, p)
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


def _guard(V):
    """g = 4 m 2^-53, m the doubles of the flat range (the loop's dcount)."""
    return 4.0 * V.local_npts[0] * V.plane_elems * 2.0 ** -53


def _run(monkeypatch, A, b, xi, start, tol, maxiter, nbuf, fused, skip=True):
    """One pcg call with ``nbuf`` p buffers and ``_fold_r`` -> (x, info, fused launches, exact passes)."""
    import torch
    from poms_amd import solvers
    monkeypatch.delenv("POMS_PCG_DEFER_X", raising=False)
    if fused:
        monkeypatch.delenv("POMS_PCG_RFOLD", raising=False)
    else:
        monkeypatch.setenv("POMS_PCG_RFOLD", "0")
    x0 = None if start == "none" else xi.copy() if start == "owned" else xi
    keep = xi._data.clone()
    n0, e0 = A.rjacobi0_count
    x, info = solvers.pcg(A, solvers.damped_jacobi, b, x0=x0, tol=tol, maxiter=maxiter, _skip_tail=skip,
                          _x0_owned=start == "owned", _defer_x=nbuf, _fold_r=True)
    assert torch.equal(xi._data, keep), "the caller's x0 was modified"
    n1, e1 = A.rjacobi0_count
    return x, info, n1 - n0, e1 - e0


def _same(got, ref, what):
    import torch
    assert torch.equal(got[0]._data, ref[0]._data), what
    assert got[1] == ref[1], (what, got[1], ref[1])
    assert ref[2] == 0 and ref[3] == 0, (what, "POMS_PCG_RFOLD=0 ran the fused launch")


_CASES = {}


def _stop_cases(monkeypatch, layout, start):
    """(problem, [(name, tol, maxiter)], jm, jl, rr, nrm0): no stop, a stop in the middle, a stop in
    iteration maxiter -- from r.r per iteration on the two-launch path (iteration j stops pcg
    when r.r_j < tol ||r0|| and no earlier one did).  Found once per (layout, start)."""
    if (layout, start) in _CASES:
        return _CASES[layout, start]
    shape, p, align, chunk = LAYOUTS[layout]
    tried = []
    for cand in CANDIDATES:
        V, A, b, xi = _problem(shape, p, align, chunk, cand)
        nrm0 = _run(monkeypatch, A, b, xi, start, 0.0, 0, 3, False)[1]["res_norm"]
        rr = [_run(monkeypatch, A, b, xi, start, 0.0, j, 3, False)[1]["res_norm"] ** 2 for j in range(1, MAXITER + 1)]
        firsts = [j for j in range(2, MAXITER + 1) if rr[j - 1] < (1.0 - 1e-6) * min(rr[:j - 1])]
        tried.append((cand, rr, firsts))
        if len(firsts) >= 2 and firsts[-1] >= 4:
            break
    else:
        pytest.fail(f"no candidate right-hand side reaches the stop branches: {tried}")
    tol_at = lambda j: 0.5 * (rr[j - 1] + min(rr[:j - 1])) / nrm0
    jl, jm = firsts[-1], min(firsts[:-1], key=lambda j: abs(j - 4))
    cases = [("none", 0.0, MAXITER), ("middle", tol_at(jm), MAXITER), ("last", tol_at(jl), jl)]
    _CASES[layout, start] = (V, A, b, xi), cases, jm, jl, rr, nrm0
    return _CASES[layout, start]


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_fused_launch_against_the_pair(gpu, layout):
    """The launch itself on random r, q and alpha (every interior point non-zero): r_new, x2 and
    J0's two sums against V_RUPD followed by the two sweeps from zero, bitwise; the tile-order sum
    against V_RUPD's within g; the pads, ghost planes and dead pitch columns of r_new exactly zero."""
    import torch
    from poms_amd.solvers import _pcg_r_update_dev
    shape, p, align, chunk = LAYOUTS[layout]
    V, A = _operator(shape, p, align, chunk)
    rng = np.random.default_rng(11)
    r = V.zeros().from_numpy(rng.standard_normal(shape))
    q = V.zeros().from_numpy(rng.standard_normal(shape))
    assert (r.to_local_numpy() != 0).all() and (q.to_local_numpy() != 0).all()
    alpha = torch.tensor([float(rng.uniform(0.3, 1.7))], dtype=torch.float64, device=r._data.device)
    r_ref, x_ref, rn, x2 = r.copy(), V.empty(), V.empty(), V.empty()
    for w in (x_ref, rn, x2):
        V.interior(w._data).fill_(float("nan"))
    rr_ref = float(_pcg_r_update_dev(V, alpha, r_ref, q))
    x1_ref, dr2_ref = A.jacobi_from_zero(r_ref, x_ref, OMEGA, want_norm=True)
    assert A.rjacobi0_supported(r, q, rn, x2)
    n0 = A.rjacobi0_count[0]
    keep_r, keep_q = r._store.clone(), q._store.clone()
    sums = A.rjacobi0(alpha, r, q, rn, x2, OMEGA).cpu().numpy()
    assert A.rjacobi0_count[0] == n0 + 1
    assert torch.equal(r._store, keep_r) and torch.equal(q._store, keep_q)
    assert torch.isfinite(r_ref._data).all() and torch.isfinite(x_ref._data).all()
    assert torch.equal(rn._data, r_ref._data)
    assert torch.equal(x2._data, x_ref._data)
    assert sums[0] == dr2_ref and sums[1] == x1_ref, (sums, dr2_ref, x1_ref)
    print(f"{layout}: tile-order {sums[2]!r} flat {rr_ref!r} rel {abs(sums[2] - rr_ref) / rr_ref:.3e} g {_guard(V):.3e}")
    assert abs(sums[2] - rr_ref) <= _guard(V) * rr_ref
    st = rn._store.clone()
    V.interior(V.view(st)).zero_()
    assert not V.planes(st).any(), "r_new's ghosts or dead pitch columns were written"
    assert not V.view(st).any()
    # without sums: the same vectors
    rn2, x3 = V.empty(), V.empty()
    assert A.rjacobi0(alpha, r, q, rn2, x3, OMEGA, sums=False) is None
    assert torch.equal(rn2._data, r_ref._data) and torch.equal(x3._data, x_ref._data)


@pytest.mark.parametrize("start", ["none", "given", "owned"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_folded_r_update_is_bitwise_neutral(gpu, monkeypatch, layout, start):
    """maxiter 7 with 2, 3 and 10 p buffers: no stop, a stop in the middle and one in iteration
    maxiter; the number of fused launches in each."""
    (V, A, b, xi), cases, jm, jl, _, _ = _stop_cases(monkeypatch, layout, start)
    for name, tol, maxiter in cases:
        for nbuf in BUFFERS:
            ref = _run(monkeypatch, A, b, xi, start, tol, maxiter, nbuf, False)
            if name == "none":
                assert ref[1]["niter"] == maxiter and not ref[1]["success"], ref[1]
            elif name == "middle":
                assert ref[1]["success"] and ref[1]["niter"] == jm - 1 < maxiter - 1, ref[1]
            else:
                assert ref[1]["success"] and ref[1]["niter"] == maxiter - 1 == jl - 1, ref[1]
            got = _run(monkeypatch, A, b, xi, start, tol, maxiter, nbuf, True)
            _same(got, ref, (layout, start, name, nbuf))
            # every iteration before iteration maxiter starts its psolve with the fused launch
            stop = maxiter if name == "none" else ref[1]["niter"] + 1   # the iteration the loop leaves in
            assert got[2] == min(stop, maxiter - 1), (layout, start, name, nbuf, got[2])
            # the exact pass runs where the tile-order sum is not clear of the threshold: in the
            # iteration that stops (the one in iteration maxiter is the norm-only pass's), never else
            # at these thresholds (half way between two iterations' r.r)
            assert got[3] == (1 if name == "middle" else 0), (layout, start, name, nbuf, got[3])


@pytest.mark.parametrize("layout", FIRST)
def test_without_skip_tail_fold_r_is_ignored(gpu, monkeypatch, layout):
    shape, p, align, chunk = LAYOUTS[layout]
    V, A, b, xi = _problem(shape, p, align, chunk)
    ref = _run(monkeypatch, A, b, xi, "given", 0.0, MAXITER, 3, False, skip=False)
    got = _run(monkeypatch, A, b, xi, "given", 0.0, MAXITER, 3, True, skip=False)
    _same(got, ref, layout)
    assert got[2] == 0 and got[3] == 0
    # ... and so it is without p buffers (no deferred x updates)
    got = _run(monkeypatch, A, b, xi, "given", 0.0, MAXITER, 0, True)
    assert got[2] == 0 and got[3] == 0


@pytest.mark.parametrize("layout", FIRST)
def test_guard_band(gpu, monkeypatch, layout):
    """The threshold tol ||r0|| a hair (1e-13: far inside g, far outside the rounding of the
    recorded r.r) above and below iteration jm's exact r.r: the tile-order sum cannot decide, the
    exact pass runs, and the loop stops (above) or goes on (below) exactly as the two launches do."""
    (V, A, b, xi), cases, jm, jl, rr, nrm0 = _stop_cases(monkeypatch, layout, "given")
    assert 1e-13 < 1e-2 * _guard(V)
    outcomes = []
    for eps in (1e-13, -1e-13):
        tol = rr[jm - 1] * (1.0 + eps) / nrm0
        ref = _run(monkeypatch, A, b, xi, "given", tol, MAXITER, 3, False)
        got = _run(monkeypatch, A, b, xi, "given", tol, MAXITER, 3, True)
        _same(got, ref, (layout, eps))
        assert got[3] >= 1, "the exact r.r pass did not run inside the guard band"
        outcomes.append(ref[1]["niter"])
    assert outcomes[0] == jm - 1, ("just above: stops in iteration jm", outcomes)
    assert outcomes[1] > jm - 1, ("just below: goes on", outcomes)


@pytest.mark.parametrize("layout", FIRST)
def test_scalar_kernel_paths_agree(gpu, monkeypatch, layout):
    """POMS_ALPHA_FOLD 0 and 1 and POMS_HOST_PARTIALS=0 (the paths the large grids take), with a
    threshold in the guard band so that the exact pass takes those paths too."""
    (V, A, b, xi), cases, jm, jl, rr, nrm0 = _stop_cases(monkeypatch, layout, "given")
    for start in ("none", "given"):
        for tol in ((0.0, rr[jm - 1] * (1.0 - 1e-13) / nrm0) if start == "given" else (0.0,)):
            ref = _run(monkeypatch, A, b, xi, start, tol, MAXITER, 3, False)
            for env in ({"POMS_ALPHA_FOLD": "1"}, {"POMS_ALPHA_FOLD": "0"}, {"POMS_HOST_PARTIALS": "0"},
                        {"POMS_HOST_PARTIALS": "0", "POMS_ALPHA_FOLD": "0"}):
                with monkeypatch.context() as mp:
                    for k, v in env.items():
                        mp.setenv(k, v)
                    got = _run(mp, A, b, xi, start, tol, MAXITER, 3, True)
                    _same(got, ref, (layout, start, tol, env))
                    assert got[2] >= 1
                    assert got[3] >= (1 if tol else 0)


@pytest.mark.parametrize("name", list(OTHER_DEGREES))
def test_other_degrees_keep_the_two_launches(gpu, monkeypatch, name):
    shape, p, align, chunk = OTHER_DEGREES[name]
    V, A, b, xi = _problem(shape, p, align, chunk)
    ref = _run(monkeypatch, A, b, xi, "given", 0.0, MAXITER, 3, False)
    got = _run(monkeypatch, A, b, xi, "given", 0.0, MAXITER, 3, True)
    _same(got, ref, name)
    assert got[2] == 0 and got[3] == 0, "only the p = 3 16-wave build has the fused launch"
    w = [V.zeros() for _ in range(4)]
    assert not A.rjacobi0_supported(*w)


@pytest.mark.parametrize("graph", ["0", "1"])
def test_speculative_and_graph_modes_keep_the_old_path(gpu, monkeypatch, graph):
    shape, p, align, chunk = LAYOUTS["p3-two-chunks"]
    V, A, b, xi = _problem(shape, p, align, chunk)
    ref = _run(monkeypatch, A, b, xi, "given", 0.0, 3, 3, False)
    monkeypatch.setenv("POMS_PCG_SPEC", "1")
    monkeypatch.setenv("POMS_PCG_GRAPH", graph)
    for _ in range(2):   # (graph mode: the capture, then a replay)
        got = _run(monkeypatch, A, b, xi, "given", 0.0, 3, 3, True)
        _same(got, ref, graph)
        assert got[2] == 0 and got[3] == 0


def test_ghost_data_operator_is_not_supported(gpu):
    """A Cart block whose ghost rows and columns hold the neighbours' data: no fused launch."""
    from poms_amd.dist import CartDistribution
    from poms_amd.stencil import KronOperator, StencilVectorSpace
    p, shape = 3, (12, 38, 40)
    mats = [assemble_1d(uniform_knots(p, n - p), p) for n in shape]
    V = StencilVectorSpace(list(shape), [p] * 3, dist=CartDistribution(shape, (1, 2, 2), 0))
    A = KronOperator.laplace(V, [m[0] for m in mats], [m[1] for m in mats])
    w = [V.zeros() for _ in range(4)]
    assert not A.rjacobi0_supported(*w)
    assert A.rjacobi0_count == (0, 0)


def test_whole_cycle_folded_against_not(gpu, monkeypatch):
    import torch
    from poms_amd.mg import TwoLevelVCycle
    mg = TwoLevelVCycle(3, 16, 4, ndim=3)
    b = mg.rhs_ones()
    monkeypatch.delenv("POMS_PCG_DEFER_X", raising=False)
    monkeypatch.setenv("POMS_PCG_RFOLD", "0")
    xr, pre_r, pos_r = mg.cycle(b)
    assert mg.A.rjacobi0_count == (0, 0)
    monkeypatch.delenv("POMS_PCG_RFOLD")
    xd, pre_d, pos_d = mg.cycle(b)
    assert mg.A.rjacobi0_count[0] > 0
    assert torch.equal(xd._data, xr._data)
    assert pre_d == pre_r and pos_d == pos_r
