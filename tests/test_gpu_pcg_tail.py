"""pcg's ``_skip_tail``: iteration ``k == maxiter`` ends after ``x += alpha p`` and ``r.r``.

The reference goes on to ``s = psolve(A, r)``, ``s.r``, ``beta`` and ``p = s + beta p``
(`sources/solvers.py:117-124`), leaves the loop and returns ``x`` and ``info`` without
reading any of them.  Dropping them must not change a bit of what is returned, in any
of the three loops (Python host / device loop, native loop, native speculative loop).
"""
import ctypes as C

import numpy as np
import pytest

from poms_amd.splines import assemble_1d, make_open_knots, uniform_knots

pytestmark = pytest.mark.gpu

# name -> (POMS_NATIVE_PCG, POMS_PCG_LOOKAHEAD, POMS_PCG_SPEC, POMS_PCG_GRAPH)
MODES = {
    "python-la0": ("0", "0", "0", "0"),
    "python-la1": ("0", "1", "0", "0"),
    "native-la0": ("1", "0", "0", "0"),
    "native-la1": ("1", "1", "0", "0"),
    "spec": ("1", "0", "1", "0"),
    "spec-graph": ("1", "0", "1", "1"),
}


def _set_mode(monkeypatch, mode):
    native, la, spec, graph = MODES[mode]
    monkeypatch.setenv("POMS_NATIVE_PCG", native)
    monkeypatch.setenv("POMS_PCG_LOOKAHEAD", la)
    monkeypatch.setenv("POMS_PCG_SPEC", spec)
    monkeypatch.setenv("POMS_PCG_GRAPH", graph)
    monkeypatch.delenv("POMS_PCG_TAIL", raising=False)


def _problem(ndim, N, p, align=False, x0=False, scale=1.0):
    from poms_amd.stencil import KronOperator, StencilVectorSpace
    M, K = assemble_1d(uniform_knots(p, N), p)
    n = N + p
    V = StencilVectorSpace([n] * ndim, [p] * ndim, align=align)
    A = KronOperator.laplace(V, [M] * ndim, [K] * ndim)
    rng = np.random.default_rng(100 * N + p)
    b = V.zeros().from_numpy(scale * rng.standard_normal((n,) * ndim))
    xi = V.zeros().from_numpy(rng.standard_normal((n,) * ndim)) if x0 else None
    return V, A, b, xi


def _both(A, b, xi, tol, maxiter):
    """pcg without and with the flag: ((x, info), (x, info))."""
    from poms_amd import solvers
    out = []
    for skip in (False, True):
        x, info = solvers.pcg(A, solvers.damped_jacobi, b, x0=xi, tol=tol, maxiter=maxiter, _skip_tail=skip)
        out.append((x.to_local_numpy(), info))
        del x
    return out


def _assert_same(off, on):
    np.testing.assert_array_equal(on[0], off[0])
    for k in ("niter", "success", "res_norm"):
        assert on[1][k] == off[1][k], (k, on[1], off[1])


@pytest.mark.parametrize("ndim,N,p,align,x0,scale,tol,maxiter", [
    (3, 16, 3, False, False, 1.0, 1e-6, 3),
    (3, 20, 3, True, True, 1.0, 1e-6, 3),     # the V-cycle's layout: the flat kernel's misaligned head
    (2, 64, 3, False, False, 1.0, 1e-6, 3),
    (2, 24, 2, False, False, 1.0, 1e-6, 1),   # the only iteration is the last
    (2, 24, 2, False, False, 1.0, 1e-6, 0),   # no iteration at all
    # damped Jacobi stops after sweep 1: abandoned sweeps sit in front of the final pass
    # (tol = 0: at this scale r.r < 1e-6 ||r0|| would stop pcg in its first iteration)
    (3, 16, 3, False, False, 1e-9, 0.0, 3),
    # pcg stops early, the tail is never reached.  r.r < tol ||r0|| depends on the scale of
    # b: here r.r / scale^2 runs 2743, 966, 194, 135 (CPU oracle) and the test asks for
    # less than 0.5 sqrt(2743) / 0.164 = 160, so it fires in iteration 3
    (3, 12, 2, False, False, 0.164, 0.5, 10),
])
@pytest.mark.parametrize("mode", list(MODES))
def test_skip_tail_is_bitwise_neutral(gpu, monkeypatch, mode, ndim, N, p, align, x0, scale, tol, maxiter):
    _set_mode(monkeypatch, mode)
    V, A, b, xi = _problem(ndim, N, p, align, x0, scale)
    off, on = _both(A, b, xi, tol, maxiter)
    _assert_same(off, on)
    if tol == 0.5:
        assert off[1]["success"] and off[1]["niter"] == 2, off[1]
    else:
        assert off[1]["niter"] == maxiter and not off[1]["success"], off[1]


@pytest.mark.parametrize("mode", list(MODES))
def test_stop_test_fires_in_the_last_iteration(gpu, monkeypatch, mode):
    """maxiter = n + 1 where the stop test fires in iteration n + 1: niter == n and
    success, x updated, with and without the flag."""
    _set_mode(monkeypatch, mode)
    V, A, b, xi = _problem(3, 12, 2, scale=0.164)   # (fires in iteration 3, see above)
    early, _ = _both(A, b, xi, 0.5, 10)
    n = early[1]["niter"]
    assert early[1]["success"] and n == 2, early[1]
    off, on = _both(A, b, xi, 0.5, n + 1)
    _assert_same(off, on)
    _assert_same(early, on)
    assert on[1]["niter"] == n and on[1]["success"] is True
    assert off[1]["niter"] == n and off[1]["success"] is True


@pytest.mark.parametrize("cap", ["0", "16"])
def test_skip_tail_device_reduction_fallback(gpu, monkeypatch, cap):
    """POMS_HOST_PARTIALS = 0 / 16: the final pass through its device-reduced form."""
    _set_mode(monkeypatch, "native-la0")
    monkeypatch.setenv("POMS_HOST_PARTIALS", cap)
    V, A, b, xi = _problem(3, 20, 3)
    off, on = _both(A, b, xi, 1e-6, 3)
    _assert_same(off, on)
    monkeypatch.setenv("POMS_NATIVE_PCG", "0")
    _, py = _both(A, b, xi, 1e-6, 3)
    _assert_same(py, on)


def test_all_loops_agree_with_the_flag(gpu, monkeypatch):
    """The three loops stay bitwise equal to one another with the flag set."""
    V, A, b, xi = _problem(3, 20, 3, align=True, x0=True)
    res = {}
    for mode in MODES:
        _set_mode(monkeypatch, mode)
        res[mode] = _both(A, b, xi, 1e-6, 3)[1]
    for mode in MODES:
        _assert_same(res["python-la0"], res[mode])


def _rel(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


@pytest.mark.parametrize("p,ne", [(1, 4), (1, 16), (3, 8)])
def test_skip_tail_against_reference_outputs(gpu, golden_dir, p, ne):
    """The reference's own pcg outputs (tests/golden/solvers_2d.npz), with the bound of
    tests/test_gpu_golden.py."""
    from poms_amd.solvers import damped_jacobi, pcg
    from poms_amd.stencil import KronOperator, StencilVectorSpace
    z = np.load(golden_dir / "solvers_2d.npz", allow_pickle=False)
    M, K = assemble_1d(make_open_knots(p, ne + p), p)
    n = ne + p
    V = StencilVectorSpace([n, n], [p, p])
    A = KronOperator.laplace(V, [M, M], [K, K])
    for rhs in ("manuf", "ones"):
        case = f"p{p}_ne{ne}_{rhs}"
        b = V.zeros().from_numpy(z[f"{case}__b"].reshape(n, n))
        for m in (1, 2, 5):
            x, info = pcg(A, damped_jacobi, b, tol=0.0, maxiter=m, _skip_tail=True)
            assert info["niter"] == int(z[f"{case}__pcg_m{m}_tol0_info"][0])
            assert _rel(x.to_local_numpy().reshape(-1), z[f"{case}__pcg_m{m}_tol0"]) <= 1e-10, (rhs, m)


def test_skip_tail_launch_counts(gpu, monkeypatch):
    """With the flag a pcg(maxiter=3) call runs 3 preconditioner calls of 8 sweep
    launches (after sweeps 1-2 from zero) and 3 apply + dot launches; without it,
    3 + 1 preconditioner calls as before."""
    _set_mode(monkeypatch, "native-la0")
    monkeypatch.delenv("POMS_PCG_LOOKAHEAD")
    from poms_amd import solvers
    V, A, b, _ = _problem(3, 16, 3)
    for skip, want in ((True, 3 * 8), (False, 4 * 8)):
        A.timing(True)
        solvers.pcg(A, solvers.damped_jacobi, b, tol=1e-6, maxiter=3, _skip_tail=skip)
        A.timing(False)
        assert A.timing_read("jacobi")[1] == want, skip
        assert A.timing_read("apply_dot")[1] == 3, skip


def _cycle_both(monkeypatch, mg):
    out = {}
    b = mg.rhs_ones()
    for tail in ("1", "0"):
        monkeypatch.setenv("POMS_PCG_TAIL", tail)
        res = mg.cycle(b)
        out[tail] = (res[0].to_local_numpy(), res[1:])
    np.testing.assert_array_equal(out["0"][0], out["1"][0])
    assert out["0"][1] == out["1"][1]
    return out


@pytest.mark.parametrize("args,kw", [
    ((3, 16, 4), {"ndim": 3}),
    ((3, 32, 8), {"ndim": 2}),
    ((3, 32, 8), {"ndim": 2, "post_smoother": "glt"}),
])
def test_vcycle_same_with_and_without_the_tail(gpu, monkeypatch, args, kw):
    """cycle() with the reference's full last iteration (POMS_PCG_TAIL=1) and without it."""
    from poms_amd.mg import TwoLevelVCycle
    _cycle_both(monkeypatch, TwoLevelVCycle(*args, **kw))


def test_multilevel_vcycle_same_with_and_without_the_tail(gpu, monkeypatch):
    from poms_amd.mg import MultilevelVCycle
    mg = MultilevelVCycle(3, 32, 8, ndim=2)
    assert mg.nlevels == 3
    _cycle_both(monkeypatch, mg)


def test_vcycle_tail_knob_changes_the_launches(gpu, monkeypatch):
    """POMS_PCG_TAIL=1 does bring the skipped preconditioner call back (the A/B compares
    two different launch sequences)."""
    from poms_amd.mg import TwoLevelVCycle
    mg = TwoLevelVCycle(3, 16, 4, ndim=3, maxiter=2)
    b = mg.rhs_ones()
    counts = {}
    for tail in ("1", "0"):
        monkeypatch.setenv("POMS_PCG_TAIL", tail)
        mg.A.timing(True)
        mg.cycle(b)
        mg.A.timing(False)
        counts[tail] = mg.A.timing_read("jacobi")[1]
    assert counts["1"] - counts["0"] == 2 * 8, counts


@pytest.mark.parametrize("shape,pads,align", [((9, 7, 70), (2, 2, 2), False), ((5, 6, 21), (3, 3, 3), True)])
def test_final_update_per_row_kernel(gpu, shape, pads, align):
    """poms_pcg_final_update_dev on a layout whose ghosts hold data (the per-row kernel):
    x + a p with one fma per element (bitwise), sum((r - a q)^2) to 1e-14."""
    from fractions import Fraction

    import torch
    from poms_amd import _lib, runtime as rt
    from poms_amd.stencil import StencilVectorSpace
    V = StencilVectorSpace(list(shape), list(pads), align=align)
    lay = _lib.Layout.make(V.n3, V.p3, V.pitch if V.aligned else 0, _lib.LAYOUT_GHOST_DATA)
    rng = np.random.default_rng(5)
    h = {k: rng.standard_normal(shape) for k in "xprq"}
    v = {k: V.zeros().from_numpy(h[k]) for k in "xprq"}
    a = 0.37
    alpha = torch.tensor([a], dtype=torch.float64, device=v["x"]._data.device)
    out = torch.zeros(1, dtype=torch.float64, device=alpha.device)
    _lib.call("poms_pcg_final_update_dev", V.ctx, C.byref(lay), rt.ptr(alpha), rt.ptr(v["x"]._data),
              rt.ptr(v["p"]._data), rt.ptr(v["r"]._data), rt.ptr(v["q"]._data), rt.ptr(out), rt.stream_handle())
    v["x"]._mark_written()
    # fma(a, p, x): the exact a p + x in rationals, rounded once (float(Fraction) rounds correctly)
    fa = Fraction(a)
    want = np.array([float(fa * Fraction(pv) + Fraction(xv))
                     for pv, xv in zip(h["p"].ravel(), h["x"].ravel())]).reshape(shape)
    got = v["x"].to_local_numpy()
    np.testing.assert_array_equal(got, want)
    # r's buffer: x as pcg's early-stop update rounds it -- the product, then the sum (numpy's own order)
    v["r"]._mark_written()
    alt = h["x"] + a * h["p"]
    np.testing.assert_array_equal(v["r"].to_local_numpy(), alt)
    assert np.any(alt != want) and _rel(got, alt) <= 1e-15
    s = float(np.sum((h["r"] - a * h["q"]) ** 2))
    assert abs(float(out.item()) - s) <= 1e-14 * s
