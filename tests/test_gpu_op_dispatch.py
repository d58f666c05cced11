"""The host side of an operator launch: what each kernel variant supports, the refusals with
their exact messages, and that a launch request reaches the kernels with no field transposed
(variant 8 against variant 9).  No diagnostic variant is launched."""
import ctypes as C

import numpy as np
import pytest

from poms_amd.splines import assemble_1d, make_open_knots, uniform_knots

pytestmark = pytest.mark.gpu

TOL = 1e-13   # one apply / residual / sweep, normwise relative (test_gpu_kernels.py)

KNOWN = [0, 4, 7, 8, 9, 10] + list(range(90, 115))
APPLY_DOT = {4, 8, 9, 10}
FUSED_DOT = {4, 7, 8, 9, 10, 114}
FROM_ZERO = {8, 9, 10, 110, 111, 112, 114}


def rel(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def kron(ndim, p, cells):
    from poms_amd.stencil import KronOperator, StencilVectorSpace
    M, K = assemble_1d(uniform_knots(p, cells), p)
    V = StencilVectorSpace([cells + p] * ndim, [p] * ndim)
    return KronOperator.laplace(V, [M] * ndim, [K] * ndim), V


def flags(A):
    return A.apply_dot_supported, A.fused_dot_supported, A.from_zero_supported


@pytest.mark.parametrize("ndim,p,cells", [(3, 2, 8), (2, 3, 16)])
def test_variant_capabilities(gpu, ndim, p, cells):
    from poms_amd import _lib
    A, _ = kron(ndim, p, cells)
    assert A.variant == 8   # pads == pmax
    for v in KNOWN:
        A.set_variant(v)
        assert A.variant == v
        assert flags(A) == (v in APPLY_DOT, v in FUSED_DOT, v in FROM_ZERO), v
    for v in (1, 2, 3, 5, 6, 11, 89, 115):
        with pytest.raises(_lib.PomsError, match="0, 4, 7, 8, 9, 10; 90-114 diagnostic"):
            A.set_variant(v)
        assert A.variant == KNOWN[-1]
    A.set_variant(8)
    assert A.variant == 8


def general_ops():
    from poms_amd.matfree import MatrixFreeOperator
    from poms_amd.stencil import StencilMatrix, StencilVectorSpace
    V = StencilVectorSpace([9, 12], [2, 3])
    return StencilMatrix(V), MatrixFreeOperator(V, [make_open_knots(2, 9), make_open_knots(3, 12)]), V


def test_general_forms_capabilities(gpu):
    """True / true / false whatever the variant field says (0 is the only value a general
    form's pads admit)."""
    S, F, _ = general_ops()
    for A in (S, F):
        assert flags(A) == (True, True, False)
        A.set_variant(0)
        assert flags(A) == (True, True, False)


def test_refusals(gpu):
    """Every refusal is decided on the host, before any launch."""
    from poms_amd import _lib, runtime as rt
    lib = _lib.lib
    st = rt.stream_handle()
    A3, V3 = kron(3, 2, 8)
    n0 = V3.npts[0]
    x, y, b = (V3.zeros() for _ in range(3))
    xp, yp, bp = rt.ptr(x._data), rt.ptr(y._data), rt.ptr(b._data)
    out = V3.scalar_buffer()
    o1, o2 = rt.ptr(out[0:1]), rt.ptr(out[1:2])

    def refused(rc, msg):
        assert rc != 0
        assert lib.poms_last_error().decode() == msg

    def reduce2(A, epi, xs, ys, bs, zb, ze, norm, dot):
        return lib.poms_op_run_reduce2(A._h, epi, 2.0 / 3.0, xs, ys, bs, zb, ze, 0, 0, norm, dot, 0, st)

    h = A3._h
    refused(reduce2(A3, 9, xp, yp, bp, 0, n0, None, None), "poms_op_run_reduce: bad epilogue")
    refused(reduce2(A3, 0, xp, yp, None, 0, n0, o1, None), "poms_op_run_reduce: apply has no reductions")
    refused(reduce2(A3, 4, xp, yp, xp, 0, n0, o1, o2), "apply + dot: dot_out only")
    refused(reduce2(A3, 4, xp, yp, xp, 0, n0, o1, None), "apply + dot: dot_out only")
    refused(reduce2(A3, 3, bp, yp, bp, 0, n0, o1, None), "jacobi from zero: both norms or neither")
    refused(reduce2(A3, 3, bp, yp, bp, 0, n0, None, o2), "jacobi from zero: both norms or neither")
    refused(reduce2(A3, 6, xp, yp, bp, 0, n0, None, None), "two sweeps per launch: 2D (planes [0, 1))")
    refused(reduce2(A3, 6, xp, yp, bp, 0, 1, None, None),
            "two sweeps per launch: one-rank 2D p = 3 Kronecker operators (variant 9) only")
    refused(lib.poms_op_jacobi_sweep(h, 2.0 / 3.0, bp, xp, xp, 0, n0, 0, st), "jacobi sweep: x_out must not alias x_in")
    A3.set_variant(7)
    refused(lib.poms_op_apply_dot(h, xp, yp, 0, n0, st), "apply + x.y: kernel variants 4, 8, 9, 10 only")
    refused(lib.poms_op_jacobi_from_zero(h, 2.0 / 3.0, bp, yp, 0, n0, 0, st),
            "jacobi from zero: not supported by this operator (poms_op_from_zero_supported)")
    A3.set_variant(8)
    refused(lib.poms_op_cheby_step(h, 0.5, 0.5, bp, xp, yp, 0, n0, st),
            "poms_op_cheby_step: Kronecker forms have no fused step (compose poms_op_jacobi_sweep and poms_vec_axpby)")
    refused(lib.poms_op_set_dirichlet(h, 1),
            "poms_op_set_dirichlet: Kronecker forms are constrained through their factors "
            "(needs a general-stencil or matrix-free operator)")
    _, F, V = general_ops()
    u, w = V.zeros(), V.zeros()
    refused(lib.poms_op_apply(F._h, rt.ptr(u._data), rt.ptr(w._data), 0, 0, st),
            "matrix-free operator: the plane range must be the whole axis 0")
    # nothing ran: the outputs are as they were
    assert not bool(y._data.any()) and not bool(w._data.any()) and not bool(out[0:2].any())


def test_request_reaches_the_kernels(gpu):
    """dot, residual, a sweep with both sums and two sweeps from zero: the default's pick
    (8: v5 here) against v3 (9)."""
    A, V = kron(3, 2, 8)
    rng = np.random.default_rng(17)
    x, b = (V.zeros().from_numpy(rng.uniform(-1, 1, V.npts)) for _ in range(2))
    om = 2.0 / 3.0

    def run(v):
        A.set_variant(v)
        y, r, s, z = (V.zeros() for _ in range(4))
        A.dot(x, out=y)
        A.residual(b, x, out=r)
        nrm, dot = A.jacobi_sweep(b, x, s, om, want_norm=True, want_dot=True)
        m1, m2 = A.jacobi_from_zero(b, z, om, want_norm=True)
        return [v.to_local_numpy() for v in (y, r, s, z)], [nrm, dot, m1, m2]

    vec8, sum8 = run(8)
    assert A.last_variant == 10
    vec9, sum9 = run(9)
    assert A.last_variant == 9
    A.set_variant(8)
    for name, a, c in zip(("dot", "residual", "jacobi_sweep", "jacobi_from_zero"), vec8, vec9):
        print(f"{name}: variant 8 against 9, relative difference {rel(a, c):.2e}")
        assert rel(a, c) <= TOL, name
    sv, bv = vec9[2], b.to_local_numpy()
    scale = [sum9[0], abs(sum9[1]) + np.linalg.norm(sv) * np.linalg.norm(bv), sum9[2], sum9[3]]
    for name, a, c, s in zip(("norm", "dot", "from zero 1", "from zero 2"), sum8, sum9, scale):
        print(f"{name}: {a!r} against {c!r}")
        assert abs(a - c) <= 1e-12 * s, name
