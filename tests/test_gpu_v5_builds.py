"""Every production selection of the v5 kernel (variant 10) launched once: p = 1..5, the
layout on which every lane's store is 16-B aligned (``align=True``) and one on which it
cannot be (an odd row pitch), axes 1 and 2 with equal Toeplitz rows (the SAME12 builds) and
with different ones, and per case every epilogue with and without its sums (the Jacobi
sweep's JDOT builds).  Two tile columns, so the per-column tables run beside the Toeplitz
fast path; several tile rows with a partial last one; about 2p + 6 cells on axis 0.

The reference is the flat v3 kernel (variant 9) on the same operator: vectors within the
project's 1e-13 (normwise relative), sums within 1e-12 of their scale
(tests/test_gpu_op_dispatch.py).  No diagnostic variant is launched.
"""
import numpy as np
import pytest

from poms_amd.splines import assemble_1d, uniform_knots

pytestmark = pytest.mark.gpu

TOL = 1e-13       # one apply / residual / sweep, normwise relative (test_gpu_kernels.py)
SUM_TOL = 1e-12   # a sum, relative to its scale (test_gpu_op_dispatch.py)
OMEGA = 2.0 / 3.0


def rel(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def cells_of(p, align, same12):
    """Cells per axis.  Axis 2 has 130, or 131 where 130 would make the unaligned row pitch
    (cells + 3p doubles) even and the 16-B stores possible after all."""
    c2 = 130 if align or (130 + 3 * p) % 2 else 131
    return (2 * p + 6, c2 if same12 else 24, c2)


@pytest.mark.parametrize("same12", [True, False], ids=["same-rows", "different-rows"])
@pytest.mark.parametrize("align", [True, False], ids=["aligned", "odd-pitch"])
@pytest.mark.parametrize("p", [1, 2, 3, 4, 5])
def test_every_production_build(gpu, p, align, same12):
    import torch
    from poms_amd.stencil import KronOperator, StencilVectorSpace
    cells = cells_of(p, align, same12)
    mats = [assemble_1d(uniform_knots(p, c), p) for c in cells]
    npts = [c + p for c in cells]
    V = StencilVectorSpace(npts, [p] * 3, align=align)
    if not align:
        assert V.pitch % 2 == 1
    A = KronOperator.laplace(V, [m[0] for m in mats], [m[1] for m in mats])
    rng = np.random.default_rng(100 * p + 10 * align + same12)
    x, b, s = (V.zeros().from_numpy(rng.uniform(-1, 1, npts)) for _ in range(3))
    beta = torch.tensor([float(rng.uniform(0.3, 1.7))], dtype=torch.float64, device=x._data.device)

    def run(v):
        A.set_variant(v)
        ran = []
        y, r, s1, s2, q, z, pn, pq = (V.zeros() for _ in range(8))
        A.dot(x, out=y)
        ran.append(A.last_variant)
        A.residual(b, x, out=r)
        ran.append(A.last_variant)
        assert A.jacobi_sweep(b, x, s1, OMEGA) is None   # no sums
        ran.append(A.last_variant)
        nrm, dot = A.jacobi_sweep(b, x, s2, OMEGA, want_norm=True, want_dot=True)
        ran.append(A.last_variant)
        xq = A.dot_inner(x, q)
        ran.append(A.last_variant)
        m1, m2 = A.jacobi_from_zero(b, z, OMEGA, want_norm=True)
        ran.append(A.last_variant)
        vecs = {"apply": y, "residual": r, "sweep": s1, "sweep + sums": s2, "apply + dot": q, "from zero": z}
        sums = {"norm": nrm, "dot": dot, "x.Ax": xq, "from zero 1": m1, "from zero 2": m2}
        if p <= 3:   # p_next = s + beta x, q = A p_next and p_next . q
            if v == 10:
                assert A.papply_dot_supported(s, x, pn, pq)
                sums["p.Ap"] = float(A.papply_dot(beta, s, x, pn, pq).item())
            else:
                pn.assign(x)
                pn.axpby_(1.0, s, float(beta.item()))
                sums["p.Ap"] = A.dot_inner(pn, pq)
            ran.append(A.last_variant)
            vecs["p_next"], vecs["A p_next"] = pn, pq
        assert ran == [v] * len(ran), ran
        return {k: w.to_local_numpy() for k, w in vecs.items()}, sums

    vec10, sum10 = run(10)
    vec9, sum9 = run(9)
    A.set_variant(8)
    for name in vec9:
        d = rel(vec10[name], vec9[name])
        print(f"{name}: variant 10 against 9, relative difference {d:.2e}")
        assert d <= TOL, name
    norm2 = lambda a: float(np.vdot(a, a))
    bn, xn = b.to_local_numpy(), x.to_local_numpy()
    scale = {"norm": sum9["norm"],
             "dot": abs(sum9["dot"]) + np.sqrt(norm2(vec9["sweep + sums"]) * norm2(bn)),
             "x.Ax": abs(sum9["x.Ax"]) + np.sqrt(norm2(xn) * norm2(vec9["apply + dot"])),
             "from zero 1": sum9["from zero 1"], "from zero 2": sum9["from zero 2"]}
    if p <= 3:
        scale["p.Ap"] = abs(sum9["p.Ap"]) + np.sqrt(norm2(vec9["p_next"]) * norm2(vec9["A p_next"]))
    for name in sum9:
        print(f"{name}: {sum10[name]!r} against {sum9[name]!r}")
        assert abs(sum10[name] - sum9[name]) <= SUM_TOL * scale[name], name
