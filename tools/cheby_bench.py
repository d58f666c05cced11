#!/usr/bin/env python
"""The Chebyshev-Jacobi smoother on one MI355X (not part of bench.py).

1. The fused step (``A.cheby_step``, EPI_CHEBY) against ``A.jacobi_sweep`` without its norm,
   stored stencil and matrix-free, 3D 131^3 and 2D 1027^2 at p = 3: the operators take turns
   call by call, device events around each call, the L2 / MALL flushed before every timed
   call by filling a 512 MiB buffer, medians of ``--reps`` (>= 7).  A second sweep on a second
   operator of the same form runs in the rotation: the sweep's own spread.  The composed
   step of the Kronecker operator at 515^3 is recorded as a plain number.
2. Cycles and wall time to ``||r|| <= 1e-10 ||b||``: the Dirichlet problems of §3.16 (unit
   square, all faces, p = 1, 2, 3, N = 8, 16, case (a)) and the variable-coefficient problem
   of §3.14 (3D 128^3 cells, p = 3, b = 1), the default smoother (pcg + damped Jacobi, 4
   resp. 2 iterations per smoothing as those sections ran them) against Chebyshev at degree
   4 and 10, ratio 10 and 30.

    python tools/cheby_bench.py [--out profiles/cheby/cheby_bench.json] [--skip-big]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch


def a_coef(x, y, *z):
    return (1.0 + 0.5 * np.sin(3 * x) * np.cos(2 * y)) * (1.0 + z[0] / 4 if z else 1.0)


def c_coef(x, y, *z):
    return 2.0 + x * y


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, default=3)
    ap.add_argument("--cells3", type=int, default=128)
    ap.add_argument("--cells2", type=int, default=1024)
    ap.add_argument("--cells-kron", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--flush-mib", type=int, default=512)
    ap.add_argument("--max-cycles", type=int, default=40)
    ap.add_argument("--skip-big", action="store_true", help="leave out the 128^3 cycles")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("cheby_bench needs a GPU: times are not taken on a CPU")
    from poms_amd.assembly import assemble_stencil
    from poms_amd.boundary import DirichletBC
    from poms_amd.field import assemble_rhs
    from poms_amd.matfree import MatrixFreeOperator, MatrixFreeVCycle
    from poms_amd.mg import GalerkinVCycle
    from poms_amd.splines import assemble_1d, uniform_knots
    from poms_amd.stencil import KronOperator, StencilVectorSpace

    torch.cuda.set_device(0)
    dev = "cuda:0"
    p = a.p
    flush = torch.empty(a.flush_mib << 17, dtype=torch.float64, device=dev) if a.flush_mib else None

    def interleaved(fns):
        """Median ms of every callable, the callables taking turns rep by rep."""
        ts = {k: [] for k in fns}
        for i in range(a.warmup + a.reps):
            for k, fn in fns.items():
                if flush is not None:
                    flush.fill_(float(i))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    ts[k].append(e0.elapsed_time(e1))
        return {k: {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ts.items()}

    res = {"device": torch.cuda.get_device_name(0), "p": p, "reps": a.reps, "flush_mib": a.flush_mib, "step": {},
           "cycles": {}}

    # ---- 1. the step against the sweep ------------------------------------------------
    for ndim, cells in ((3, a.cells3), (2, a.cells2)):
        T = uniform_knots(p, cells)
        V = StencilVectorSpace([cells + p] * ndim, [p] * ndim, align=True)
        rng = np.random.default_rng(0)
        x, b = (V.zeros().from_numpy(rng.uniform(-1, 1, V.npts)) for _ in range(2))
        y = V.zeros().from_numpy(rng.uniform(-1, 1, V.npts))
        cfg = {"cells": cells, "ndof": V.dimension}
        for form, make in (("matfree", lambda: MatrixFreeOperator(V, [T] * ndim, a=a_coef, c=c_coef)),
                           ("stencil", lambda: assemble_stencil(V, [T] * ndim, a=a_coef, c=c_coef))):
            A, B = make(), make()
            t = interleaved({"jacobi_sweep": lambda: A.jacobi_sweep(b, x, y, 2.0 / 3.0),
                             "jacobi_sweep_again": lambda: B.jacobi_sweep(b, x, y, 2.0 / 3.0),
                             "cheby_step": lambda: A.cheby_step(b, x, y, 0.4, 0.5),
                             "cheby_step_beta0": lambda: A.cheby_step(b, x, y, 0.4, 0.0)})
            sw = [t["jacobi_sweep"], t["jacobi_sweep_again"]]
            t["sweep_spread_ms"] = max(s["max_ms"] for s in sw) - min(s["min_ms"] for s in sw)
            t["step_minus_sweep_ms"] = t["cheby_step"]["ms"] - t["jacobi_sweep"]["ms"]
            t["extra_8B_per_dof_at_4TBs_ms"] = 8.0 * V.dimension / 4e12 * 1e3
            cfg[form] = t
            del A, B
        res["step"][f"{ndim}d_p{p}_{cells}"] = cfg
        print(json.dumps({f"step_{ndim}d_p{p}_{cells}": cfg}), flush=True)
        del x, b, y
    # the composed step of the Kronecker form
    N = a.cells_kron
    M, K = assemble_1d(uniform_knots(p, N), p)
    V = StencilVectorSpace([N + p] * 3, [p] * 3, align=True)
    A = KronOperator.laplace(V, [M] * 3, [K] * 3)
    rng = np.random.default_rng(0)
    x, b, y = (V.zeros().from_numpy(rng.uniform(-1, 1, V.npts)) for _ in range(3))
    w = V.empty()
    t = interleaved({"jacobi_sweep": lambda: A.jacobi_sweep(b, x, y, 2.0 / 3.0),
                     "cheby_step_composed": lambda: A.cheby_step(b, x, y, 0.4, 0.5, work=w)})
    res["step"][f"kron_3d_p{p}_{N}"] = dict(t, cells=N, ndof=V.dimension)
    print(json.dumps({f"step_kron_3d_p{p}_{N}": t}), flush=True)
    del A, x, b, y, w

    # ---- 2. cycles and wall time to 1e-10 ||b|| ----------------------------------------
    def solve(mg, b):
        nb = float(np.sqrt(b.dot(b)))
        x, k, hist = None, 0, []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while k < a.max_cycles:
            x, k = mg.cycle(b, x0=x)[0], k + 1
            r = mg.A.residual(b, x)
            hist.append(float(np.sqrt(r.dot(r))) / nb)
            if not hist[-1] > 1e-10 or not np.isfinite(hist[-1]):
                break
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        rate = (hist[-1] / hist[0]) ** (1.0 / (len(hist) - 1)) if len(hist) > 1 and hist[-1] > 0 else None
        return {"cycles": k, "converged": bool(hist[-1] <= 1e-10), "ms": ms, "ms_per_cycle": ms / k,
                "rel_residuals": hist[:3] + hist[-1:], "mean_reduction_per_cycle": rate}

    smoothers = {"default": {}}
    for dg in (4, 10):
        for ratio in (10.0, 30.0):
            smoothers[f"cheby_d{dg}_r{int(ratio)}"] = dict(smoother="chebyshev", cheby_degree=dg, cheby_ratio=ratio)

    u = lambda xx, yy: torch.sin(np.pi * xx) * torch.sin(np.pi * yy)
    f = lambda xx, yy: (2 * np.pi ** 2 + 1) * u(xx, yy)
    for pp in (1, 2, 3):
        for Nc in (8, 16):
            for name, cls in (("galerkin", GalerkinVCycle), ("matfree", MatrixFreeVCycle)):
                row = {}
                for sname, kw in smoothers.items():
                    nl = 2 if Nc == 8 else 3
                    mg = cls.uniform(pp, Nc, 4, 2, tol=0.0, maxiters=[4] * (nl - 1), dirichlet="all", **kw)
                    Vd, Td = mg.space, [mg.knots[0]] * 2
                    bc = DirichletBC(Vd, Td, "all")
                    bb = bc.homogenize(mg.A, assemble_rhs(Vd, Td, f), Vd.zeros())
                    solve(mg, bb)   # warm-up (first launches, allocations)
                    row[sname] = solve(mg, bb)
                    if kw:
                        row[sname]["lmax"] = mg.cheby_lmax
                res["cycles"][f"dirichlet_2d_p{pp}_{Nc}_{name}"] = row
                print(json.dumps({f"dirichlet_2d_p{pp}_{Nc}_{name}": {k: (v["cycles"], round(v["ms"], 3), v["converged"])
                                                                       for k, v in row.items()}}), flush=True)
    if not a.skip_big:
        for name, cls in (("matfree", MatrixFreeVCycle), ("galerkin", GalerkinVCycle)):
            row = {}
            for sname, kw in smoothers.items():
                t0 = time.perf_counter()
                mg = cls.uniform(p, a.cells3, 8, 3, a=a_coef, c=c_coef, tol=0.0, **kw)
                torch.cuda.synchronize()
                cons = (time.perf_counter() - t0) * 1e3
                if not kw:
                    mg.maxiters = [2] * (mg.nlevels - 1)
                row[sname] = dict(solve(mg, mg.rhs_ones()), construction_ms=cons)
                if kw:
                    row[sname]["lmax"] = mg.cheby_lmax
                print(json.dumps({f"varcoef_3d_p{p}_{a.cells3}_{name}_{sname}": row[sname]}), flush=True)
                del mg
                torch.cuda.empty_cache()
            res["cycles"][f"varcoef_3d_p{p}_{a.cells3}_{name}"] = row
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
