#!/usr/bin/env python
"""The block vector kernels and LOBPCG on one MI355X (not part of bench.py).

One process, 3D, p = 3, 128^3 cells by default:

1. ``block_gram`` of 12 x 12 vectors (symmetric) against the 78 ``poms_vec_dot`` calls it
   replaces, and ``block_combine`` (12 -> 8) against the chain of one ``poms_vec_scale`` and
   eleven ``poms_vec_axpby`` per output: the two sides take turns rep by rep after a warm-up,
   device events around each, the L2 / MALL flushed before every timed call by filling a
   buffer (``--flush-mib 0``: not flushed), medians of ``--reps``.  Bytes per second come from
   the byte model of DESIGN §3.20 (vector passes issued by the kernels, not HBM traffic).
2. One ``lobpcg(k=4)`` for ``-Δ + 1`` against the mass matrix, preconditioned by
   ``GalerkinVCycle.uniform(..., smoother="chebyshev").preconditioner()``: iterations, wall
   time per iteration, and -- from a second run with a device synchronise around every
   preconditioner call, operator apply and block operation -- its split into preconditioner,
   applies, block operations (``block_gram``, ``block_combine``) and the rest (the copies to
   the host, the small eigenproblem, Python).

    python tools/eigen_bench.py [--out profiles/eigen/eigen_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch


class Timed:
    """An operator whose ``dot`` is bracketed by device synchronises and timed."""

    def __init__(self, op, acc, key):
        self.op, self.space, self.acc, self.key = op, op.space, acc, key

    def dot(self, x, out=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = self.op.dot(x, out=out)
        torch.cuda.synchronize()
        self.acc[self.key] += time.perf_counter() - t0
        return y


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, default=3)
    ap.add_argument("--cells", type=int, default=128)
    ap.add_argument("--n", type=int, default=12, help="vectors of the Gram matrix and inputs of the combine")
    ap.add_argument("--nout", type=int, default=8)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--maxiter", type=int, default=60)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--flush-mib", type=int, default=512)
    ap.add_argument("--skip-lobpcg", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("eigen_bench needs a GPU: times are not taken on a CPU")
    from poms_amd import _lib, runtime as rt
    from poms_amd.eigen import block_combine, block_gram, lobpcg
    from poms_amd.mg import GalerkinVCycle
    from poms_amd.splines import assemble_1d, uniform_knots
    from poms_amd.stencil import KronOperator, StencilVectorSpace

    torch.cuda.set_device(0)
    dev = "cuda:0"
    p, N, n, nout = a.p, a.cells, a.n, a.nout
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

    res = {"device": torch.cuda.get_device_name(0), "p": p, "cells": N, "reps": a.reps, "flush_mib": a.flush_mib}

    # ---- 1. the fused kernels against the entry points they replace -----------------------
    V = StencilVectorSpace([N + p] * 3, [p] * 3, align=True)
    lay, st = C.byref(V.layout), rt.stream_handle()
    rng = np.random.default_rng(0)
    xs = [V.zeros().from_numpy(rng.standard_normal(V.npts)) for _ in range(n)]
    outs = [V.empty() for _ in range(nout)]
    outs2 = [V.empty() for _ in range(nout)]
    Cm = rng.standard_normal((n, nout))
    Cd = torch.from_numpy(Cm).to(dev)
    G = torch.empty((n, n), dtype=torch.float64, device=dev)
    Gd = torch.zeros((n, n), dtype=torch.float64, device=dev)
    vec_bytes = 8.0 * (V.local_npts[0] * V.plane_elems)   # one pass over a vector's flat range

    def dots():
        for i in range(n):
            for j in range(i, n):
                _lib.call("poms_vec_dot", V.ctx, lay, rt.ptr(xs[i]._data), rt.ptr(xs[j]._data), rt.ptr(Gd[i, j:]), st)

    def chain():
        for j, o in enumerate(outs2):
            _lib.call("poms_vec_scale", V.ctx, lay, float(Cm[0, j]), rt.ptr(xs[0]._data), rt.ptr(o._data), st)
            for i in range(1, n):
                _lib.call("poms_vec_axpby", V.ctx, lay, float(Cm[i, j]), rt.ptr(xs[i]._data), 1.0, rt.ptr(o._data),
                          rt.ptr(o._data), st)

    t = interleaved({"block_gram": lambda: block_gram(xs, xs, symmetric=True, out=G),
                     "vec_dots": dots,
                     "block_combine": lambda: block_combine(xs, Cd, outs),
                     "axpby_chain": chain})
    T = 4
    tiles = (n // T) * (n // T + 1) // 2 if n % T == 0 else None
    model = {"vector_bytes": vec_bytes,
             "gram_vector_reads": None if tiles is None else tiles * 2 * T, "dots_vector_reads": n * (n + 1),
             "combine_vector_passes": n + nout, "chain_vector_passes": nout * (2 + 3 * (n - 1))}
    for key, passes in (("block_gram", model["gram_vector_reads"]), ("vec_dots", model["dots_vector_reads"]),
                        ("block_combine", model["combine_vector_passes"]), ("axpby_chain", model["chain_vector_passes"])):
        if passes is not None:
            t[key]["model_TB_per_s"] = passes * vec_bytes / (t[key]["ms"] * 1e-3) / 1e12
    t["gram_speedup"] = t["vec_dots"]["ms"] / t["block_gram"]["ms"]
    t["combine_speedup"] = t["axpby_chain"]["ms"] / t["block_combine"]["ms"]
    # the two sides computed the same thing
    iu = np.triu_indices(n)
    g, gd = G.cpu().numpy(), Gd.cpu().numpy()
    t["gram_max_rel_diff"] = float(np.max(np.abs(g[iu] - gd[iu]) / np.sqrt(np.outer(np.diag(g), np.diag(g)))[iu]))
    t["combine_max_abs_diff"] = float(max((V.interior(o._data) - V.interior(o2._data)).abs().max().item()
                                          for o, o2 in zip(outs, outs2)))
    res["kernels"] = dict(t, n=n, nout=nout, ndof=V.dimension, model=model)
    print(json.dumps({"kernels": res["kernels"]}), flush=True)
    del xs, outs, outs2

    # ---- 2. one lobpcg ---------------------------------------------------------------------
    if not a.skip_lobpcg:
        t0 = time.perf_counter()
        vc = GalerkinVCycle.uniform(p, N, 8, 3, smoother="chebyshev")
        torch.cuda.synchronize()
        cons = time.perf_counter() - t0
        A, Vv = vc.A, vc.space
        M = assemble_1d(uniform_knots(p, N), p)[0]
        B = KronOperator.product(Vv, [M] * 3)
        pre = vc.preconditioner()
        kw = dict(k=a.k, tol=a.tol, maxiter=a.maxiter, seed=0)
        lobpcg(A, B, precond=pre, **dict(kw, maxiter=2))   # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lam, X, info = lobpcg(A, B, precond=pre, **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        acc = {"precond": 0.0, "apply_A": 0.0, "apply_B": 0.0, "block_gram": 0.0, "block_combine": 0.0}

        def bracketed(fn, key):
            def run(*args, **kwargs):
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                out = fn(*args, **kwargs)
                torch.cuda.synchronize()
                acc[key] += time.perf_counter() - t1
                return out
            return run

        timed_pre = bracketed(pre, "precond")
        # the solver's block operations, bracketed the same way for this run only
        from poms_amd import eigen
        plain = eigen.block_gram, eigen.block_combine
        eigen.block_gram = bracketed(plain[0], "block_gram")
        eigen.block_combine = bracketed(plain[1], "block_combine")
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lam2, _, info2 = lobpcg(Timed(A, acc, "apply_A"), Timed(B, acc, "apply_B"), precond=timed_pre, **kw)
            torch.cuda.synchronize()
            wall2 = time.perf_counter() - t0
        finally:
            eigen.block_gram, eigen.block_combine = plain
        it = max(info["niter"], 1)
        it2 = max(info2["niter"], 1)
        res["lobpcg"] = {"construction_s": cons, "k": a.k, "tol": a.tol, "niter": info["niter"],
                         "converged": [bool(c) for c in info["converged"]], "restarts": info["restarts"],
                         "lam": [float(v) for v in lam], "res": [float(v) for v in info["res"]],
                         "wall_s": wall, "ms_per_iteration": wall / it * 1e3,
                         "timed_run": {"niter": info2["niter"], "wall_s": wall2, "same_lam": bool(np.array_equal(lam, lam2)),
                                       "ms_per_iteration": wall2 / it2 * 1e3,
                                       "precond_ms_per_iteration": acc["precond"] / it2 * 1e3,
                                       "applies_ms_per_iteration": (acc["apply_A"] + acc["apply_B"]) / it2 * 1e3,
                                       "block_gram_ms_per_iteration": acc["block_gram"] / it2 * 1e3,
                                       "block_combine_ms_per_iteration": acc["block_combine"] / it2 * 1e3,
                                       "rest_ms_per_iteration": (wall2 - sum(acc.values())) / it2 * 1e3}}
        print(json.dumps({"lobpcg": res["lobpcg"]}), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
