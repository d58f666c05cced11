#!/usr/bin/env python
"""Times of the spline-field calls at a size a user would run (not part of bench.py).

Default: 3D, p = 3, 128 cells per axis -- 131^3 coefficients, a 512^3-point quadrature
grid, 1.07 GB per array of point values.  Prints one JSON line with the median time of
``QuadGrid.evaluate``, ``load_vector`` and ``l2_error`` (device events; the L2 / MALL are
flushed before every repetition by filling a 512 MiB buffer, as ``bench.py --full`` does),
and next to each:

* ``t_8tbs_ms``     -- the algorithmic bytes (the large array once, the coefficients once)
  at 8 TB/s;
* ``copy_ms``       -- a ``torch`` copy of one array of the large array's size, same run
  (it reads and writes the array: twice the bytes of the write- or read-bound floor);
* ``dense_ms``      -- what a user would write today: three dense ``torch`` contractions
  with the (Q x n) collocation matrices.

    python tools/field_bench.py [--cells 128] [--p 3] [--reps 7] [--out profiles/...json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=128)
    ap.add_argument("--p", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--flush-mib", type=int, default=512)
    ap.add_argument("--chunk-mib", type=int, default=256)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("field_bench needs a GPU: times are not taken on a CPU")
    from poms_amd.field import QuadGrid
    from poms_amd.splines import uniform_knots
    from poms_amd.stencil import StencilVectorSpace

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    p, N = a.p, a.cells
    T = uniform_knots(p, N)
    n = N + p
    V = StencilVectorSpace([n] * 3, [p] * 3)
    g = QuadGrid(V, [T] * 3, chunk_bytes=a.chunk_mib << 20)
    Q = g.shape[0]
    rng = np.random.default_rng(0)
    x = V.zeros().from_numpy(rng.uniform(-1, 1, (n,) * 3))
    gen = torch.Generator(device=dev).manual_seed(1)
    f = torch.rand(g.shape, dtype=torch.float64, device=dev, generator=gen) * 2 - 1
    out = torch.empty(g.shape, dtype=torch.float64, device=dev)
    b = V.zeros()
    flush = torch.empty(a.flush_mib << 17, dtype=torch.float64, device=dev) if a.flush_mib else None

    def timed(fn):
        ts = []
        for i in range(a.warmup + a.reps):
            if flush is not None:
                flush.fill_(float(i))        # evict the operands from L2 / MALL (not timed)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), min(ts), max(ts)

    # the dense formulation: (Q x n) collocation matrices, one contraction per axis
    Cm = np.zeros((Q, n))
    from poms_amd.assembly import quad_point_tables
    tab = quad_point_tables(T, p)
    for q in range(Q):
        Cm[q, tab["first"][q]:tab["first"][q] + p + 1] = tab["basis"][q, :, 0]
    Cd = torch.from_numpy(Cm).to(dev)
    Wd = torch.from_numpy(tab["weights"]).to(dev)
    CWt = (Cd * Wd[:, None]).t().contiguous()
    xi = V.interior(x._data).contiguous()

    def dense_eval():
        t = torch.tensordot(Cd, xi, dims=([1], [0]))                      # (Q, n, n)
        t = torch.tensordot(t, Cd, dims=([1], [1]))                       # (Q, n, Q): axis 1 last
        return torch.tensordot(t.transpose(1, 2), Cd, dims=([2], [1]))    # (Q, Q, Q)

    def dense_load():
        t = torch.tensordot(f, CWt, dims=([2], [1]))                      # (Q, Q, n)
        t = torch.tensordot(CWt, t, dims=([1], [1]))                      # (n, Q, n)
        return torch.tensordot(CWt, t, dims=([1], [1]))                   # (n, n, n)

    def dense_error():
        d = dense_eval() - f
        return (Wd[:, None, None] * Wd[None, :, None] * Wd[None, None, :] * d * d).sum()

    big = 8.0 * Q ** 3
    small = 8.0 * n ** 3
    res = {"config": {"ndim": 3, "p": p, "cells": N, "n": n, "points_per_axis": Q, "large_array_gb": big / 1e9,
                      "chunk_q0": g.chunk_q0, "flush_mib": a.flush_mib, "reps": a.reps},
           "device": torch.cuda.get_device_name(0)}
    copy_dst = torch.empty_like(out)
    res["copy_ms"] = timed(lambda: copy_dst.copy_(f))[0]
    del copy_dst
    calls = {
        "evaluate": (lambda: g.evaluate(x, out=out), dense_eval, big + small),
        "load_vector": (lambda: g.load_vector(f, out=b), dense_load, big + small),
        "l2_error": (lambda: g.sq_error(x, f), dense_error, big + small),
    }
    for name, (fn, dense, nbytes) in calls.items():
        med, lo, hi = timed(fn)
        dmed = timed(dense)[0]
        t8 = nbytes / 8e12 * 1e3
        res[name] = {"ms": med, "min_ms": lo, "max_ms": hi, "algorithmic_bytes": nbytes, "t_8tbs_ms": t8,
                     "fraction_of_8tbs": t8 / med, "copy_ms": res["copy_ms"], "ratio_to_copy": med / res["copy_ms"],
                     "dense_ms": dmed, "ratio_to_dense": med / dmed}
    # the dense and the sum-factorised results agree (same data, same run)
    ev = g.evaluate(x, out=out)
    res["check"] = {"evaluate_vs_dense_max": float((ev - dense_eval()).abs().max().item()),
                    "load_vs_dense_max": float((V.interior(g.load_vector(f, out=b)._data) - dense_load()).abs().max().item())}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
