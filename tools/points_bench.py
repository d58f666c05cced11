#!/usr/bin/env python
"""Times of the scattered-point calls at a size a particle code would run (not part of
bench.py).

Default: 3D, p = 3, 64 cells per axis (67^3 coefficients), N = 2^22 points.  Prints one
JSON line with the median time of ``SplinePoints.evaluate``, ``evaluate_grad``, ``deposit``
binned (the binning timed on its own and included) and ``deposit`` atomic, on two point
sets: (a) uniform random points, (b) the same points pre-sorted by cell.  Device events;
the L2 / MALL are flushed before every repetition by filling a 512 MiB buffer.  Next to
each time:

* ``t_8tbs_ms``  -- the algorithmic bytes at 8 TB/s: ``8 (ndim + 1) N`` for evaluate (and
  for deposit: positions and weights), plus ``8 ndim N`` for the gradient, plus the
  coefficient array once;
* ``torch_ms``   -- a formulation in torch ops only, with the per-point 1D basis rows and
  first indices precomputed (their time is NOT counted: the baseline is spared the basis
  evaluation): evaluate gathers the (p+1)^3 neighbours and contracts them with ``einsum``,
  deposit is ``index_put_(accumulate=True)`` of the outer products;
* for the atomic deposit the estimate of its atomic traffic: ``8 (p+1)^3 N`` bytes at the
  chip-wide float-atomic rate of 1.3 TB/s (full 256-B wave instructions; one lane per row
  was measured an order of magnitude slower).

    python tools/points_bench.py [--cells 64] [--p 3] [--log2n 22] [--out profiles/points/points_bench.json]
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
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--p", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--flush-mib", type=int, default=512)
    ap.add_argument("--torch-chunk", type=int, default=1 << 19, help="points per step of the torch formulation")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("points_bench needs a GPU: times are not taken on a CPU")
    from poms_amd.points import SplinePoints
    from poms_amd.splines import basis_funs_ders, uniform_knots
    from poms_amd.stencil import StencilVectorSpace

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    p, nc, N = a.p, a.cells, 1 << a.log2n
    r = p + 1
    T = uniform_knots(p, nc)
    n = nc + p
    V = StencilVectorSpace([n] * 3, [p] * 3)
    sp = SplinePoints(V, [T] * 3)
    rng = np.random.default_rng(0)
    x = V.zeros().from_numpy(rng.uniform(-1, 1, (n,) * 3))
    gen = torch.Generator(device=dev).manual_seed(1)
    pos_a = torch.rand((3, N), dtype=torch.float64, device=dev, generator=gen)
    w = torch.rand(N, dtype=torch.float64, device=dev, generator=gen) * 2 - 1
    order = torch.sort(sp.cells(pos_a), stable=True).indices
    pos_b = pos_a[:, order].contiguous()
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

    # the torch formulation's precomputed tables (not timed): first indices (3, N) and the
    # value rows (3, N, r), the triangle of basis_funs_ders vectorised over the points
    def tables(pos):
        e = torch.clamp((pos * nc).to(torch.int64), 0, nc - 1)
        first = e                                            # span - p = e on open uniform knots
        rows = torch.empty((3, N, r), dtype=torch.float64, device=dev)
        ph = pos.cpu().numpy()
        eh = e.cpu().numpy()
        for d in range(3):
            rows[d] = torch.from_numpy(_rows(T, p, ph[d], eh[d] + p)).to(dev)
        return first, rows

    def _rows(T, p, xs, span):
        K = len(xs)
        Nv = np.zeros((K, p + 1))
        Nv[:, 0] = 1.0
        left = np.zeros((K, p + 1))
        right = np.zeros((K, p + 1))
        for j in range(1, p + 1):
            left[:, j] = xs - T[span + 1 - j]
            right[:, j] = T[span + j] - xs
            saved = np.zeros(K)
            for q in range(j):
                tmp = Nv[:, q] / (right[:, q + 1] + left[:, j - q])
                Nv[:, q] = saved + right[:, q + 1] * tmp
                saved = left[:, j - q] * tmp
            Nv[:, j] = saved
        return Nv

    k0 = 12345
    chk = basis_funs_ders(T, p, float(pos_a[0, k0].item()), int(min(int(pos_a[0, k0].item() * nc), nc - 1)) + p, 0)[0]
    xi = V.interior(x._data).contiguous().reshape(-1)
    ar = torch.arange(r, device=dev)
    step = a.torch_chunk

    def torch_eval(first, rows, out):
        for b in range(0, N, step):
            s = slice(b, min(b + step, N))
            i0 = (first[0, s, None] + ar)[:, :, None, None]
            i1 = (first[1, s, None] + ar)[:, None, :, None]
            i2 = (first[2, s, None] + ar)[:, None, None, :]
            blk = xi[(i0 * n + i1) * n + i2]
            out[s] = torch.einsum("kabc,ka,kb,kc->k", blk, rows[0, s], rows[1, s], rows[2, s])
        return out

    def torch_deposit(first, rows, bflat):
        bflat.zero_()
        for b in range(0, N, step):
            s = slice(b, min(b + step, N))
            i0 = (first[0, s, None] + ar)[:, :, None, None]
            i1 = (first[1, s, None] + ar)[:, None, :, None]
            i2 = (first[2, s, None] + ar)[:, None, None, :]
            vals = torch.einsum("k,ka,kb,kc->kabc", w[s], rows[0, s], rows[1, s], rows[2, s])
            bflat.index_put_((((i0 * n + i1) * n + i2).reshape(-1),), vals.reshape(-1), accumulate=True)
        return bflat

    small = 8.0 * n ** 3
    ev_bytes = 8.0 * 4 * N + small
    gr_bytes = ev_bytes + 8.0 * 3 * N
    atomic_bytes = 8.0 * r ** 3 * N
    res = {"config": {"ndim": 3, "p": p, "cells": nc, "n": n, "N": N, "flush_mib": a.flush_mib, "reps": a.reps,
                      "uniform_axes": list(sp.uniform), "slabs": len(sp._slabs())},
           "device": torch.cuda.get_device_name(0),
           "atomic_estimate": {"atomic_bytes": atomic_bytes, "ms_at_1p3_tbs": atomic_bytes / 1.3e12 * 1e3}}
    out1 = torch.empty(N, dtype=torch.float64, device=dev)
    out4 = torch.empty((4, N), dtype=torch.float64, device=dev)
    tout = torch.empty(N, dtype=torch.float64, device=dev)
    b = V.zeros()
    bflat = torch.zeros(n ** 3, dtype=torch.float64, device=dev)

    def entry(med, lo, hi, nbytes, tmed=None):
        t8 = nbytes / 8e12 * 1e3
        e = {"ms": med, "min_ms": lo, "max_ms": hi, "algorithmic_bytes": nbytes, "t_8tbs_ms": t8,
             "fraction_of_8tbs": t8 / med}
        if tmed is not None:
            e.update(torch_ms=tmed, ratio_to_torch=med / tmed)
        return e

    for label, pos in (("random", pos_a), ("sorted", pos_b)):
        first, rows = tables(pos)
        if label == "random":
            res["check_rows_vs_host"] = float(np.abs(rows[0, k0].cpu().numpy() - chk).max())
        t_ev = timed(lambda: torch_eval(first, rows, tout))[0]
        t_dep = timed(lambda: torch_deposit(first, rows, bflat))[0]
        r_ = {}
        r_["evaluate"] = entry(*timed(lambda: sp.evaluate(x, pos, out=out1)), ev_bytes, t_ev)
        r_["evaluate_grad"] = entry(*timed(lambda: sp.evaluate_grad(x, pos, out=out4)), gr_bytes, t_ev)
        r_["bin"] = entry(*timed(lambda: sp.bin(pos)), 8.0 * 3 * N)
        binning = sp.bin(pos)
        r_["deposit_binned_prebinned"] = entry(*timed(lambda: sp.deposit(pos, w, out=b, binning=binning)), ev_bytes,
                                               t_dep)
        r_["deposit_binned"] = entry(*timed(lambda: sp.deposit(pos, w, out=b)), ev_bytes, t_dep)
        r_["deposit_atomic"] = entry(*timed(lambda: sp.deposit(pos, w, out=b, method="atomic")), ev_bytes, t_dep)
        r_["deposit_atomic"]["ratio_to_atomic_estimate"] = (r_["deposit_atomic"]["ms"]
                                                            / res["atomic_estimate"]["ms_at_1p3_tbs"])
        r_["binned_over_atomic"] = r_["deposit_binned"]["ms"] / r_["deposit_atomic"]["ms"]
        # the torch and the HIP results agree (same data, same run)
        ev = sp.evaluate(x, pos, out=out1)
        scale = float(ev.abs().max().item())
        dep = V.interior(sp.deposit(pos, w, out=b)._data).reshape(-1)
        r_["check"] = {"evaluate_vs_torch_max": float((ev - torch_eval(first, rows, tout)).abs().max().item()) / scale,
                       "deposit_vs_torch_max": float((dep - torch_deposit(first, rows, bflat)).abs().max().item())
                       / float(dep.abs().max().item())}
        res[label] = r_
        del first, rows
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
