#!/usr/bin/env python
"""The cost of the Robin face terms in the general kernels (csrc/stencil_general.hip,
csrc/matfree.hip; not part of bench.py): apply and Jacobi sweep of the matrix-free and the
stored-stencil operator, without face terms and with a Robin term on every face, in one
process.

Per configuration (tools/matfree_bench.py's: 3D p = 3, 128^3 cells = 131^3 functions, and 2D
p = 3, 1024^2 cells = 1027^2 functions) the operators (two forms, each without face terms and
with all faces) take turns call by call, device events around each call, a warm-up, the
median of ``--reps`` (>= 7), the L2 / MALL flushed before every timed call by filling a
512 MiB buffer.  A second face-free operator of each form runs in the same rotation: its
distance from the first is the run-to-run spread the other times are to be read against.
The stored stencil holds the face terms in its coefficients, so its two variants run the
same kernel on different numbers; the matrix-free operator runs its FACE builds.

    python tools/robin_bench.py [--out profiles/robin/robin_bench.json]
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


def a_coef(x, y, *z):
    return (1.0 + 0.5 * np.sin(3 * x) * np.cos(2 * y)) * (1.0 + z[0] / 4 if z else 1.0)


def c_coef(x, y, *z):
    return 2.0 + x * y


def beta(*X):
    return 1.0 + 0.5 * X[0] + 0.25 * X[-1] * X[0]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, default=3)
    ap.add_argument("--cells3", type=int, default=128)
    ap.add_argument("--cells2", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--flush-mib", type=int, default=512)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("robin_bench needs a GPU: times are not taken on a CPU")
    from poms_amd.assembly import assemble_stencil
    from poms_amd.matfree import MatrixFreeOperator
    from poms_amd.splines import uniform_knots
    from poms_amd.stencil import StencilVectorSpace

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

    res = {"device": torch.cuda.get_device_name(0), "p": p, "reps": a.reps, "flush_mib": a.flush_mib, "configs": {}}
    for ndim, cells in ((3, a.cells3), (2, a.cells2)):
        T = uniform_knots(p, cells)
        V = StencilVectorSpace([cells + p] * ndim, [p] * ndim, align=True)
        robin = {(d, s): beta for d in range(ndim) for s in (0, 1)}
        ops = {}
        for form, make in (("matfree", lambda **kw: MatrixFreeOperator(V, [T] * ndim, a=a_coef, c=c_coef, **kw)),
                           ("stencil", lambda **kw: assemble_stencil(V, [T] * ndim, a=a_coef, c=c_coef, **kw))):
            ops[f"{form}_free"] = make()
            ops[f"{form}_free_again"] = make()
            ops[f"{form}_all_faces"] = make(robin=robin)
            assert ops[f"{form}_free"].face_terms() == () and len(ops[f"{form}_all_faces"].face_terms()) == 2 * ndim
        rng = np.random.default_rng(0)
        x = V.zeros().from_numpy(rng.uniform(-1, 1, V.npts))
        b = V.zeros().from_numpy(rng.uniform(-1, 1, V.npts))
        y = V.zeros()
        times = {}
        for kind, call in (("dot", lambda A: A.dot(x, out=y)),
                           ("jacobi_sweep", lambda A: A.jacobi_sweep(b, x, y, 2.0 / 3.0, want_norm=True, lazy=True))):
            t = interleaved({k: (lambda A=A: call(A)) for k, A in ops.items()})
            for form in ("matfree", "stencil"):
                free, again, rob = (t[f"{form}_{k}"]["ms"] for k in ("free", "free_again", "all_faces"))
                t[f"{form}_robin_over_free"] = rob / free
                t[f"{form}_spread_ms"] = abs(again - free)
                t[f"{form}_extra_ms"] = rob - free
            times[kind] = t
        cfg = {"cells": cells, "ndof": V.dimension, "times": times}
        res["configs"][f"{ndim}d_p{p}_{cells}"] = cfg
        print(json.dumps({f"{ndim}d_p{p}_{cells}": cfg}), flush=True)
        del ops, x, b, y
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
