#!/usr/bin/env python
"""Times of the device Galerkin product ``P^T A P`` of a general stencil
(``poms_op_galerkin_stencil``; not part of bench.py) against its two alternatives.

Per configuration (default 3D p = 3, 128^3 -> 64^3 cells and 2D p = 3, 1024^2 -> 512^2)
the median of ``--reps`` calls after a warm-up call, device events around the call and
the host clock (the call ends in a device synchronise; it allocates and frees its
scratch, which is part of both times):

* ``galerkin``        -- ``galerkin_stencil(A_f, P)``, A_f assembled on the device;
* ``assemble_coarse`` -- ``assemble_stencil`` on the coarse knots: rediscretising, the
  alternative where the coefficients are known on the coarse quadrature grid.

Next to the Galerkin time the model's bytes (every pass reads its input planes and writes
its output planes once) and their time at 8 TB/s.  At ``--cells-host`` (32^3, where scipy
finishes) the host route of the parent commit -- ``tosparse`` -> scipy ``P^T A P`` ->
``StencilMatrix.from_data`` -> first ``dot`` (the upload) -- against the device call, and
the largest difference of the two results.

    python tools/galerkin_bench.py [--out profiles/galerkin/galerkin_bench.json]
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
    return 1.0 + 0.5 * np.sin(3 * x) * np.cos(2 * y)


def c_coef(x, y, *z):
    return 2.0 + x * y


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, default=3)
    ap.add_argument("--cells3", type=int, default=128)
    ap.add_argument("--cells2", type=int, default=1024)
    ap.add_argument("--cells-host", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("galerkin_bench needs a GPU: times are not taken on a CPU")
    import scipy.sparse as sp
    from poms_amd.assembly import assemble_stencil
    from poms_amd.mg import two_level_setup_1d
    from poms_amd.multilevels import galerkin_stencil
    from poms_amd.splines import uniform_knots
    from poms_amd.stencil import StencilMatrix, StencilVectorSpace

    torch.cuda.set_device(0)
    p = a.p

    def timed(fn):
        ev, wall = [], []
        for i in range(1 + a.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            t1 = time.perf_counter()
            del out
            if i >= 1:
                ev.append(e0.elapsed_time(e1))
                wall.append((t1 - t0) * 1e3)
        return {"ms": statistics.median(ev), "min_ms": min(ev), "max_ms": max(ev), "wall_ms": statistics.median(wall)}

    def setup(ndim, cells):
        Tc = uniform_knots(p, cells // 2)
        T, _, P1 = two_level_setup_1d(p, uniform_knots(p, cells), Tc)
        Vf = StencilVectorSpace([cells + p] * ndim, [p] * ndim, align=True)
        Vc = StencilVectorSpace([cells // 2 + p] * ndim, [p] * ndim, align=True)
        return T, Tc, P1, Vf, Vc

    def model_bytes(ndim, nf, nc):
        W = (2 * p + 1) ** ndim
        ext, tot = [nf] * ndim, 0.0
        for d in range(ndim):
            rows_in = float(np.prod(ext))
            ext[d] = nc
            tot += 8.0 * W * (rows_in + float(np.prod(ext)))
        return tot

    res = {"device": torch.cuda.get_device_name(0), "p": p, "reps": a.reps, "configs": {}}
    for ndim, cells in ((3, a.cells3), (2, a.cells2)):
        T, Tc, P1, Vf, Vc = setup(ndim, cells)
        A = assemble_stencil(Vf, [T] * ndim, a=a_coef, c=c_coef)
        torch.cuda.synchronize()
        nb = model_bytes(ndim, cells + p, cells // 2 + p)
        fine_bytes = 8.0 * (2 * p + 1) ** ndim * (cells + p) ** ndim
        g = timed(lambda: galerkin_stencil(A, [P1] * ndim, coarse_space=Vc))
        g.update(model_bytes=nb, fine_coefficient_bytes=fine_bytes, t_8tbs_ms=nb / 8e12 * 1e3)
        g["fraction_of_8tbs"] = g["t_8tbs_ms"] / g["ms"]
        r = timed(lambda: assemble_stencil(Vc, [Tc] * ndim, a=a_coef, c=c_coef))
        res["configs"][f"{ndim}d_p{p}_{cells}"] = {
            "cells_fine": cells, "cells_coarse": cells // 2, "galerkin": g, "assemble_coarse": r,
            "galerkin_over_assemble": g["ms"] / r["ms"]}
        del A
    # the host route of the parent commit, where scipy finishes
    ndim, cells = 3, a.cells_host
    T, Tc, P1, Vf, Vc = setup(ndim, cells)
    A = assemble_stencil(Vf, [T] * ndim, a=a_coef, c=c_coef)
    nc1 = P1.shape[1]
    x = Vc.zeros().from_numpy(np.random.default_rng(0).uniform(-1, 1, (nc1,) * ndim))

    def host_route():
        Af = A.tosparse()
        Pm = sp.csr_matrix(P1)
        Pk = Pm
        for _ in range(ndim - 1):
            Pk = sp.kron(Pk, Pm, format="csr")
        Ac = (Pk.T @ Af @ Pk).tocoo()
        data = np.zeros(Vc.padded_shape + (2 * p + 1,) * ndim)
        ri = np.unravel_index(Ac.row, (nc1,) * ndim)
        ci = np.unravel_index(Ac.col, (nc1,) * ndim)
        data[tuple(r_ + p for r_ in ri) + tuple(c_ - r_ + p for r_, c_ in zip(ri, ci))] = Ac.data
        M = StencilMatrix.from_data(Vc, data)
        M.dot(x)
        torch.cuda.synchronize()
        return M

    def host_timed():
        ts = []
        for _ in range(3):
            A._host = None   # the download is part of the route
            t0 = time.perf_counter()
            M = host_route()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), M

    h_ms, Mh = host_timed()
    gd = timed(lambda: galerkin_stencil(A, [P1] * ndim, coarse_space=Vc))
    Md = galerkin_stencil(A, [P1] * ndim, coarse_space=Vc)
    diff = float(np.max(np.abs(Md._data - Mh._data)) / np.max(np.abs(Mh._data)))
    res["host_route"] = {"ndim": ndim, "cells_fine": cells, "cells_coarse": cells // 2, "host_wall_ms": h_ms,
                         "galerkin": gd, "host_over_device": h_ms / gd["wall_ms"], "maxrel_device_vs_host": diff}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
