#!/usr/bin/env python3
"""One-slab proxy of the 8-GPU V-cycle on ONE GPU.

Rank r of the 8-rank bench owns 64-65 of the 515 axis-0 planes.  This runs the
same V-cycle schedule (pcg + damped Jacobi, residual, restriction, coarse solve,
prolongation, post pcg) on a single-GPU grid of (planes x 515 x 515) DOF: the
per-rank kernel work without the ghost exchange and all-reduces, i.e. a lower
bound on the 8-GPU cycle time.  Comparing the wall time per cycle with the sum of
kernel durations (rocprofv3 --kernel-trace --stats on this script) gives the
host-issue floor: the time the GPU waits for the Python host.

    python tools/slab_proxy.py --planes 67 --steps 3

``--loopback-rank R --world W`` runs rank R's slab of the W-rank split of the real
global problem instead (``SlabDistribution.loopback``): the production distributed
schedule -- interior planes, the p-plane exchange on the communication stream, the
boundary launch, the native pcg loop's all-reduces and lazy norms -- with every
exchange and sum going through a one-rank RCCL communicator (the slab sends its
boundary planes to itself).  RCCL's on-device copy stands in for the xGMI link.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def build(planes_cells: int, cells: int, p: int, coarse: int):
    import numpy as np
    from poms_amd.mg import TwoLevelVCycle, two_level_setup_1d
    from poms_amd.multilevels import KronTransfer
    from poms_amd.splines import assemble_1d, band_to_dense, uniform_knots
    from poms_amd.stencil import KronOperator, StencilVectorSpace

    cells3 = (planes_cells, cells, cells)
    Ms, Ks, Ps, Mcs, Kcs = [], [], [], [], []
    for N in cells3:
        T, _, P1 = two_level_setup_1d(p, uniform_knots(p, N), uniform_knots(p, coarse))
        M, K = assemble_1d(T, p)
        Ms.append(M), Ks.append(K), Ps.append(P1)
        Md, Kd = band_to_dense(M), band_to_dense(K)
        Mcs.append(P1.T @ Md @ P1), Kcs.append(P1.T @ Kd @ P1)
    npts = [m.shape[0] for m in Ms]
    mg = TwoLevelVCycle.__new__(TwoLevelVCycle)
    mg.p, mg.ndim, mg.glt, mg.tol, mg.maxiters, mg.post_smoother = p, 3, None, 1e-6, [10], "jacobi"
    V = StencilVectorSpace(npts, [p] * 3, align=True)
    mg.spaces, mg.ops, mg.transfers = [V], [KronOperator.laplace(V, Ms, Ks)], [KronTransfer(V, Ps)]
    mg.fused = [mg.transfer.set_operator(mg.A)]   # (fused where it applies, as TwoLevelVCycle's 3D default)
    kr = lambda a, b, c: np.kron(np.kron(a, b), c)
    Ac = kr(Mcs[0], Mcs[1], Mcs[2])
    for d in range(3):
        Ac = Ac + kr(*[Kcs[e] if e == d else Mcs[e] for e in range(3)])
    mg._set_coarse(Ac)
    return mg, npts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=67, help="axis-0 DOF planes (p + cells, nested in the coarse grid)")
    ap.add_argument("--cells", type=int, default=512)
    ap.add_argument("--p", type=int, default=3)
    ap.add_argument("--coarse", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--loopback-rank", type=int, default=None)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=0, help="axis-0 chunk of every operator launch (0: auto)")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    if a.loopback_rank is not None:
        from poms_amd.dist import SlabDistribution
        from poms_amd.mg import TwoLevelVCycle
        n = a.cells + a.p
        d = SlabDistribution.loopback(n, a.loopback_rank, a.world)
        mg = TwoLevelVCycle(a.p, a.cells, a.coarse, ndim=3, dist=d, chunk=a.chunk)
        npts = [d.n_local, n, n]
        label = (f"rank {a.loopback_rank} of {a.world}: {npts[0]}x{n}x{n} owned DOF of the {n}^3 problem, "
                 f"exchanges with {(d.prev is not None) + (d.next is not None)} neighbour side(s) "
                 f"looped back through a one-rank RCCL communicator ({d.transport})")
    else:
        mg, npts = build(a.planes - a.p, a.cells, a.p, a.coarse)
        if a.chunk:
            mg.A.set_chunk(a.chunk)
        label = f"{npts[0]}x{npts[1]}x{npts[2]} DOF (one slab of the 8-GPU bench, no halo)"
    bf = mg.rhs_ones()
    for _ in range(a.warmup):
        mg.cycle(bf)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        x, ipre, ipos = mg.cycle(bf)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    # a second, instrumented pass: the GPU time of every operator launch (the events
    # cost the host a few us each, so the wall time above is taken without them)
    mg.A.timing(True, reserve=400 * a.steps)
    for _ in range(a.steps):
        mg.cycle(bf)
    torch.cuda.synchronize()
    mg.A.timing(False)
    per = {}
    for kind in ("apply", "residual", "jacobi", "jacobi_from_zero", "apply_dot"):
        t, n, _ = mg.A.timing_read(kind)
        per[kind] = {"gpu_ms_per_cycle": t * 1e3 / a.steps, "launches_per_cycle": n / a.steps}
    print(json.dumps({"proxy": label,
                      "ms_per_cycle": dt * 1e3,
                      "operator_gpu_ms_per_cycle": sum(v["gpu_ms_per_cycle"] for v in per.values()),
                      "operator": per, "info_pre": ipre, "info_pos": ipos}), flush=True)


if __name__ == "__main__":
    main()
