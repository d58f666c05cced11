#!/usr/bin/env python
"""The matrix-free operator (``MatrixFreeOperator``, csrc/matfree.hip; not part of
bench.py) against the stored stencil of the same coefficients, in one process.

Per configuration (default 3D p = 3, 128^3 cells and 2D p = 3, 1024^2 cells):

* ``dot``, ``jacobi_sweep`` (with its norm) and ``dot_inner`` of both operators,
  interleaved call by call, device events around each call, a warm-up, the median of
  ``--reps`` (>= 7), and the L2 / MALL flushed before every timed call by filling a
  512 MiB buffer (as tools/field_bench.py does);
* the device bytes each operator holds: the model and the drop of free device memory
  over its construction;
* the set-up wall time of ``MatrixFreeOperator(...)`` and ``assemble_stencil(...)``;
* one cycle of ``MatrixFreeVCycle`` and of ``GalerkinVCycle`` (2 pcg iterations per
  smoothing) and each one's construction time;
* next to the matrix-free ``dot`` the model's flops and bytes per DOF and the fractions
  of the FP64 vector peak (78.6 TF) and of 8 TB/s they amount to.

With ``--cells-big`` (default 256, 0 to skip) the matrix-free cycle alone at that 3D
size, its coefficients built as device tensors: cycle time, bytes held and the
residual reduction over three cycles.

    python tools/matfree_bench.py [--out profiles/matfree/matfree_bench.json]

``--tensor`` measures the tensor-coefficient operators instead, at the same
shapes and with the same protocol, and writes ``profiles/tensor/tensor_bench.json``:

* ``dot``, ``jacobi_sweep`` and ``dot_inner`` of the tensor ``MatrixFreeOperator`` and of
  the stored tensor stencil, interleaved; the wall time of the assembly and of the
  matrix-free set-up (tables and the diagonal kernel); the coefficients are built on the
  device (``G = M M^T + I``);
* the tensor ``dot`` against the scalar ``dot`` of this tree, next to the model's ratio
  of stage C's work per point, (9 fma, ncomp + 1 loads) against (3 mul, 2 loads);
* with ``--parent-lib PATH`` (a ``libpoms_hip.so`` built from the parent commit; the
  package itself cannot load it through ``POMS_HIP_LIB``, it lacks the new entry points)
  the scalar ``dot`` of this tree's library against the parent's, both called through
  ``poms_op_apply`` on handles created from the same tables and arrays, taking turns
  with a second handle of the parent's library, whose distance from the first is the
  parent's own run-to-run spread.

    python tools/matfree_bench.py --tensor [--parent-lib PATH] [--out profiles/tensor/tensor_bench.json]
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

PEAK_FP64 = 78.6e12
PEAK_HBM = 8e12


def a_coef(x, y, *z):
    return (1.0 + 0.5 * np.sin(3 * x) * np.cos(2 * y)) * (1.0 + z[0] / 4 if z else 1.0)


def c_coef(x, y, *z):
    return 2.0 + x * y


def model(ndim, p, nq, tile=8):
    """Flops and HBM bytes per DOF of one matrix-free apply as built: per
    quadrature plane of a tile the fmas of stages A-F, the 2D case through a trivial
    axis 0; bytes: x with the tile halo, a_q and c_q once, y."""
    w, Q = tile + 2 * p, (tile + p) * nq
    p0, nq0 = (p, nq) if ndim == 3 else (0, 1)
    fma = (2 * (p0 + 1) * w * w + 3 * (p + 1) * Q * w + 4 * (p + 1) * Q * Q + 4 * Q * Q      # A, B, C (+ scaling)
           + 4 * nq * (p + 1) * tile * Q + 3 * nq * (p + 1) * tile * tile + 2 * (p0 + 1) * tile * tile)   # D, E, F
    per_dof = 2.0 * fma * nq0 / (tile * tile)
    byt = 8.0 * (2 * nq ** ndim + (w / tile) ** 2 + 1)
    return per_dof, byt


def m_coef(i, j, X):
    """M_ij of the tensor mode's G = M M^T + I: smooth and distinct (torch, on the device)."""
    arg = (i + 1.0) * X[0] + (2.0 * j + 1.0) * X[1] + ((i + j + 1.5) * X[2] if len(X) == 3 else 0.0)
    return (0.3 + 0.1 * i + 0.05 * j) * torch.sin(arg + 0.5 * i - 0.3 * j)


def tensor_model(ndim, p, nq, tile=8):
    """The scalar model with stage C's scaling (4 Q^2 products per plane: w c u and
    three w a d_i) replaced by the tensor's (w c u, and per flux 3 multiply-adds and the
    product with w), and ncomp + 1 coefficient arrays instead of 2."""
    flops, byt = model(ndim, p, nq, tile)
    Q = (tile + p) * nq
    nq0 = nq if ndim == 3 else 1
    ncomp = ndim * (ndim + 1) // 2
    flops += 2.0 * (3 * 3 * Q * Q) * nq0 / (tile * tile)
    byt += 8.0 * (ncomp - 1) * nq ** ndim
    return flops, byt


class RawMatfree:
    """A scalar matrix-free operator made and applied through the C entry points of a
    given library (``poms_ctx_create``, ``poms_op_create_matfree``, ``poms_op_apply``):
    the same calls whichever build the library is."""

    def __init__(self, lib, V, knots, aq, cq):
        from poms_amd import _lib
        from poms_amd.assembly import axis_tables
        for name in ("poms_ctx_create", "poms_ctx_destroy", "poms_op_create_matfree", "poms_op_apply",
                     "poms_op_destroy"):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = _lib._SIGS[name], C.c_int
        lib.poms_last_error.restype = C.c_char_p
        self.lib, self.V, self.keep = lib, V, [aq, cq]
        nd = V.ndim
        lead = 3 - nd
        tabs = [axis_tables(np.asarray(T, float), V.pads[d]) for d, T in enumerate(knots)]

        def arr3(key, dtype):
            out = (C.c_void_p * 3)()
            for k, t in enumerate(tabs):
                a_ = np.ascontiguousarray(t[key], dtype=dtype)
                self.keep.append(a_)
                out[lead + k] = a_.ctypes.data
            return out

        ints = lambda key: (C.c_int * 3)(*([0] * lead + [int(t[key]) for t in tabs]))
        self.ctx, self.h = C.c_void_p(), C.c_void_p()
        self._ok(lib.poms_ctx_create(V.device, C.byref(self.ctx)))
        self._ok(lib.poms_op_create_matfree(
            self.ctx, nd, C.byref(V.layout), ints("nel"), ints("nq"), ints("p"), arr3("first", np.int32),
            arr3("es", np.int32), arr3("ee", np.int32), arr3("basis", np.float64), arr3("weights", np.float64),
            (C.c_int64 * 3)(*([1] * lead + [int(t["n"]) for t in tabs])), C.c_void_p(aq.data_ptr()),
            C.c_void_p(cq.data_ptr()), 1.0, C.byref(self.h)))
        self.n0 = int(V.npts[0]) if nd == 3 else 1

    def _ok(self, status):
        if status != 0:
            raise RuntimeError(self.lib.poms_last_error().decode(errors="replace"))

    def dot(self, x, y):
        from poms_amd import runtime as rt
        self._ok(self.lib.poms_op_apply(self.h, rt.ptr(x._data), rt.ptr(y._data), 0, self.n0, rt.stream_handle()))

    def close(self):
        self.lib.poms_op_destroy(self.h)
        self.lib.poms_ctx_destroy(self.ctx)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, default=3)
    ap.add_argument("--cells3", type=int, default=128)
    ap.add_argument("--cells2", type=int, default=1024)
    ap.add_argument("--cells-big", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--flush-mib", type=int, default=512)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--probe-dots", type=int, default=0,
                    help="only build the 3D matrix-free operator and call dot this many times (for rocprofv3 runs)")
    ap.add_argument("--tensor", action="store_true", help="measure the tensor-coefficient operators (DESIGN 3.15)")
    ap.add_argument("--parent-lib", type=str, default=None,
                    help="--tensor: a libpoms_hip.so of the parent commit for the scalar dot comparison")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("matfree_bench needs a GPU: times are not taken on a CPU")
    from poms_amd.assembly import assemble_stencil, axis_tables
    from poms_amd.matfree import MatrixFreeOperator, MatrixFreeVCycle
    from poms_amd.mg import GalerkinVCycle, two_level_setup_1d
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

    def built(fn):
        """(object, wall ms, drop of free device memory in bytes)."""
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        t0 = time.perf_counter()
        obj = fn()
        torch.cuda.synchronize()
        return obj, (time.perf_counter() - t0) * 1e3, free0 - torch.cuda.mem_get_info()[0]

    def cycles(mg, n):
        mg.maxiters = [2] * (mg.nlevels - 1)
        b = mg.rhs_ones()
        x, res, ts = None, [], []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x, _ = mg.cycle(b, x0=x)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            r = mg.A.residual(b, x)
            res.append(float(np.sqrt(r.dot(r))))
        return {"cycle_ms": ts, "residuals": res}

    if a.probe_dots:
        V = StencilVectorSpace([a.cells3 + p] * 3, [p] * 3, align=True)
        A = MatrixFreeOperator(V, [uniform_knots(p, a.cells3)] * 3, a=a_coef, c=c_coef)
        x, y = V.zeros().from_numpy(np.random.default_rng(0).uniform(-1, 1, V.npts)), V.zeros()
        for _ in range(a.probe_dots):
            A.dot(x, out=y)
        torch.cuda.synchronize()
        return 0
    res = {"device": torch.cuda.get_device_name(0), "p": p, "reps": a.reps, "flush_mib": a.flush_mib, "configs": {}}
    if a.tensor:
        from poms_amd import _lib
        parent = C.CDLL(a.parent_lib) if a.parent_lib else None
        res["parent_lib"] = bool(parent)
        for ndim, cells in ((3, a.cells3), (2, a.cells2)):
            T = uniform_knots(p, cells)
            V = StencilVectorSpace([cells + p] * ndim, [p] * ndim, align=True)
            ndof = V.dimension
            pts = torch.from_numpy(axis_tables(T, p)["points"].reshape(-1)).to(dev)
            X = [pts.reshape([-1 if k == d else 1 for k in range(ndim)]) for d in range(ndim)]
            M = [[m_coef(i, j, X) for j in range(ndim)] for i in range(ndim)]
            G = torch.stack([torch.broadcast_to(sum(M[i][k] * M[j][k] for k in range(ndim)) + float(i == j),
                                                (pts.numel(),) * ndim)
                             for i in range(ndim) for j in range(i, ndim)]).contiguous()
            aq = torch.broadcast_to((1.0 + 0.5 * torch.sin(3 * X[0]) * torch.cos(2 * X[1]))
                                    * (1.0 + X[2] / 4 if ndim == 3 else 1.0), (pts.numel(),) * ndim).contiguous()
            cq = torch.broadcast_to(2.0 + X[0] * X[1], (pts.numel(),) * ndim).contiguous()
            del M
            Amf, mf_ms, mf_held = built(lambda: MatrixFreeOperator(V, [T] * ndim, a=G, c=cq))
            Ast, st_ms, st_held = built(lambda: assemble_stencil(V, [T] * ndim, a=G, c=cq))
            Asc, sc_ms, _ = built(lambda: MatrixFreeOperator(V, [T] * ndim, a=aq, c=cq))
            rng = np.random.default_rng(0)
            x = V.zeros().from_numpy(rng.uniform(-1, 1, V.npts))
            b = V.zeros().from_numpy(rng.uniform(-1, 1, V.npts))
            y = V.zeros()
            ref = Ast.dot(x)._data
            diff = float((Amf.dot(x)._data - ref).abs().max() / ref.abs().max())
            del ref
            times = {}
            for kind, call in (("dot", lambda A: A.dot(x, out=y)),
                               ("jacobi_sweep", lambda A: A.jacobi_sweep(b, x, y, 2.0 / 3.0, want_norm=True, lazy=True)),
                               ("dot_inner", lambda A: A.dot_inner(x, y, device=True))):
                fns = {"matfree_tensor": lambda: call(Amf), "stencil_tensor": lambda: call(Ast)}
                if kind == "dot":
                    fns["matfree_scalar"] = lambda: call(Asc)
                t = interleaved(fns)
                t["matfree_over_stencil"] = t["matfree_tensor"]["ms"] / t["stencil_tensor"]["ms"]
                times[kind] = t
            fl_s, by_s = model(ndim, p, p + 1)
            fl_t, by_t = tensor_model(ndim, p, p + 1)
            ncomp = ndim * (ndim + 1) // 2
            W = (2 * p + 1) ** ndim
            cfg = {"cells": cells, "ndof": ndof, "maxrel_matfree_vs_stencil": diff, "times": times,
                   "setup_ms": {"matfree_tensor_with_diagonal": mf_ms, "assemble_stencil_tensor": st_ms,
                                "matfree_scalar_with_diagonal": sc_ms},
                   "bytes_held": {"matfree_model": Amf.device_bytes(), "matfree_measured": mf_held,
                                  "stencil_model": 8 * W * ndof, "stencil_measured": st_held,
                                  "model_ratio": Amf.device_bytes() / (8.0 * W * ndof)},
                   "tensor_over_scalar_dot": {
                       "measured": times["dot"]["matfree_tensor"]["ms"] / times["dot"]["matfree_scalar"]["ms"],
                       "stage_c_per_point": {"tensor": f"9 multiply-adds and 3 products with w, {ncomp + 1} loads",
                                             "scalar": "w a and 3 products, 2 loads"},
                       "model_flops_ratio": fl_t / fl_s, "model_bytes_ratio": by_t / by_s}}
            if parent is not None:
                mine = RawMatfree(_lib.lib, V, [T] * ndim, aq, cq)
                par_a = RawMatfree(parent, V, [T] * ndim, aq, cq)
                par_b = RawMatfree(parent, V, [T] * ndim, aq, cq)
                y2 = V.zeros()
                mine.dot(x, y)
                par_a.dot(x, y2)
                same = bool(torch.equal(y._data, y2._data))
                t = interleaved({"parent_a": lambda: par_a.dot(x, y), "this_tree": lambda: mine.dot(x, y),
                                 "parent_b": lambda: par_b.dot(x, y)})
                lo = min(t["parent_a"]["min_ms"], t["parent_b"]["min_ms"])
                hi = max(t["parent_a"]["max_ms"], t["parent_b"]["max_ms"])
                t["bitwise_equal_to_parent"] = same
                t["this_tree_median_within_parent_min_max"] = bool(lo <= t["this_tree"]["ms"] <= hi)
                cfg["scalar_dot_vs_parent"] = t
                for o in (mine, par_a, par_b):
                    o.close()
            res["configs"][f"{ndim}d_p{p}_{cells}"] = cfg
            print(json.dumps({f"{ndim}d_p{p}_{cells}": cfg}), flush=True)
            del Amf, Ast, Asc, G, aq, cq, x, b, y
        out = a.out or "profiles/tensor/tensor_bench.json"
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(json.dumps(res) + "\n")
        return 0
    for ndim, cells in ((3, a.cells3), (2, a.cells2)):
        T = uniform_knots(p, cells)
        V = StencilVectorSpace([cells + p] * ndim, [p] * ndim, align=True)
        ndof = V.dimension
        Amf, mf_ms, mf_held = built(lambda: MatrixFreeOperator(V, [T] * ndim, a=a_coef, c=c_coef))
        Ast, st_ms, st_held = built(lambda: assemble_stencil(V, [T] * ndim, a=a_coef, c=c_coef))
        rng = np.random.default_rng(0)
        x = V.zeros().from_numpy(rng.uniform(-1, 1, V.npts))
        b = V.zeros().from_numpy(rng.uniform(-1, 1, V.npts))
        y = V.zeros()
        diff = float((Amf.dot(x)._data - Ast.dot(x)._data).abs().max() / Ast.dot(x)._data.abs().max())
        times = {}
        for kind, call in (("dot", lambda A: A.dot(x, out=y)),
                           ("jacobi_sweep", lambda A: A.jacobi_sweep(b, x, y, 2.0 / 3.0, want_norm=True, lazy=True)),
                           ("dot_inner", lambda A: A.dot_inner(x, y, device=True))):
            t = interleaved({"matfree": lambda: call(Amf), "stencil": lambda: call(Ast)})
            t["matfree_over_stencil"] = t["matfree"]["ms"] / t["stencil"]["ms"]
            times[kind] = t
        flops, byt = model(ndim, p, p + 1)
        t_dot = times["dot"]["matfree"]["ms"] * 1e-3
        W = (2 * p + 1) ** ndim
        cfg = {"cells": cells, "ndof": ndof, "maxrel_matfree_vs_stencil": diff, "times": times,
               "setup_ms": {"matfree": mf_ms, "assemble_stencil": st_ms},
               "bytes_held": {"matfree_model": Amf.device_bytes(), "matfree_measured": mf_held,
                              "stencil_model": 8 * W * ndof, "stencil_measured": st_held,
                              "model_ratio": Amf.device_bytes() / (8.0 * W * ndof)},
               "model": {"flops_per_dof": flops, "bytes_per_dof": byt,
                         "fraction_of_fp64_vector_peak": flops * ndof / t_dot / PEAK_FP64,
                         "fraction_of_8tbs": byt * ndof / t_dot / PEAK_HBM,
                         "stencil_fraction_of_8tbs": (8.0 * W + 16) * ndof / (times["dot"]["stencil"]["ms"] * 1e-3) / PEAK_HBM}}
        del Amf, Ast, x, b, y
        coarsest = 8 if ndim == 3 else 16
        mgm, cm, _ = built(lambda: MatrixFreeVCycle.uniform(p, cells, coarsest, ndim, a=a_coef, c=c_coef, tol=0.0))
        rm = cycles(mgm, 3)
        del mgm
        mgg, cg, _ = built(lambda: GalerkinVCycle.uniform(p, cells, coarsest, ndim, a=a_coef, c=c_coef, tol=0.0))
        rg = cycles(mgg, 3)
        del mgg
        cfg["vcycle"] = {"matfree": dict(rm, construction_ms=cm), "galerkin": dict(rg, construction_ms=cg)}
        res["configs"][f"{ndim}d_p{p}_{cells}"] = cfg
        print(json.dumps({f"{ndim}d_p{p}_{cells}": cfg}), flush=True)
    if a.cells_big:
        ndim, cells = 3, a.cells_big
        cells_all = [cells]
        while cells_all[-1] // 2 >= 8 and cells_all[-1] % 2 == 0:
            cells_all.append(cells_all[-1] // 2)
        knots = [uniform_knots(p, N) for N in cells_all]
        P1 = [two_level_setup_1d(p, knots[l], knots[l + 1])[2] for l in range(len(cells_all) - 1)]
        V = StencilVectorSpace([cells + p] * ndim, [p] * ndim, align=True)

        def big():
            pts = torch.from_numpy(axis_tables(knots[0], p)["points"].reshape(-1)).to(dev)
            X, Y, Z = pts[:, None, None], pts[None, :, None], pts[None, None, :]
            aq = ((1.0 + 0.5 * torch.sin(3 * X) * torch.cos(2 * Y)) * (1.0 + Z / 4)).contiguous()
            cq = (2.0 + X * Y + 0.0 * Z).contiguous()
            A = MatrixFreeOperator(V, [knots[0]] * ndim, a=aq, c=cq)
            V1 = StencilVectorSpace([cells // 2 + p] * ndim, [p] * ndim, align=True)
            A1 = assemble_stencil(V1, [knots[1]] * ndim, a=a_coef, c=c_coef)
            return MatrixFreeVCycle(A, [[P1l] * ndim for P1l in P1], A1, tol=0.0)

        mg, cons, held = built(big)
        r = cycles(mg, 3)
        res["big"] = dict(r, cells=cells, ndof=V.dimension, construction_ms=cons, bytes_held_all_levels=held,
                          fine_operator_bytes=mg.A.device_bytes(),
                          stored_stencil_would_need=8 * (2 * p + 1) ** ndim * V.dimension)
        print(json.dumps({"big": res["big"]}), flush=True)
    line = json.dumps(res)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
