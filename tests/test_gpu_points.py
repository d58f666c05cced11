"""Spline fields at scattered points on the device (csrc/spline_points.hip,
poms_amd/points.py): span search, evaluation with gradient, deposition (binned and atomic)
against a long-double reference kept here, and the ties to the tensor-grid code.

Reference, per point and per axis: ``find_span`` gives the span; a long-double copy of the
Cox-de Boor triangle gives the values; the first derivatives are
``p (N_{r-1,p-1} / Δ1 − N_{r,p-1} / Δ2)`` next to their absolute form ``p (|·| + |·|)``.
Tensor sums are formed in long double.

Tolerances (derived, not tuned), with ``u = 2^-53``:

* evaluation: ``(Σ_d (5 p_d + 3) + ndim + Π_d (p_d + 1)) u S``, ``S`` the same tensor sum of
  the absolute 1D rows (the absolute derivative form where ``der[d] = 1``) and ``|x|``:
  ``5 p + 3`` roundings bound one axis' triangle (two differences, a quotient, a product and
  a sum per level), ``ndim`` products, one add per term;
* deposition: ``(Σ_d (5 p_d + 3) + ndim + 1 + N_i) u S_i``, ``N_i`` the points in the
  support of ``i`` and ``S_i = Σ_k |w_k| B_i(x_k)``: it holds for any order of summation,
  so for the atomic form too.
"""
import functools

import numpy as np
import pytest

from poms_amd.splines import find_span, uniform_knots

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble


def _nonuniform_knots(p, cells, power=1.4):
    breaks = np.linspace(0.0, 1.0, cells + 1) ** power
    return np.concatenate([np.zeros(p), breaks, np.ones(p)])


def _breaks_knots(p, breaks):
    breaks = np.asarray(breaks, dtype=float)
    return np.concatenate([np.full(p, breaks[0]), breaks, np.full(p, breaks[-1])])


# p = 3, the interior knot 0.45 repeated: an empty span in the middle
T_REP = _breaks_knots(3, [0.0, 0.1, 0.2, 0.3, 0.45, 0.45, 0.6, 0.7, 0.85, 1.0])

CASES = {
    # name: (degrees, cells, knots, align)
    "1d_p2": ((2,), (150,), "uniform", False),
    "2d_p23": ((2, 3), (6, 5), "nonuniform", False),
    "3d_p3": ((3, 3, 3), (3, 2, 17), "uniform", False),
    "3d_p3_aligned": ((3, 3, 3), (3, 2, 17), "uniform", True),
    "3d_p5": ((5, 5, 5), (3, 3, 3), "uniform", False),
    "3d_p1": ((1, 1, 1), (4, 4, 4), "nonuniform", False),
    "1d_p3_rep": ((3,), None, "repeated", False),
}
RANDOM_N = (1, 63, 257, 5000)


# ---- the long-double reference ---------------------------------------------------------
def _host_cells(T, p, x):
    """Per point: span of find_span, its index among the non-empty spans, inside or not."""
    n = len(T) - p - 1
    spans = np.array([s for s in range(p, n) if T[s + 1] > T[s]])
    inside = (x >= T[p]) & (x <= T[n])            # NaN compares false
    xs = np.where(inside, x, T[p])
    span = np.array([find_span(T, p, float(v)) for v in xs], dtype=np.int64)
    el = np.searchsorted(spans, span)
    assert np.array_equal(spans[el], span)
    return span, el, inside, len(spans)


def _ld_rows(T, p, x, span):
    """Long-double triangle at the points ``x`` (N,) on ``span`` (N,): values (N, p+1), first
    derivatives and their absolute form."""
    Tl = np.asarray(T, dtype=LD)
    xl = np.asarray(x, dtype=LD)
    K = len(xl)
    N = np.zeros((K, p + 1), dtype=LD)
    N[:, 0] = 1
    prev = N.copy()
    left = np.zeros((K, p + 1), dtype=LD)
    right = np.zeros((K, p + 1), dtype=LD)
    for j in range(1, p + 1):
        prev = N.copy()                            # degree j - 1
        left[:, j] = xl - Tl[span + 1 - j]
        right[:, j] = Tl[span + j] - xl
        saved = np.zeros(K, dtype=LD)
        for r in range(j):
            tmp = N[:, r] / (right[:, r + 1] + left[:, j - r])
            N[:, r] = saved + right[:, r + 1] * tmp
            saved = left[:, j - r] * tmp
        N[:, j] = saved
    D = np.zeros((K, p + 1), dtype=LD)
    Da = np.zeros((K, p + 1), dtype=LD)
    for r in range(p + 1):
        a = prev[:, r - 1] / (Tl[span + r] - Tl[span + r - p]) if r >= 1 else 0
        b = prev[:, r] / (Tl[span + r + 1] - Tl[span + r + 1 - p]) if r < p else 0
        D[:, r] = p * (a - b)
        Da[:, r] = p * (np.abs(a) + np.abs(b))
    return N, D, Da


def _outer(rows):
    """(N, r0, r1, ...) products of the per-axis rows (N, r_d), in long double."""
    out = rows[0]
    for r in rows[1:]:
        out = out[..., None] * r.reshape((r.shape[0],) + (1,) * (out.ndim - 1) + (r.shape[1],))
    return out


def _index(firsts, ps):
    """Fancy index of the coefficient block (N, r0, r1, ...) of every point."""
    nd = len(ps)
    idx = []
    for d, (f, p) in enumerate(zip(firsts, ps)):
        i = f[:, None] + np.arange(p + 1)[None, :]
        idx.append(i.reshape((len(f),) + tuple(p + 1 if k == d else 1 for k in range(nd))))
    return tuple(idx)


def _within(got, ref, bound, what):
    """Elementwise |got - ref| <= bound; prints the largest err/bound."""
    bound = np.asarray(bound, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=LD) - ref).astype(np.float64)
    if err.size == 0:
        return True
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print(f"{what}: max err/bound = {float(ratio.max()):.3f} (max err {err.max():.3e})")
    return not (err > bound).any()


class PointSet:
    """Positions with their reference rows; points outside get weight 0 in every sum."""

    def __init__(self, c, pos):
        self.pos = np.ascontiguousarray(pos, dtype=np.float64)
        self.N = self.pos.shape[1]
        self._dep = {}
        self.inside = np.ones(self.N, dtype=bool)
        self.first, self.rows, self.drows, self.arows, els = [], [], [], [], []
        for d, (T, p) in enumerate(zip(c.knots, c.p)):
            span, el, ins, nel = _host_cells(T, p, self.pos[d])
            self.inside &= ins
            xs = np.where(ins, self.pos[d], T[p])
            Nv, Dv, Da = _ld_rows(T, p, xs, span)
            self.first.append(span - p)
            self.rows.append(Nv); self.drows.append(Dv); self.arows.append(Da)
            els.append((el, nel))
        cell = np.zeros(self.N, dtype=np.int64)
        for el, nel in els:
            cell = cell * nel + el
        self.cell = np.where(self.inside, cell, -1)
        self.idx = _index(self.first, c.p)
        self.dev = c.torch.from_numpy(self.pos).to(c.dev)

    def eval_ref(self, c, der):
        """(reference, S) of value (der None) or the derivative along axis ``der``."""
        rows = [self.drows[d] if d == der else self.rows[d] for d in range(c.nd)]
        arows = [self.arows[d] if d == der else np.abs(self.rows[d]) for d in range(c.nd)]
        blk = np.asarray(c.x, dtype=LD)[self.idx]
        ax = tuple(range(1, c.nd + 1))
        ref = (_outer(rows) * blk).sum(axis=ax)
        S = (_outer(arows) * np.abs(blk)).sum(axis=ax)
        m = self.inside
        return np.where(m, ref, 0), np.where(m, S, 0).astype(np.float64)

    def deposit_ref(self, c, w):
        """(reference b, S_i, N_i) of the weights ``w`` (N,); kept per weight array."""
        key = np.asarray(w, dtype=np.float64).tobytes()
        if key not in self._dep:
            self._dep[key] = self._deposit_ref(c, w)
        return self._dep[key]

    def _deposit_ref(self, c, w):
        wl = np.where(self.inside, np.asarray(w, dtype=LD), 0).reshape((self.N,) + (1,) * c.nd)
        B = _outer(self.rows)
        b = np.zeros(c.npts, dtype=LD); S = np.zeros(c.npts, dtype=LD); cnt = np.zeros(c.npts)
        np.add.at(b, self.idx, wl * B)
        np.add.at(S, self.idx, np.abs(wl) * np.abs(B))
        np.add.at(cnt, self.idx, np.broadcast_to(self.inside.reshape(wl.shape).astype(float), B.shape))
        return b, S.astype(np.float64), cnt


class Case:
    def __init__(self, name, scratch_bytes=None):
        import torch
        from poms_amd.points import SplinePoints
        from poms_amd.stencil import StencilVectorSpace
        self.name = name
        self.p, self.cells, kind, self.align = CASES[name]
        self.nd = len(self.p)
        if kind == "repeated":
            self.knots = [T_REP]
        else:
            self.knots = [uniform_knots(p, k) if kind == "uniform" else _nonuniform_knots(p, k)
                          for p, k in zip(self.p, self.cells)]
        self.npts = tuple(len(T) - p - 1 for T, p in zip(self.knots, self.p))
        self.torch, self.dev = torch, torch.device("cuda:0")
        self.V = StencilVectorSpace(self.npts, self.p, align=self.align)
        kw = {} if scratch_bytes is None else {"scratch_bytes": scratch_bytes}
        self.sp = SplinePoints(self.V, self.knots, **kw)
        self.rng = np.random.default_rng(sum(map(ord, name)))
        self.x = self.rng.uniform(-1, 1, self.npts)
        self.xv = self.V.zeros().from_numpy(self.x)
        self.lo = np.array([T[p] for T, p in zip(self.knots, self.p)])
        self.hi = np.array([T[-1] for T in self.knots])
        self.eval_factor = sum(5 * p + 3 for p in self.p) + self.nd + int(np.prod([p + 1 for p in self.p]))
        self.dep_factor = sum(5 * p + 3 for p in self.p) + self.nd + 1

    def breaks(self, d):
        return np.unique(self.knots[d])

    def _random_pos(self, N, rng):
        return self.lo[:, None] + (self.hi - self.lo)[:, None] * rng.uniform(0, 1, (self.nd, N))

    @functools.lru_cache(maxsize=None)
    def points(self, kind):
        rng = np.random.default_rng(self.nd * 1000 + (kind if isinstance(kind, int) else len(kind)))
        if isinstance(kind, int):
            pos = self._random_pos(kind, rng)
        elif kind == "breaks":
            # every breakpoint, its neighbours 1 ulp to both sides, both ends of the domain
            per = []
            for d in range(self.nd):
                b = self.breaks(d)
                per.append(np.concatenate([b, np.nextafter(b, -np.inf), np.nextafter(b, np.inf), b[[0, -1]]]))
            K = max(len(a) for a in per)
            pos = np.stack([np.resize(a, K) for a in per])
            # ... and each axis' special points again with the other axes at random inside
            blocks = [pos]
            for d in range(self.nd):
                blk = self._random_pos(len(per[d]), rng)
                blk[d] = per[d]
                blocks.append(blk)
            pos = np.concatenate(blocks, axis=1)
        elif kind == "onecell":
            # 3000 points in one cell: a chain longer than a workgroup, every other cell empty
            pos = np.empty((self.nd, 3000))
            for d in range(self.nd):
                b = self.breaks(d)
                e = (len(b) - 1) // 2
                pos[d] = b[e] + (b[e + 1] - b[e]) * rng.uniform(0, 1, 3000)
        elif kind == "outside":
            pos = self._random_pos(257, rng)
            pos[0, 3] = self.lo[0] - 1e-3
            pos[-1, 40] = self.hi[-1] + 0.5
            pos[0, 64] = np.nan
            pos[-1, 130] = np.inf
            pos[self.nd // 2, 256] = -1e300
        else:
            raise KeyError(kind)
        return PointSet(self, pos)

    def weights(self, ps):
        return np.random.default_rng(ps.N).uniform(-1, 1, ps.N)


@functools.lru_cache(maxsize=None)
def _case(name, scratch_bytes=None):
    return Case(name, scratch_bytes)


ALL_SETS = RANDOM_N + ("onecell", "outside")


# ---- 1. spans --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_cells_are_find_span(gpu, name):
    c = _case(name)
    assert c.sp.ncells == int(np.prod([len(c.breaks(d)) - 1 for d in range(c.nd)]))
    assert c.sp.uniform == tuple(CASES[name][2] == "uniform" for _ in range(c.nd))
    for kind in ALL_SETS + ("breaks",):
        ps = c.points(kind)
        got = c.sp.cells(ps.dev).cpu().numpy()
        assert got.dtype == np.int64 and got.shape == (ps.N,)
        assert np.array_equal(got, ps.cell), f"{name} {kind}: {np.flatnonzero(got != ps.cell)[:8]}"
        assert np.array_equal(got == -1, ~ps.inside)
    out = c.points("outside")
    assert (~out.inside).sum() == 5
    assert (~c.points("breaks").inside).any() and c.points("breaks").inside.any()


# ---- 2. evaluation ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_evaluate_against_reference(gpu, name):
    c = _case(name)
    for kind in ALL_SETS + ("breaks",):
        ps = c.points(kind)
        val, grad = c.sp.evaluate_grad(c.xv, ps.dev)
        assert tuple(val.shape) == (ps.N,) and tuple(grad.shape) == (c.nd, ps.N)
        for der in (None,) + tuple(range(c.nd)):
            dt = None if der is None else tuple(int(k == der) for k in range(c.nd))
            got = c.sp.evaluate(c.xv, ps.dev, der=dt)
            ref, S = ps.eval_ref(c, der)
            assert _within(got.cpu().numpy(), ref, c.eval_factor * U * S, f"{name} {kind} der {der}")
            # the one-pass gradient is the separate calls bitwise
            assert c.torch.equal(got, val if der is None else grad[der])
            assert not got.cpu().numpy()[~ps.inside].any()


# ---- 3. the tensor-grid code -------------------------------------------------------------
def _irregular_points(rng, k):
    inner = rng.uniform(0.0, 1.0, k - 3)
    return np.sort(np.concatenate([[0.0, 1.0], inner, inner[:1]]))


@pytest.mark.parametrize("name", ["2d_p23", "3d_p3", "3d_p3_aligned"])
def test_evaluate_agrees_with_point_grid(gpu, name):
    from poms_amd.field import PointGrid, evaluate_at
    c = _case(name)
    rng = np.random.default_rng(5)
    pts = [_irregular_points(rng, k) for k in (7, 11, 9)[:c.nd]]
    g = PointGrid(c.V, c.knots, pts)
    pos = np.stack([m.reshape(-1) for m in np.meshgrid(*pts, indexing="ij")])
    ps = PointSet(c, pos)
    L = max(c.p) + 1
    for der in (None,) + tuple(range(c.nd)):
        dt = None if der is None else tuple(int(k == der) for k in range(c.nd))
        got = c.sp.evaluate(c.xv, ps.dev, der=dt).cpu().numpy()
        grid = g.evaluate(c.xv, der=dt).cpu().numpy().reshape(-1)
        _ref, S = ps.eval_ref(c, der)
        assert _within(got, grid.astype(LD), (c.eval_factor + 3 * L + 6) * U * S, f"{name} grid der {der}")
    assert c.torch.equal(evaluate_at(c.V, c.knots, c.xv, ps.dev), c.sp.evaluate(c.xv, ps.dev))


# ---- 4. deposition -------------------------------------------------------------------------
def _outside_interior(V, vec):
    s = vec._store.clone()
    V.interior(V.view(s)).zero_()
    return s


@pytest.mark.parametrize("method", ["binned", "atomic"])
@pytest.mark.parametrize("name", list(CASES))
def test_deposit_against_reference(gpu, name, method):
    c = _case(name)
    t = c.torch
    for kind in ALL_SETS:
        ps = c.points(kind)
        w = c.weights(ps)
        wd = t.from_numpy(w).to(c.dev)
        ref, S, cnt = ps.deposit_ref(c, w)
        bound = (c.dep_factor + cnt) * U * S
        b = c.sp.deposit(ps.dev, wd, method=method)
        got = b.to_local_numpy()
        assert _within(got, ref, bound, f"{name} {kind} {method}")
        assert not got[cnt == 0].any()                      # where no point reaches: exactly 0
        assert not _outside_interior(c.V, b).any()          # ghosts, dead pitch columns
        # into a vector that holds something else: overwritten without accumulate ...
        out = c.V.zeros().from_numpy(np.full(c.npts, 7.0))
        assert c.sp.deposit(ps.dev, wd, out=out, method=method) is out
        assert _within(out.to_local_numpy(), ref, bound, f"{name} {kind} {method} overwrite")
        # ... and unit weights when w is None
        ref1, S1, _ = ps.deposit_ref(c, np.ones(ps.N))
        assert _within(c.sp.deposit(ps.dev, method=method).to_local_numpy(), ref1, (c.dep_factor + cnt) * U * S1,
                       f"{name} {kind} {method} unit weights")


@pytest.mark.parametrize("method", ["binned", "atomic"])
def test_deposit_accumulates_and_leaves_ghosts(gpu, method):
    """Aligned layout, ``out`` pre-filled with a sentinel everywhere (ghost cells and dead
    pitch columns included): the interior gains the deposit, the rest keeps its bits.  The
    sum into 7 rounds once more per add at magnitude 7 + S_i."""
    c = _case("3d_p3_aligned")
    t = c.torch
    ps = c.points(5000)
    w = c.weights(ps)
    ref, S, cnt = ps.deposit_ref(c, w)
    out = c.V.zeros()
    out._store.fill_(7.0)
    before = _outside_interior(c.V, out)
    c.sp.deposit(ps.dev, t.from_numpy(w).to(c.dev), out=out, accumulate=True, method=method)
    assert t.equal(_outside_interior(c.V, out), before)
    bound = (c.dep_factor + cnt) * U * S + (cnt + 1) * U * (7.0 + S)
    assert _within(out.to_local_numpy(), ref + 7, bound, f"accumulate {method}")


@pytest.mark.parametrize("method", ["binned", "atomic"])
def test_points_outside_change_nothing(gpu, method):
    c = _case("3d_p3")
    t = c.torch
    pos = t.tensor([[-0.5, 2.0, float("nan"), 0.5], [0.5, 0.5, 0.5, float("inf")], [0.5, 0.5, 0.5, 0.5]],
                   dtype=t.float64, device=c.dev)
    assert not c.sp.deposit(pos, method=method)._store.any()
    out = c.V.zeros().from_numpy(c.x)
    keep = out._store.clone()
    c.sp.deposit(pos, out=out, accumulate=True, method=method)
    assert t.equal(out._store, keep)
    assert not c.sp.evaluate(c.xv, pos).any() and (c.sp.cells(pos) == -1).all()


# ---- 5. reproducibility of the binned form ---------------------------------------------------
@pytest.mark.parametrize("name", ["3d_p3", "3d_p5", "2d_p23"])
def test_binned_deposit_is_reproducible(gpu, name):
    c = _case(name)
    t = c.torch
    for kind in (5000, "onecell", "outside"):
        ps = c.points(kind)
        wd = t.from_numpy(c.weights(ps)).to(c.dev)
        b = c.sp.deposit(ps.dev, wd)
        assert t.equal(c.sp.deposit(ps.dev, wd)._store, b._store)
        binning = c.sp.bin(ps.dev)
        assert int(binning.n_inside.item()) == int(ps.inside.sum())
        assert t.equal(t.sort(binning.perm).values, t.arange(ps.N, device=c.dev))
        assert t.equal(c.sp.deposit(ps.dev, wd, binning=binning)._store, b._store)
        assert t.equal(c.sp.deposit(ps.dev, wd, binning=binning)._store, b._store)   # the binning is reusable


@pytest.mark.parametrize("name,per_e0,slabs", [("3d_p3", 2 * 17 * 64 * 8, 3), ("3d_p3_aligned", 2 * 17 * 64 * 8, 3),
                                               ("2d_p23", 5 * 12 * 8, 6), ("1d_p2", 2 * 3 * 8, 75)])
def test_chunked_binned_deposit(gpu, name, per_e0, slabs):
    """Scratch for one axis-0 layer of cells: three slabs on the (3, 2, 17) grid (two layers
    in 1D).  The slabs change the association of the sum, so the result is within the
    deposit's bound of the unchunked one, not bitwise."""
    c = _case(name)
    ck = _case(name, per_e0)
    assert len(ck.sp._slabs()) == slabs and len(c.sp._slabs()) == 1
    t = c.torch
    for kind in (5000, "onecell"):
        ps = c.points(kind)
        w = c.weights(ps)
        wd = t.from_numpy(w).to(c.dev)
        ref, S, cnt = ps.deposit_ref(c, w)
        bound = (c.dep_factor + cnt) * U * S
        one = c.sp.deposit(ps.dev, wd).to_local_numpy()
        b = ck.sp.deposit(ps.dev, wd)
        assert _within(b.to_local_numpy(), ref, bound, f"chunked {kind} vs reference")
        assert _within(b.to_local_numpy(), one.astype(LD), bound, f"chunked {kind} vs unchunked")
        assert t.equal(ck.sp.deposit(ps.dev, wd)._store, b._store)
        assert not _outside_interior(ck.V, b).any()


# ---- 6. adjointness ----------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["binned", "atomic"])
@pytest.mark.parametrize("name", list(CASES))
def test_deposit_is_the_adjoint_of_evaluate(gpu, name, method):
    c = _case(name)
    t = c.torch
    ps = c.points(5000)
    w = c.weights(ps)
    _, Sd, cnt = ps.deposit_ref(c, w)
    _, Se = ps.eval_ref(c, None)
    b = c.sp.deposit(ps.dev, t.from_numpy(w).to(c.dev), method=method).to_local_numpy()
    v = c.sp.evaluate(c.xv, ps.dev).cpu().numpy()
    lhs = (b.astype(LD) * c.x.astype(LD)).sum()
    rhs = (w.astype(LD) * v.astype(LD)).sum()
    tol = float((((c.dep_factor + cnt) * U * Sd) * np.abs(c.x)).sum() + (np.abs(w) * c.eval_factor * U * Se).sum())
    print(f"{name} {method}: |<b, x> - <w, u>| / tol = {float(abs(lhs - rhs)) / tol:.3f}")
    assert abs(lhs - rhs) <= tol


# ---- 7. the load vector ------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["binned", "atomic"])
@pytest.mark.parametrize("name", ["2d_p23", "3d_p3", "3d_p3_aligned"])
def test_deposit_of_quadrature_points_is_the_load_vector(gpu, name, method):
    from poms_amd.field import QuadGrid, deposit
    c = _case(name)
    t = c.torch
    g = QuadGrid(c.V, c.knots)
    f = np.random.default_rng(3).uniform(-1, 1, g.shape)
    W = functools.reduce(np.multiply.outer, g.weights)
    pos = np.stack([m.reshape(-1) for m in np.meshgrid(*g.points, indexing="ij")])
    ps = PointSet(c, pos)
    w = (W * f).reshape(-1)
    wd = t.from_numpy(w).to(c.dev)
    ref, S, cnt = ps.deposit_ref(c, w)
    L = max((p + 1) * (p + 1) for p in c.p)        # QuadGrid: p + 1 points per span
    load = g.load_vector(f).to_local_numpy()
    got = c.sp.deposit(ps.dev, wd, method=method).to_local_numpy()
    assert _within(got, load.astype(LD), (c.dep_factor + cnt + 3 * L + 6) * U * S, f"{name} {method} vs load_vector")
    assert _within(got, ref, (c.dep_factor + cnt) * U * S, f"{name} {method} vs reference")
    if method == "binned":
        assert t.equal(deposit(c.V, c.knots, ps.dev, wd)._store, c.sp.deposit(ps.dev, wd)._store)


# ---- 8. arguments ------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_launch(gpu):
    c = _case("3d_p3")
    t, sp = c.torch, c.sp
    good = c.points(63).dev
    bad = (ValueError, TypeError)
    for pos in (good[:2], good.reshape(-1), good.reshape(3, 3, 21), good.float(), good.cpu(), good.cpu().numpy()):
        with pytest.raises(bad):
            sp.cells(pos)
        with pytest.raises(bad):
            sp.evaluate(c.xv, pos)
        with pytest.raises(bad):
            sp.evaluate_grad(c.xv, pos)
        with pytest.raises(bad):
            sp.deposit(pos)
        with pytest.raises(bad):
            sp.bin(pos)
    with pytest.raises(TypeError):
        sp.evaluate(_case("3d_p5").xv, good)
    with pytest.raises(TypeError):
        sp.deposit(good, out=_case("3d_p5").xv)
    with pytest.raises(ValueError, match="der"):
        sp.evaluate(c.xv, good, der=(2, 0, 0))
    with pytest.raises(ValueError, match="der"):
        sp.evaluate(c.xv, good, der=(0, 0))
    with pytest.raises(ValueError, match="method"):
        sp.deposit(good, method="sorted")
    with pytest.raises(ValueError, match="binning"):
        sp.deposit(good, binning=sp.bin(c.points(257).dev))
    with pytest.raises(ValueError, match="w must"):
        sp.deposit(good, t.ones(62, dtype=t.float64, device=c.dev))
    with pytest.raises(ValueError, match="out"):
        sp.evaluate(c.xv, good, out=t.empty(64, dtype=t.float64, device=c.dev))
    # a non-contiguous view of the right shape is accepted
    wide = t.zeros(3, 126, dtype=t.float64, device=c.dev)
    wide[:, ::2] = good
    assert t.equal(sp.cells(wide[:, ::2]), sp.cells(good))
    # 1D: a flat tensor of positions
    c1 = _case("1d_p2")
    p1 = c1.points(63).dev
    assert t.equal(c1.sp.evaluate(c1.xv, p1.reshape(-1)), c1.sp.evaluate(c1.xv, p1))


def test_no_points(gpu):
    c = _case("3d_p3")
    t, sp = c.torch, c.sp
    pos = t.empty(3, 0, dtype=t.float64, device=c.dev)
    assert sp.cells(pos).shape == (0,) and sp.cells(pos).dtype == t.int64
    assert sp.evaluate(c.xv, pos).shape == (0,)
    val, grad = sp.evaluate_grad(c.xv, pos)
    assert val.shape == (0,) and grad.shape == (3, 0)
    binning = sp.bin(pos)
    assert binning.perm.numel() == 0 and not binning.cell_start.any() and int(binning.n_inside.item()) == 0
    for method in ("binned", "atomic"):
        assert not sp.deposit(pos, method=method)._store.any()
        out = c.V.zeros().from_numpy(c.x)
        keep = out._store.clone()
        sp.deposit(pos, out=out, accumulate=True, method=method)
        assert t.equal(out._store, keep)
        sp.deposit(pos, out=out, method=method)
        assert not out._store.any()


def test_knots_and_scratch_are_checked(gpu):
    from poms_amd import _lib
    from poms_amd.points import SplinePoints
    c = _case("3d_p3")
    with pytest.raises(ValueError):
        SplinePoints(c.V, c.knots[:2])
    with pytest.raises(ValueError):
        SplinePoints(c.V, [c.knots[0], c.knots[1], c.knots[2][:-1]])
    T = c.knots[2].copy()
    T[6], T[7] = T[7], T[6]
    with pytest.raises(_lib.PomsError, match="non-decreasing"):
        SplinePoints(c.V, [c.knots[0], c.knots[1], T])
    T = c.knots[2].copy()
    T[0] = -0.1
    with pytest.raises(_lib.PomsError, match="open"):
        SplinePoints(c.V, [c.knots[0], c.knots[1], T])
    with pytest.raises(_lib.PomsError, match="scratch"):
        SplinePoints(c.V, c.knots, scratch_bytes=2 * 17 * 64 * 8 - 8)


def test_distributed_space_is_not_implemented(gpu):
    from poms_amd.dist import SlabDistribution
    from poms_amd.points import SplinePoints
    from poms_amd.stencil import StencilVectorSpace
    T = uniform_knots(2, 6)
    V = StencilVectorSpace([8, 8, 8], [2, 2, 2], dist=SlabDistribution(8, 0, 2))
    with pytest.raises(NotImplementedError, match="undistributed"):
        SplinePoints(V, [T] * 3)


# ---- 9. capture --------------------------------------------------------------------------------
def test_first_calls_under_capture(gpu):
    """poms_points_eval and poms_points_deposit_binned (binning prebuilt by another handle)
    are the first calls of a fresh handle, inside a graph capture: they allocate nothing.
    Replays equal the eager results bitwise, also after the inputs changed."""
    import torch
    from poms_amd.points import SplinePoints
    c = _case("3d_p3_aligned")
    ps, ps2 = c.points(5000), c.points("onecell")
    pos = ps.dev.clone()
    pos2 = torch.cat([ps2.dev, ps.dev[:, :2000]], dim=1).contiguous()
    wd = torch.from_numpy(c.weights(ps)).to(c.dev)
    want_v, want_g = (a.clone() for a in c.sp.evaluate_grad(c.xv, pos))
    want_b = c.sp.deposit(pos, wd)._store.clone()
    want_v2 = c.sp.evaluate_grad(c.xv, pos2)[0].clone()
    want_b2 = c.sp.deposit(pos2, wd)._store.clone()
    assert not torch.equal(want_b, want_b2)
    binning = c.sp.bin(pos)
    perm, cell_start = binning.perm.clone(), binning.cell_start.clone()

    fresh = SplinePoints(c.V, c.knots)
    out = torch.full((4, ps.N), float("nan"), dtype=torch.float64, device=c.dev)
    b = c.V.zeros()
    b._store.fill_(float("nan"))
    c.V.interior(b._data).zero_()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        fresh.evaluate_grad(c.xv, pos, out=out)
        fresh.deposit(pos, wd, out=b, binning=type(binning)(perm, cell_start, binning.n_inside))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], want_v) and torch.equal(out[1:], want_g)
    assert torch.equal(c.V.interior(b._data), c.V.interior(c.V.view(want_b)))
    pos.copy_(pos2)
    nb = c.sp.bin(pos)
    perm.copy_(nb.perm)
    cell_start.copy_(nb.cell_start)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], want_v2)
    assert torch.equal(c.V.interior(b._data), c.V.interior(c.V.view(want_b2)))
