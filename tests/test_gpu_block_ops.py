"""The block vector kernels on the device (csrc/block_ops.hip): the Gram matrix of two lists of
vectors and linear combinations of a list, against NumPy on the interiors, with their
reproducibility, storage invariants and refusals.

Spaces: a flat range shorter than one block (2D 5 x 6), one with odd pitches (2D 9 x 12) and
one of several blocks (3D 6 x 9 x 17), each unaligned (pitches that put the vectors on both
16-B phases: the 8-B path or a leading single element) and aligned (16-B accesses).  List
sizes: one tile, whole tiles, a ragged tile edge, and the maximum."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52

SPACES = {
    "2d_5x6_p11": ((5, 6), (1, 1)),
    "2d_9x12_p23": ((9, 12), (2, 3)),
    "3d_6x9x17_p123": ((6, 9, 17), (1, 2, 3)),
}
GRAM_SIZES = [(1, 1), (4, 4), (5, 7), (12, 12), (24, 24)]
COMBINE_SIZES = [(1, 1), (3, 2), (12, 8), (24, 16)]


@functools.lru_cache(maxsize=None)
def setup(space, align):
    """The space, 24 + 24 seeded vectors on it and their interiors as columns (shared, never
    modified)."""
    from poms_amd.stencil import StencilVectorSpace
    npts, pads = SPACES[space]
    V = StencilVectorSpace(list(npts), list(pads), align=align)
    rng = np.random.default_rng(17)
    Xn = rng.standard_normal((24,) + npts)
    Yn = rng.standard_normal((24,) + npts)
    xs = [V.zeros().from_numpy(a) for a in Xn]
    ys = [V.zeros().from_numpy(a) for a in Yn]
    return V, xs, ys, Xn.reshape(24, -1).T.copy(), Yn.reshape(24, -1).T.copy()


def n_flat(V):
    """Length of the flat range the kernels sum over (whole interior planes)."""
    return (V.local_npts[0] if V.ndim == 3 else 1) * V.plane_elems


@pytest.mark.parametrize("align", [False, True], ids=["unaligned", "aligned"])
@pytest.mark.parametrize("space", list(SPACES))
@pytest.mark.parametrize("nx,ny", GRAM_SIZES)
def test_gram_against_numpy(gpu, nx, ny, space, align):
    from poms_amd.eigen import block_gram
    V, xs, ys, Xd, Yd = setup(space, align)
    got = block_gram(xs[:nx], ys[:ny]).cpu().numpy()
    want = Xd[:, :nx].T @ Yd[:, :ny]
    bound = n_flat(V) * EPS * (np.abs(Xd[:, :nx]).T @ np.abs(Yd[:, :ny]))
    err = np.abs(got - want)
    print(f"gram {nx}x{ny} {space} align={align}: max err/bound {np.max(err / bound):.3e}")
    assert got.shape == (nx, ny)
    assert np.all(err <= bound)


@pytest.mark.parametrize("align", [False, True], ids=["unaligned", "aligned"])
@pytest.mark.parametrize("space", list(SPACES))
@pytest.mark.parametrize("n", sorted({s[0] for s in GRAM_SIZES if s[0] == s[1]}))
def test_gram_is_reproducible_and_symmetric(gpu, n, space, align):
    from poms_amd.eigen import block_gram
    V, xs, ys, Xd, Yd = setup(space, align)
    full = block_gram(xs[:n], xs[:n]).cpu().numpy()
    again = block_gram(xs[:n], xs[:n]).cpu().numpy()
    assert np.array_equal(full, again)
    sym = block_gram(xs[:n], xs[:n], symmetric=True).cpu().numpy()
    assert np.array_equal(sym, sym.T)
    iu = np.triu_indices(n)
    assert np.array_equal(sym[iu], full[iu])
    assert np.array_equal(sym, block_gram(xs[:n], xs[:n], symmetric=True).cpu().numpy())
    # two different lists: the upper triangle is the full call's there too
    mixed = block_gram(xs[:n], ys[:n], symmetric=True).cpu().numpy()
    assert np.array_equal(mixed[iu], block_gram(xs[:n], ys[:n]).cpu().numpy()[iu])
    assert np.array_equal(mixed, mixed.T)


@pytest.mark.parametrize("align", [False, True], ids=["unaligned", "aligned"])
@pytest.mark.parametrize("space", list(SPACES))
def test_gram_and_vector_dot(gpu, space, align):
    from poms_amd.eigen import block_gram
    V, xs, ys, Xd, Yd = setup(space, align)
    for i, j in ((0, 0), (3, 5)):
        g = float(block_gram([xs[i]], [ys[j]]).cpu().numpy()[0, 0])
        d = xs[i].dot(ys[j])
        bound = n_flat(V) * EPS * float(np.abs(Xd[:, i]) @ np.abs(Yd[:, j]))
        assert abs(g - d) <= bound
        assert abs(g - float(Xd[:, i] @ Yd[:, j])) <= bound


@pytest.mark.parametrize("align", [False, True], ids=["unaligned", "aligned"])
@pytest.mark.parametrize("space", list(SPACES))
@pytest.mark.parametrize("nin,nout", COMBINE_SIZES)
def test_combine_against_numpy(gpu, nin, nout, space, align):
    import torch
    from poms_amd.eigen import block_combine
    V, xs, ys, Xd, Yd = setup(space, align)
    rng = np.random.default_rng(1000 * nin + nout)
    Cm = rng.standard_normal((nin, nout))
    unit = min(nin - 1, 2)
    if nout > 1:                        # a unit column: that input, bitwise (1 -> 1 keeps its
        Cm[:, nout - 1] = 0.0           # random coefficient: a scaled product)
        Cm[unit, nout - 1] = 1.0
    before = [x._store.clone() for x in xs[:nin]]
    outs = [V.empty() for _ in range(nout)]
    for o in outs:                      # (interiors unspecified: fill them with something else)
        V.interior(o._data).fill_(7.25)
    # the coefficients as a host array, and again as a device tensor
    block_combine(xs[:nin], Cm, outs)
    got = np.stack([o.to_local_numpy().reshape(-1) for o in outs], axis=1)
    want = Xd[:, :nin] @ Cm
    bound = nin * EPS * (np.abs(Xd[:, :nin]) @ np.abs(Cm))
    err = np.abs(got - want)
    print(f"combine {nin}->{nout} {space} align={align}: max err/bound "
          f"{np.max(err[bound > 0] / bound[bound > 0]):.3e}")
    assert np.all(err <= bound)
    if nout > 1:
        assert np.array_equal(got[:, nout - 1], Xd[:, unit])
    else:                               # the unit column through the one-output build: a copy
        copy = [V.empty()]
        block_combine(xs[:nin], np.eye(nin, 1), copy)
        assert np.array_equal(copy[0].to_local_numpy().reshape(-1), Xd[:, 0])
    for x, b in zip(xs[:nin], before):
        assert torch.equal(x._store, b)
    # everything of the padded array outside the interior: ghosts and dead pitch columns (an
    # aligned space's buffer also has slack in front of and behind the array: not the vector's)
    outside = torch.zeros_like(outs[0]._store, dtype=torch.bool)
    outside[V.shift:V.shift + V.padded_shape[0] * V.strides[0]] = True
    V.interior(V.view(outside)).fill_(False)
    for o in outs:
        assert torch.count_nonzero(o._store[outside]) == 0
    outs2 = [V.empty() for _ in range(nout)]
    block_combine(xs[:nin], torch.from_numpy(Cm).to(xs[0]._data.device), outs2)
    lo, hi = V.shift, V.shift + V.padded_shape[0] * V.strides[0]   # (the array, without the buffer's slack)
    for o, o2 in zip(outs, outs2):
        assert torch.equal(o._store[lo:hi], o2._store[lo:hi])


@pytest.mark.parametrize("space", list(SPACES))
def test_mixed_phases(gpu, space):
    """Vectors that do not share their 16-B phase (every other one starts one double into its
    buffer) take the 8-B path: the same bounds."""
    import torch
    from poms_amd.eigen import block_combine, block_gram
    from poms_amd.stencil import StencilVector
    V, xs, ys, Xd, Yd = setup(space, False)
    dev = xs[0]._data.device

    def shifted(v, odd):
        big = torch.zeros(V.store_elems + 2, dtype=torch.float64, device=dev)
        w = StencilVector(V, _store=big[:V.store_elems])
        if odd:   # (as_strided's offset counts from the start of the storage)
            w._store = big[1:1 + V.store_elems]
            w._data = torch.as_strided(big, V.padded_shape, V.strides, V.shift + 1)
        return w.assign(v)

    n = 5
    xm = [shifted(x, i % 2 == 1) for i, x in enumerate(xs[:n])]
    ym = [shifted(y, i % 2 == 0) for i, y in enumerate(ys[:n])]
    assert len({x._data.data_ptr() % 16 for x in xm}) == 2
    got = block_gram(xm, ym).cpu().numpy()
    bound = n_flat(V) * EPS * (np.abs(Xd[:, :n]).T @ np.abs(Yd[:, :n]))
    assert np.all(np.abs(got - Xd[:, :n].T @ Yd[:, :n]) <= bound)
    assert np.array_equal(got, block_gram(xm, ym).cpu().numpy())
    Cm = np.random.default_rng(4).standard_normal((n, 3))
    outs = [shifted(V.zeros(), j % 2 == 0) for j in range(3)]
    block_combine(xm, Cm, outs)
    res = np.stack([o.to_local_numpy().reshape(-1) for o in outs], axis=1)
    assert np.all(np.abs(res - Xd[:, :n] @ Cm) <= n * EPS * (np.abs(Xd[:, :n]) @ np.abs(Cm)))
    # the same combination on vectors of one phase: the same bits
    outs1 = [V.empty() for _ in range(3)]
    block_combine(xs[:n], Cm, outs1)
    assert np.array_equal(res, np.stack([o.to_local_numpy().reshape(-1) for o in outs1], axis=1))


def raw_lists(V, xs):
    return (C.c_void_p * len(xs))(*[x._data.data_ptr() for x in xs])


def test_refusals(gpu):
    import torch
    from poms_amd import _lib, runtime as rt
    from poms_amd.eigen import block_combine, block_gram
    V, xs, ys, Xd, Yd = setup("2d_9x12_p23", False)
    outs = [V.empty() for _ in range(17)]
    coef = torch.zeros(24 * 17, dtype=torch.float64, device=xs[0]._data.device)
    small = torch.zeros(25 * 25, dtype=torch.float64, device=xs[0]._data.device)
    comb = lambda ins, os_: _lib.call("poms_block_combine", V.ctx, C.byref(V.layout), len(ins), raw_lists(V, ins),
                                      len(os_), raw_lists(V, os_), rt.ptr(coef), rt.stream_handle())
    with pytest.raises(_lib.PomsError, match="also an input"):
        comb(xs[:3], [outs[0], xs[1]])
    with pytest.raises(_lib.PomsError, match="same vector"):
        comb(xs[:3], [outs[0], outs[1], outs[0]])
    with pytest.raises(_lib.PomsError, match="outputs"):
        comb(xs[:3], outs[:17])
    with pytest.raises(_lib.PomsError, match="inputs"):
        comb(xs + ys[:1], outs[:2])
    with pytest.raises(_lib.PomsError, match="POMS_BLOCK_MAX"):
        _lib.call("poms_block_gram", V.ctx, C.byref(V.layout), 25, raw_lists(V, xs + ys[:1]), 1, raw_lists(V, ys[:1]),
                  0, rt.ptr(small), rt.stream_handle())
    with pytest.raises(_lib.PomsError, match="nx == ny"):
        _lib.call("poms_block_gram", V.ctx, C.byref(V.layout), 2, raw_lists(V, xs[:2]), 3, raw_lists(V, ys[:3]),
                  1, rt.ptr(small), rt.stream_handle())
    # a layout whose ghost rows hold data is refused (the flat range would sum them)
    lay = _lib.Layout.make(V.n3, V.p3, 0, _lib.LAYOUT_GHOST_DATA)
    with pytest.raises(_lib.PomsError, match="GHOST_DATA"):
        _lib.call("poms_block_gram", V.ctx, C.byref(lay), 1, raw_lists(V, xs[:1]), 1, raw_lists(V, ys[:1]),
                  0, rt.ptr(small), rt.stream_handle())
    # the Python wrappers pass these on, and check what they can themselves
    with pytest.raises(_lib.PomsError):
        block_combine(xs[:2], np.ones((2, 1)), [xs[0]])
    with pytest.raises(ValueError, match="2 x 1"):
        block_combine(xs[:2], np.ones((1, 2)), [outs[0]])
    with pytest.raises(TypeError):
        block_gram([], xs[:1])
    # nothing above launched anything: the inputs are intact
    assert np.array_equal(xs[1].to_local_numpy().reshape(-1), Xd[:, 1])
