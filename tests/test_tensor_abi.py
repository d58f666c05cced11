"""The C entry points of the tensor-coefficient operators
(poms_op_create_matfree_tensor, poms_op_assemble_stencil_tensor) without a device: the
names are declared, bound and exported, null or garbage arguments come back as a status
and a message naming the entry point, never a crash, and the host-side preparation of a
tensor coefficient refuses a wrong ncomp, shape, dtype, device or layout.

Both calls take the arguments of their scalar counterparts with ``a_q`` replaced by
``(g_q, ncomp)``: 16 + 1 = 17 for the matrix-free call, 17 + 1 = 18 for the assembly
(which also has the slab offset ``g0``)."""
import ctypes as C

import numpy as np
import pytest

from poms_amd import _lib

MATFREE, ASSEMBLE = "poms_op_create_matfree_tensor", "poms_op_assemble_stencil_tensor"
ARGS = ["ctx", "layout", "nel", "nq", "p", "first", "es", "ee", "basis", "weights", "nglob", "g_q", "out"]


def _args(name, drop=None, ncomp=3):
    """Well-formed arguments of a 2D p = 2 space of 6 x 6 functions (4 cells per axis);
    the context is null (none exists without a device), g_q a host array nothing reads."""
    from poms_amd.assembly import axis_tables
    from poms_amd.splines import uniform_knots
    t = axis_tables(uniform_knots(2, 4), 2)
    lay = _lib.Layout.make((1, 6, 6), (0, 2, 2))
    gq = np.ones((3, 12, 12))
    keep = [lay, t, gq]

    def arr3(key, dtype):
        out = (C.c_void_p * 3)()
        a = np.ascontiguousarray(t[key], dtype=dtype)
        keep.append(a)
        out[1] = out[2] = a.ctypes.data
        return out

    i3 = lambda key: (C.c_int * 3)(0, int(t[key]), int(t[key]))
    h = C.c_void_p()
    keep.append(h)
    vals = dict(ctx=None, layout=C.byref(lay), nel=i3("nel"), nq=i3("nq"), p=i3("p"), first=arr3("first", np.int32),
                es=arr3("es", np.int32), ee=arr3("ee", np.int32), basis=arr3("basis", np.float64),
                weights=arr3("weights", np.float64), nglob=(C.c_int64 * 3)(1, 6, 6),
                g_q=C.c_void_p(gq.ctypes.data), out=C.byref(h))
    if drop:
        vals[drop] = None
    a = [vals[k] for k in ARGS]
    # (ctx, ndim, layout, nel, nq, p, first, es, ee, basis, weights, nglob, g_q, ncomp, c_q, mass_coef, [g0,] op)
    tail = [a[11], ncomp, None, 1.0] + ([0] if name == ASSEMBLE else []) + [a[12]]
    return [a[0], 2] + a[1:11] + tail, keep, h


def test_tensor_symbols_are_declared_bound_and_exported():
    for name, nargs in ((MATFREE, 17), (ASSEMBLE, 18)):
        assert name in _lib.header_symbols()
        assert name in _lib._SIGS
        fn = getattr(_lib.lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs
    # the scalar calls keep their signatures
    assert len(_lib.lib.poms_op_create_matfree.argtypes) == 16
    assert len(_lib.lib.poms_op_assemble_stencil.argtypes) == 17
    assert _lib.lib.poms_abi_version() >= 6


def test_the_header_cites_the_call_the_entry_points_generalise():
    text = _lib.HEADER_PATH.read_text()
    for name in (MATFREE, ASSEMBLE):
        comment = text[:text.index("int " + name)].rsplit("/*", 1)[1]
        assert "sources/matrix_assembler.py:84-179" in comment.replace("\n * ", " "), name


@pytest.mark.parametrize("name", [MATFREE, ASSEMBLE])
@pytest.mark.parametrize("drop", ARGS)
def test_tensor_calls_reject_null_arguments(name, drop):
    """Every null argument (the context included, g_q too: a tensor operator has no
    default coefficient) is refused before anything is read through it."""
    args, keep, h = _args(name, drop=None if drop == "ctx" else drop)
    assert getattr(_lib.lib, name)(*args) != 0
    msg = _lib.lib.poms_last_error().lower()
    assert b"null" in msg and name.encode() in msg
    assert not h.value
    with pytest.raises(_lib.PomsError, match="null"):
        _lib.call(name, *args)


@pytest.mark.parametrize("name", [MATFREE, ASSEMBLE])
def test_tensor_calls_with_garbage_sizes_and_a_null_context_do_not_crash(name):
    lay = _lib.Layout.make((-3, 0, 1 << 40), (-1, 7, 99))
    bad_i = (C.c_int * 3)(-1, 0, 1 << 30)
    bad = (C.c_int64 * 3)(-1, 0, 1 << 62)
    parr = (C.c_void_p * 3)(None, None, None)
    h = C.c_void_p()
    g0 = [1 << 50] if name == ASSEMBLE else []
    for ndim in (-1, 0, 1, 2, 3, 4, 1 << 20):
        for ncomp in (-7, 0, 3, 6, 1 << 30):
            assert getattr(_lib.lib, name)(None, ndim, C.byref(lay), bad_i, bad_i, bad_i, parr, parr, parr, parr, parr,
                                           bad, None, ncomp, None, float("nan"), *g0, C.byref(h)) != 0
            assert _lib.lib.poms_last_error() and not h.value


def test_geometry_names_are_exported_lazily():
    import poms_amd
    for name in ("Mapping", "SplineMapping", "MappedDomain", "pullback"):
        assert name in poms_amd.__all__
        assert getattr(poms_amd, name).__name__ == name


def _tabs():
    from poms_amd.assembly import axis_tables
    from poms_amd.splines import uniform_knots
    return [axis_tables(uniform_knots(2, 4), 2), axis_tables(uniform_knots(3, 5), 3)], (4 * 3, 5 * 4)


def test_the_number_of_dimensions_tells_a_tensor_from_a_scalar_field():
    from poms_amd.assembly import split_coef, tensor_ncomp
    tabs, shape = _tabs()
    assert [tensor_ncomp(d) for d in (1, 2, 3)] == [1, 3, 6]
    assert split_coef(None, tabs) == (None, False)
    assert split_coef(2.0, tabs)[1] is False
    assert split_coef(np.ones(shape), tabs)[1] is False
    assert split_coef(np.ones((3,) + shape), tabs)[1] is True
    assert split_coef(lambda x, y: 1.0 + x * y, tabs)[1] is False
    vals, tensor = split_coef(lambda x, y: np.stack([1 + x, x * y, 2 + y]), tabs)
    assert tensor and vals.shape == (3,) + shape
    # the callable sees the meshgrid of the quadrature points, indexing='ij'
    assert np.array_equal(vals[0][:, 0], 1 + tabs[0]["points"].reshape(-1))
    assert np.array_equal(vals[2][0, :], 2 + tabs[1]["points"].reshape(-1))


def test_tensor_preparation_checks_ncomp_shape_dtype_device_and_layout_on_the_host():
    import torch
    from poms_amd.assembly import tensor_coef
    tabs, shape = _tabs()
    ok = tensor_coef(np.ones((3,) + shape), tabs, "cpu")
    assert ok.dtype == torch.float64 and tuple(ok.shape) == (3,) + shape and ok.is_contiguous()
    t = torch.ones((3,) + shape, dtype=torch.float64)
    assert tensor_coef(t, tabs, "cpu") is t          # a tensor of the right kind is used in place
    for ncomp in (1, 2, 4, 6):
        with pytest.raises(ValueError, match="ncomp"):
            tensor_coef(np.ones((ncomp,) + shape), tabs, "cpu")
    for bad in (np.ones((3,) + shape[::-1]), np.ones((3, 3, 3)), np.ones((3,) + shape + (1,)), np.ones(shape)):
        with pytest.raises(ValueError, match="shape"):
            tensor_coef(bad, tabs, "cpu")
    with pytest.raises(TypeError, match="float64"):
        tensor_coef(torch.ones((3,) + shape, dtype=torch.float32), tabs, "cpu")
    with pytest.raises(ValueError, match="lives on"):
        tensor_coef(t, tabs, "cuda:0")
    with pytest.raises(ValueError, match="contiguous"):
        tensor_coef(torch.ones(shape + (3,), dtype=torch.float64).permute(2, 0, 1), tabs, "cpu")
    # a 3D space wants six components
    tabs3 = [tabs[0]] * 3
    with pytest.raises(ValueError, match="ncomp"):
        tensor_coef(np.ones((3, 12, 12, 12)), tabs3, "cpu")
    assert tuple(tensor_coef(np.ones((6, 12, 12, 12)), tabs3, "cpu").shape) == (6, 12, 12, 12)
