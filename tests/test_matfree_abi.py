"""The C entry points of the matrix-free operator (csrc/matfree.hip,
poms_op_create_matfree, poms_op_diagonal) without a device: the names are declared,
bound and exported, null or garbage arguments come back as a status and a message,
never a crash, and the host-side preparation of the coefficient arguments refuses a
wrong shape."""
import ctypes as C

import numpy as np
import pytest

from poms_amd import _lib

NAME = "poms_op_create_matfree"
ARGS = ["ctx", "layout", "nel", "nq", "p", "first", "es", "ee", "basis", "weights", "nglob", "out"]


def _args(drop=None, ctx=None):
    """Well-formed arguments of a 2D p = 2 space of 6 x 6 functions (4 cells per axis)."""
    from poms_amd.assembly import axis_tables
    from poms_amd.splines import uniform_knots
    t = axis_tables(uniform_knots(2, 4), 2)
    lay = _lib.Layout.make((1, 6, 6), (0, 2, 2))
    keep = [lay, t]

    def arr3(key, dtype):
        out = (C.c_void_p * 3)()
        a = np.ascontiguousarray(t[key], dtype=dtype)
        keep.append(a)
        out[1] = out[2] = a.ctypes.data
        return out

    i3 = lambda key: (C.c_int * 3)(0, int(t[key]), int(t[key]))
    h = C.c_void_p()
    keep.append(h)
    vals = dict(ctx=ctx, layout=C.byref(lay), nel=i3("nel"), nq=i3("nq"), p=i3("p"), first=arr3("first", np.int32),
                es=arr3("es", np.int32), ee=arr3("ee", np.int32), basis=arr3("basis", np.float64),
                weights=arr3("weights", np.float64), nglob=(C.c_int64 * 3)(1, 6, 6), out=C.byref(h))
    if drop:
        vals[drop] = None
    a = [vals[k] for k in ARGS]
    # (ctx, ndim, layout, nel, nq, p, first, es, ee, basis, weights, nglob, a_q, c_q, mass_coef, op)
    return [a[0], 2] + a[1:11] + [None, None, 1.0, a[11]], keep, h


def test_matfree_symbols_are_declared_bound_and_exported():
    for name, nargs in ((NAME, 16), ("poms_op_diagonal", 2)):
        assert name in _lib.header_symbols()
        assert name in _lib._SIGS
        fn = getattr(_lib.lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == nargs
    assert _lib.lib.poms_abi_version() >= 5


@pytest.mark.parametrize("drop", ARGS)
def test_matfree_rejects_null_arguments(drop):
    """Every null argument (the context included: none exists without a device) is
    refused before anything is read through it."""
    args, keep, h = _args(drop=None if drop == "ctx" else drop)
    assert getattr(_lib.lib, NAME)(*args) != 0
    msg = _lib.lib.poms_last_error().lower()
    assert b"null" in msg and NAME.encode() in msg
    assert not h.value
    with pytest.raises(_lib.PomsError, match="null"):
        _lib.call(NAME, *args)


def test_matfree_garbage_sizes_with_a_null_context_do_not_crash():
    lay = _lib.Layout.make((-3, 0, 1 << 40), (-1, 7, 99))
    bad_i = (C.c_int * 3)(-1, 0, 1 << 30)
    bad = (C.c_int64 * 3)(-1, 0, 1 << 62)
    parr = (C.c_void_p * 3)(None, None, None)
    h = C.c_void_p()
    for ndim in (-1, 0, 1, 2, 3, 4, 1 << 20):
        assert getattr(_lib.lib, NAME)(None, ndim, C.byref(lay), bad_i, bad_i, bad_i, parr, parr, parr, parr, parr, bad,
                                       None, None, float("nan"), C.byref(h)) != 0
        assert _lib.lib.poms_last_error() and not h.value


def test_diagonal_rejects_null_arguments():
    out = np.zeros(4)
    assert _lib.lib.poms_op_diagonal(None, out.ctypes.data_as(C.c_void_p)) != 0
    assert b"null" in _lib.lib.poms_last_error().lower()
    assert _lib.lib.poms_op_diagonal(None, None) != 0


def test_matfree_names_are_exported_lazily():
    import poms_amd
    for name in ("MatrixFreeOperator", "MatrixFreeVCycle"):
        assert name in poms_amd.__all__
        assert getattr(poms_amd, name).__name__ == name


def test_coefficient_preparation_checks_the_shape_on_the_host():
    """An array that is not of the quadrature grid's shape is a ValueError before any
    device is touched; None stays None (a = 1, c = mass_coef: no array is read)."""
    from poms_amd.assembly import axis_tables
    from poms_amd.matfree import _coef_arg
    from poms_amd.splines import uniform_knots
    tabs = [axis_tables(uniform_knots(2, 4), 2), axis_tables(uniform_knots(3, 5), 3)]
    shape = (4 * 3, 5 * 4)
    assert _coef_arg(None, tabs, "cuda:0") is None
    for bad in (np.ones((3, 3)), np.ones(shape[::-1]), np.ones(shape + (1,)), np.ones(shape[0])):
        with pytest.raises(ValueError, match="shape"):
            _coef_arg(bad, tabs, "cuda:0")
    import torch
    with pytest.raises(ValueError, match="shape"):
        _coef_arg(torch.ones(3, 3, dtype=torch.float64), tabs, "cpu")
    with pytest.raises(TypeError, match="float64"):
        _coef_arg(torch.ones(*shape, dtype=torch.float32), tabs, "cpu")
