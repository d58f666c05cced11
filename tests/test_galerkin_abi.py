"""The C entry point of the device Galerkin product (csrc/stencil_galerkin.hip,
poms_op_galerkin_stencil) without a device: the name is declared, bound and exported, and
null or garbage arguments come back as a status and a message, never a crash."""
import ctypes as C

import numpy as np
import pytest

from poms_amd import _lib

NAME = "poms_op_galerkin_stencil"


def _args(layout=True, nf=True, nc=True, P=True, out=True):
    lay = _lib.Layout.make((1, 6, 6), (0, 2, 2))
    n3 = (C.c_int64 * 3)(1, 6, 6)
    ones = np.ones((1, 1))
    parr = (C.c_void_p * 3)(*[ones.ctypes.data_as(C.c_void_p)] * 3)
    h = C.c_void_p()
    keep = (lay, n3, ones, parr, h)
    return (C.byref(lay) if layout else None, n3 if nf else None, n3 if nc else None, parr if P else None,
            C.byref(h) if out else None), keep


def test_galerkin_symbol_is_declared_bound_and_exported():
    assert NAME in _lib.header_symbols()
    assert NAME in _lib._SIGS
    fn = getattr(_lib.lib, NAME)
    assert fn.restype is C.c_int and len(fn.argtypes) == 6


@pytest.mark.parametrize("drop", ["fine", "layout", "nf", "nc", "P", "out"])
def test_galerkin_rejects_null_arguments(drop):
    """Every null argument (the operator handle included: none exists without a device)
    is refused before anything is read through it."""
    args, keep = _args(**({drop: False} if drop != "fine" else {}))
    assert getattr(_lib.lib, NAME)(None, *args) != 0
    msg = _lib.lib.poms_last_error().lower()
    assert b"null" in msg and NAME.encode() in msg
    assert not keep[-1].value
    with pytest.raises(_lib.PomsError, match="null"):
        _lib.call(NAME, None, *args)


def test_galerkin_garbage_sizes_with_a_null_operator_do_not_crash():
    lay = _lib.Layout.make((-3, 0, 1 << 40), (-1, 7, 99))
    bad = (C.c_int64 * 3)(-1, 0, 1 << 62)
    parr = (C.c_void_p * 3)(None, None, None)
    h = C.c_void_p()
    assert getattr(_lib.lib, NAME)(None, C.byref(lay), bad, bad, parr, C.byref(h)) != 0
    assert _lib.lib.poms_last_error() and not h.value


def test_galerkin_names_are_exported_lazily():
    import poms_amd
    for name in ("galerkin_stencil", "GalerkinVCycle"):
        assert name in poms_amd.__all__
