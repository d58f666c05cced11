"""The C entry points of the scattered-point kernels (csrc/spline_points.hip) that need no
device: every one refuses a null handle with a message, destroy(NULL) is a no-op, and the
names are declared, bound and exported."""
import ctypes as C

import pytest

from poms_amd import _lib

RUN_CALLS = {
    # name: arguments after a null handle
    "poms_points_info": (None,),
    "poms_points_cells": (None, 1, None, None),
    "poms_points_eval": (None, None, 1, 0, None, None),
    "poms_points_deposit_atomic": (None, None, 1, None, None),
    "poms_points_deposit_binned": (None, None, 1, None, None, 0, 1, 0, None, None),
}


def test_points_symbols_are_declared_and_bound():
    names = {n for n in _lib.header_symbols() if n.startswith("poms_points_")}
    assert names == set(RUN_CALLS) | {"poms_points_create", "poms_points_destroy"}
    assert names <= set(_lib._SIGS)
    for n in names:
        assert getattr(_lib.lib, n).restype is C.c_int


def test_points_destroy_null_is_a_no_op():
    assert _lib.lib.poms_points_destroy(None) == 0


@pytest.mark.parametrize("name", sorted(RUN_CALLS))
def test_points_entry_points_reject_null_handles(name):
    lib = _lib.lib
    assert getattr(lib, name)(None, *RUN_CALLS[name]) != 0
    msg = lib.poms_last_error().lower()
    assert b"null" in msg and name.encode() in msg
    with pytest.raises(_lib.PomsError, match="null"):
        _lib.call(name, None, *RUN_CALLS[name])


def test_points_create_rejects_null_arguments():
    h = C.c_void_p()
    assert _lib.lib.poms_points_create(None, 3, None, None, None, None, 1 << 20, C.byref(h)) != 0
    assert b"null" in _lib.lib.poms_last_error().lower() and not h.value
    with pytest.raises(_lib.PomsError):
        _lib.call("poms_points_create", None, 3, None, None, None, None, 1 << 20, C.byref(h))


def test_points_names_are_exported_lazily():
    import poms_amd
    for name in ("SplinePoints", "Binning", "evaluate_at", "deposit"):
        assert name in poms_amd.__all__
