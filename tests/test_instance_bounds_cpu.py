"""CPU checks of the per-instance bound verbs (tinympc_set_bound_constraints_batch and its _device form): declared, exported and typed
in the ctypes table; a NULL handle is refused before anything touches a device; the Python method refuses a solver that was never set
up."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest
from conftest import ROOT

VERBS = ["tinympc_set_bound_constraints_batch", "tinympc_set_bound_constraints_batch_device"]


def test_verbs_are_declared_exported_and_typed(pkg):
    header = open(os.path.join(ROOT, "include", "tinympc_hip.h")).read()
    lib = pkg.load_library()
    for name in VERBS:
        assert name + "(tinympc_solver *s, const double *" in header
        assert hasattr(lib, name)
        restype, args = pkg._lib.SIGNATURES[name]
        assert restype is C.c_int and len(args) == 8
        assert args[1:5] == [C.c_void_p if name.endswith("_device") else pkg._lib.c_double_p] * 4
        assert args[5:] == [C.c_int] * 3


@pytest.mark.parametrize("name", VERBS)
def test_null_handle_is_not_initialized(pkg, name):
    lib = pkg.load_library()
    buf = np.zeros(12 * 50 * 2)
    ptr = C.c_void_p(buf.ctypes.data) if name.endswith("_device") else buf.ctypes.data_as(pkg._lib.c_double_p)
    assert getattr(lib, name)(None, ptr, ptr, ptr, ptr, 50, 0, 2) == pkg._lib.ERR_NOT_INITIALIZED


def test_python_method_needs_setup(pkg):
    s = pkg.TinyMPC()
    for call in (lambda: s.set_bound_constraints_batch(np.zeros((12, 4)), np.ones((12, 4)), np.zeros((4, 4)), np.ones((4, 4))),
                 lambda: s.set_bound_constraints_batch(np.zeros((12, 50, 4)), np.ones((12, 50, 4)), np.zeros((4, 49, 4)),
                                                       np.ones((4, 49, 4)), first=2)):
        with pytest.raises(pkg.TinyMPCError) as ei:
            call()
        assert ei.value.code == pkg._lib.ERR_NOT_INITIALIZED
