"""CPU checks of the per-instance rho verbs (tinympc_set_rho_batch and its _device form): declared, exported and typed in the ctypes
table; a NULL handle is refused before anything touches a device; the Python method refuses a solver that was never set up."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest
from conftest import ROOT

VERBS = ["tinympc_set_rho_batch", "tinympc_set_rho_batch_device"]


def test_verbs_are_declared_exported_and_typed(pkg):
    header = open(os.path.join(ROOT, "include", "tinympc_hip.h")).read()
    lib = pkg.load_library()
    L = pkg._lib
    for name in VERBS:
        assert "int " + name + "(tinympc_solver *s, const double *" in header
        assert hasattr(lib, name)
        res, args = L.SIGNATURES[name]
        assert res is C.c_int
        assert args == [L.Handle, C.c_void_p if name.endswith("_device") else L.c_double_p, C.c_int, C.c_int]
    assert "rho, N and the settings stay the handle's" not in header  # (the model verb's comment points to the new verb instead)


@pytest.mark.parametrize("name", VERBS)
def test_null_handle_is_not_initialized(pkg, name):
    lib = pkg.load_library()
    L = pkg._lib
    buf = np.ones(4)
    p = C.c_void_p(buf.ctypes.data) if name.endswith("_device") else buf.ctypes.data_as(L.c_double_p)
    assert getattr(lib, name)(None, p, 0, 2) == L.ERR_NOT_INITIALIZED
    assert getattr(lib, name)(None, None, 0, 2) == L.ERR_NOT_INITIALIZED


def test_python_method_needs_setup(pkg):
    s = pkg.TinyMPC()
    for call in (lambda: s.set_rho_batch(np.ones(3)), lambda: s.set_rho_batch(np.ones(2), first=5)):
        with pytest.raises(pkg.TinyMPCError) as ei:
            call()
        assert ei.value.code == pkg._lib.ERR_NOT_INITIALIZED
