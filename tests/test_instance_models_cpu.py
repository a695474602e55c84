"""CPU checks of the per-instance model verbs (tinympc_set_model_batch and its _device form, tinympc_clear_model_batch,
tinympc_get_cache_batch): declared, exported and typed in the ctypes table; a NULL handle is refused before anything touches a device;
the Python methods refuse a solver that was never set up."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest
from conftest import ROOT

VERBS = ["tinympc_set_model_batch", "tinympc_set_model_batch_device", "tinympc_clear_model_batch", "tinympc_get_cache_batch"]


def test_verbs_are_declared_exported_and_typed(pkg):
    header = open(os.path.join(ROOT, "include", "tinympc_hip.h")).read()
    lib = pkg.load_library()
    L = pkg._lib
    for name in VERBS:
        assert name + "(tinympc_solver *s" in header
        assert hasattr(lib, name)
        assert L.SIGNATURES[name][0] is C.c_int
    for name in VERBS[:2]:
        assert name + "(tinympc_solver *s, const double *" in header
        args = L.SIGNATURES[name][1]
        assert len(args) == 8
        assert args[1:6] == [C.c_void_p if name.endswith("_device") else L.c_double_p] * 5
        assert args[6:] == [C.c_int] * 2
    assert L.SIGNATURES["tinympc_clear_model_batch"][1] == [L.Handle]
    assert L.SIGNATURES["tinympc_get_cache_batch"][1] == [L.Handle] + [L.c_double_p] * 4 + [L.c_int_p, C.c_int, C.c_int]


@pytest.mark.parametrize("name", VERBS)
def test_null_handle_is_not_initialized(pkg, name):
    lib = pkg.load_library()
    L = pkg._lib
    buf = np.zeros(12 * 12 * 2)
    it = np.zeros(2, dtype=np.int32)
    if name == "tinympc_clear_model_batch":
        rc = lib.tinympc_clear_model_batch(None)
    elif name == "tinympc_get_cache_batch":
        p = buf.ctypes.data_as(L.c_double_p)
        rc = lib.tinympc_get_cache_batch(None, p, p, p, p, it.ctypes.data_as(L.c_int_p), 0, 2)
    else:
        p = C.c_void_p(buf.ctypes.data) if name.endswith("_device") else buf.ctypes.data_as(L.c_double_p)
        rc = getattr(lib, name)(None, p, p, p, p, p, 0, 2)
    assert rc == L.ERR_NOT_INITIALIZED


def test_python_methods_need_setup(pkg):
    s = pkg.TinyMPC()
    calls = (lambda: s.set_model_batch(np.zeros((12, 12, 2)), np.zeros((12, 4, 2)), np.zeros((12, 12, 2)), np.zeros((4, 4, 2))),
             lambda: s.set_model_batch(np.zeros((4, 4, 1)), np.zeros((4, 1, 1)), np.zeros((4, 4, 1)), np.zeros((1, 1, 1)), fdyn=np.zeros((4, 1)), first=3),
             lambda: s.clear_model_batch(), lambda: s.get_cache_batch(), lambda: s.get_cache_batch(first=1, count=2))
    for call in calls:
        with pytest.raises(pkg.TinyMPCError) as ei:
            call()
        assert ei.value.code == pkg._lib.ERR_NOT_INITIALIZED
