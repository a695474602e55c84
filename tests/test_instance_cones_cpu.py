"""CPU checks of the per-instance cone-slope verbs (tinympc_set_cone_slopes_batch and its _device form): declared, exported and typed in
the ctypes table; a NULL handle is refused before anything touches a device; the Python method refuses a solver that was never set up
and arguments of the wrong shape; the sharding helper cuts the verb's arrays along the instance axis; and the sample conditions of the
GPU tests' converging cases hold on the plain-C oracle alone (instance_cone_cases.py states the recipe and the conditions)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest
from conftest import ROOT

import instance_cone_cases as K

VERBS = ["tinympc_set_cone_slopes_batch", "tinympc_set_cone_slopes_batch_device"]


def test_verbs_are_declared_exported_and_typed(pkg):
    header = open(os.path.join(ROOT, "include", "tinympc_hip.h")).read()
    lib = pkg.load_library()
    L = pkg._lib
    for name in VERBS:
        assert "int " + name + "(tinympc_solver *s, const double *" in header
        assert hasattr(lib, name)
        res, args = L.SIGNATURES[name]
        ptr = C.c_void_p if name.endswith("_device") else L.c_double_p
        assert res is C.c_int
        assert args == [L.Handle, ptr, C.c_int, ptr, C.c_int, C.c_int, C.c_int]
    assert "#define TINYMPC_ABI_VERSION 1" in header  # (symbols were added, nothing changed)


@pytest.mark.parametrize("name", VERBS)
def test_null_handle_is_not_initialized(pkg, name):
    lib = pkg.load_library()
    L = pkg._lib
    c = np.ones(2)
    p = C.c_void_p(c.ctypes.data) if name.endswith("_device") else c.ctypes.data_as(L.c_double_p)
    assert getattr(lib, name)(None, p, 1, p, 1, 0, 1) == L.ERR_NOT_INITIALIZED
    assert getattr(lib, name)(None, None, 0, None, 0, 0, 1) == L.ERR_NOT_INITIALIZED


def test_python_method_needs_setup(pkg):
    s = pkg.TinyMPC()
    for call in (lambda: s.set_cone_slopes_batch(np.ones((1, 3)), np.ones((1, 3))), lambda: s.set_cone_slopes_batch(None, np.ones((2, 2)), first=5)):
        with pytest.raises(pkg.TinyMPCError) as ei:
            call()
        assert ei.value.code == pkg._lib.ERR_NOT_INITIALIZED


def test_python_method_checks_shapes_before_the_library(pkg, monkeypatch):
    """What the wrapper refuses on its own: arrays that are not (nc, count), sides with different counts, no slopes at all. (_check_setup is
    stepped over: no handle, no device -- a call that got past the wrapper's checks would fail on the missing library handle.)"""
    s = pkg.TinyMPC()
    monkeypatch.setattr(s, "_check_setup", lambda: None)
    s.batch = 3
    E = pkg._lib.ERR_INVALID_INPUT
    for cx, cu in ((np.ones((1, 3, 2)), None), (np.ones(3), np.ones((1, 3))), (np.ones((1, 3)), np.ones((1, 4))), (None, None),
                   (np.zeros((0, 3)), np.zeros((0, 3)))):
        with pytest.raises(pkg.TinyMPCError) as ei:
            s.set_cone_slopes_batch(cx, cu)
        assert ei.value.code == E, (cx, cu)


def test_sharding_cuts_the_instance_axis(pkg):
    B = pkg.batch
    cx, cu = np.arange(37.0)[None, :] + 1.0, np.arange(74.0).reshape(2, 37) + 1.0
    seen = []
    for rank in range(4):
        first, (sx, su, none) = B.shard_instances((cx, cu, None), rank, 4)
        assert (first, sx.shape[-1]) == B.shard_range(37, rank, 4) and none is None
        np.testing.assert_array_equal(sx, cx[:, first:first + sx.shape[-1]])
        np.testing.assert_array_equal(su, cu[:, first:first + su.shape[-1]])
        seen += list(range(first, first + sx.shape[-1]))
    assert seen == list(range(37))


@pytest.mark.parametrize("name", K.CONDITIONED)
def test_sample_conditions_hold_on_the_oracle(pkg, name):
    _, _, settings = K.case(pkg, name)
    K.assert_sample_conditions(name, settings, *K.reference(pkg, name))
