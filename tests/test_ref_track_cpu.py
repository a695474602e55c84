"""CPU checks of the reference-track verbs (tinympc_set_x_ref_track_batch / _u_ref_track_batch, the step verbs and auto-advance):
declared, exported and typed in the ctypes table; a NULL handle is refused before anything touches a device; the Python methods
refuse a solver that was never set up, and wrong shapes before any call into the library."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest
from conftest import ROOT

TRACK_VERBS = ["tinympc_set_x_ref_track_batch", "tinympc_set_u_ref_track_batch", "tinympc_set_x_ref_track_batch_device",
               "tinympc_set_u_ref_track_batch_device"]
STEP_VERBS = ["tinympc_set_ref_step_batch", "tinympc_set_ref_step_batch_device", "tinympc_get_ref_step_batch"]
SCALAR_VERBS = ["tinympc_advance_ref_step_batch", "tinympc_set_ref_auto_advance"]


def test_verbs_are_declared_exported_and_typed(pkg):
    header = open(os.path.join(ROOT, "include", "tinympc_hip.h")).read()
    lib, sig, L = pkg.load_library(), pkg._lib.SIGNATURES, pkg._lib
    for name in TRACK_VERBS:
        assert name + "(tinympc_solver *s, const double *" in header
        assert hasattr(lib, name)
        restype, args = sig[name]
        assert restype is C.c_int and len(args) == 6
        assert args[1] is (C.c_void_p if name.endswith("_device") else L.c_double_p)
        assert args[2:] == [C.c_int] * 4
    for name in STEP_VERBS:
        assert name + "(tinympc_solver *s, " in header and hasattr(lib, name)
        restype, args = sig[name]
        assert restype is C.c_int and len(args) == 4
        assert args[1] is (C.c_void_p if name.endswith("_device") else L.c_int_p)
        assert args[2:] == [C.c_int] * 2
    for name in SCALAR_VERBS:
        assert name + "(tinympc_solver *s, int delta)" in header and hasattr(lib, name)
        assert sig[name] == (C.c_int, [L.Handle, C.c_int])
    assert pkg.abi_version() == 1  # (an extension: the ABI version stays)


@pytest.mark.parametrize("name", TRACK_VERBS + STEP_VERBS + SCALAR_VERBS)
def test_null_handle_is_not_initialized(pkg, name):
    lib = pkg.load_library()
    if name in TRACK_VERBS:
        buf = np.zeros(12 * 20 * 2)
        ptr = C.c_void_p(buf.ctypes.data) if name.endswith("_device") else buf.ctypes.data_as(pkg._lib.c_double_p)
        rc = getattr(lib, name)(None, ptr, 12, 20, 0, 2)
    elif name in STEP_VERBS:
        buf = np.zeros(2, dtype=np.int32)
        ptr = C.c_void_p(buf.ctypes.data) if name.endswith("_device") else buf.ctypes.data_as(pkg._lib.c_int_p)
        rc = getattr(lib, name)(None, ptr, 0, 2)
    else:
        rc = getattr(lib, name)(None, 1)
    assert rc == pkg._lib.ERR_NOT_INITIALIZED


def test_python_methods_need_setup(pkg):
    s = pkg.TinyMPC()
    for call in (lambda: s.set_x_ref_track_batch(np.zeros((12, 20, 4))), lambda: s.set_u_ref_track_batch(np.zeros((4, 7, 4)), first=2),
                 lambda: s.set_ref_step_batch([0, 1]), lambda: s.advance_ref_step(1), lambda: s.set_ref_auto_advance(1),
                 lambda: s.get_ref_step_batch()):
        with pytest.raises(pkg.TinyMPCError) as ei:
            call()
        assert ei.value.code == pkg._lib.ERR_NOT_INITIALIZED


class _NoLibrary:
    """Stands in for the loaded library: any call into it fails the test."""

    def __getattr__(self, name):
        def verb(*args):
            raise AssertionError("the library was called (%s) although the arguments are malformed" % name)
        return verb


def _solver_without_library(pkg, batch):
    s = pkg.TinyMPC()
    s.nx, s.nu, s.N, s.batch, s.is_setup = 12, 4, 10, batch, True
    s._L = _NoLibrary()
    return s


def test_python_methods_reject_wrong_shapes_before_the_library(pkg):
    s = _solver_without_library(pkg, 8)
    bad = [lambda: s.set_x_ref_track_batch(np.zeros((12, 20))),         # a batched solver needs nx x T x count
           lambda: s.set_x_ref_track_batch(np.zeros((11, 20, 8))),      # wrong rows
           lambda: s.set_x_ref_track_batch(np.zeros((12, 0, 8))),       # T = 0
           lambda: s.set_u_ref_track_batch(np.zeros((12, 20, 8))),      # x-shaped tracks for u
           lambda: s.set_u_ref_track_batch(np.zeros((4, 5, 8, 1))),     # four dimensions
           lambda: s.set_ref_step_batch(np.zeros((2, 4), dtype=np.int32)),  # not a vector
           lambda: s.set_ref_step_batch(np.array([0.5, 1.0])),          # not integers
           lambda: s.set_ref_step_batch(np.array([2**31]))]             # beyond 32 bits
    for call in bad:
        with pytest.raises(pkg.TinyMPCError) as ei:
            call()
        assert ei.value.code == pkg._lib.ERR_INVALID_INPUT
    s.is_setup = False  # (nothing to release)
    s._L = None


def test_single_instance_tracks_may_be_two_dimensional(pkg):
    """nx x T on a single-instance solver reaches the library as nx x T x 1."""
    calls = []

    class L(_NoLibrary):
        def tinympc_set_x_ref_track_batch(self, h, p, rows, T, first, count):
            calls.append((rows, T, first, count))
            return 0

    s = _solver_without_library(pkg, 1)
    s._L = L()
    s.set_x_ref_track_batch(np.zeros((12, 33)))
    assert calls == [(12, 33, 0, 1)]
    s.is_setup = False
    s._L = None
