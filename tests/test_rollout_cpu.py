"""CPU checks of the closed-loop rollout verbs (tinympc_rollout_batch and its _device form, tinympc_plant_step_batch, tinympc_set_plant_batch
and its _device form, tinympc_clear_plant_batch): declared in the header with the documented signatures, exported and typed in the ctypes
table; a NULL handle is refused before anything touches a device; the Python methods refuse a solver that was never set up and arguments
of the wrong shape; the ABI version stays 1."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest
from conftest import ROOT

DECLARATIONS = {
    "tinympc_rollout_batch": "int tinympc_rollout_batch(tinympc_solver *s, int ticks, const double *disturbance, const tinympc_rollout_logs *logs, float *gpu_ms);",
    "tinympc_rollout_batch_device": "int tinympc_rollout_batch_device(tinympc_solver *s, int ticks, const double *d_disturbance, const tinympc_rollout_logs *d_logs);",
    "tinympc_plant_step_batch": "int tinympc_plant_step_batch(tinympc_solver *s, const double *disturbance);",
    "tinympc_set_plant_batch": "int tinympc_set_plant_batch(tinympc_solver *s, const double *A, const double *B, const double *f, int first, int count);",
    "tinympc_set_plant_batch_device": "int tinympc_set_plant_batch_device(tinympc_solver *s, const double *d_A, const double *d_B, const double *d_f, int first, int count);",
    "tinympc_clear_plant_batch": "int tinympc_clear_plant_batch(tinympc_solver *s);",
}
LOGS_TYPE = "typedef struct { double *x_log, *u_log; int *iter_log, *status_log; } tinympc_rollout_logs;"


def test_verbs_are_declared_exported_and_typed(pkg):
    header = open(os.path.join(ROOT, "include", "tinympc_hip.h")).read()
    lib, L = pkg.load_library(), pkg._lib
    assert LOGS_TYPE in header
    for name, text in DECLARATIONS.items():
        assert text in header, name
        assert hasattr(lib, name), name
        assert L.SIGNATURES[name][0] is C.c_int
    H, dp, vp, logs = L.Handle, L.c_double_p, C.c_void_p, C.POINTER(L.RolloutLogs)
    assert L.SIGNATURES["tinympc_rollout_batch"][1] == [H, C.c_int, dp, logs, C.POINTER(C.c_float)]
    assert L.SIGNATURES["tinympc_rollout_batch_device"][1] == [H, C.c_int, vp, logs]
    assert L.SIGNATURES["tinympc_plant_step_batch"][1] == [H, dp]
    assert L.SIGNATURES["tinympc_set_plant_batch"][1] == [H, dp, dp, dp, C.c_int, C.c_int]
    assert L.SIGNATURES["tinympc_set_plant_batch_device"][1] == [H, vp, vp, vp, C.c_int, C.c_int]
    assert L.SIGNATURES["tinympc_clear_plant_batch"][1] == [H]
    # the struct of the ctypes table is the header's: four pointers, in the header's order
    assert [n for n, _ in L.RolloutLogs._fields_] == ["x_log", "u_log", "iter_log", "status_log"]
    assert C.sizeof(L.RolloutLogs) == 4 * C.sizeof(C.c_void_p)


def test_abi_version_is_unchanged(pkg):
    header = open(os.path.join(ROOT, "include", "tinympc_hip.h")).read()
    assert "#define TINYMPC_ABI_VERSION 1" in header  # (symbols were added, nothing changed)
    assert pkg.abi_version() == 1


def test_null_handle_is_not_initialized(pkg):
    lib, L = pkg.load_library(), pkg._lib
    a = np.ones(4)
    p, v = a.ctypes.data_as(L.c_double_p), C.c_void_p(a.ctypes.data)
    logs = L.RolloutLogs(None, None, None, None)
    ms = C.c_float(-1.0)
    E = L.ERR_NOT_INITIALIZED
    assert lib.tinympc_rollout_batch(None, 3, None, None, None) == E
    assert "not initialized" in L.last_error().lower()
    assert lib.tinympc_rollout_batch(None, 3, p, C.byref(logs), C.byref(ms)) == E
    assert ms.value == -1.0
    assert lib.tinympc_rollout_batch_device(None, 3, None, None) == E
    assert lib.tinympc_rollout_batch_device(None, 3, v, C.byref(logs)) == E
    assert lib.tinympc_plant_step_batch(None, None) == E
    assert lib.tinympc_plant_step_batch(None, p) == E
    assert lib.tinympc_set_plant_batch(None, p, p, None, 0, 1) == E
    assert lib.tinympc_set_plant_batch_device(None, v, v, v, 0, 1) == E
    assert lib.tinympc_clear_plant_batch(None) == E


def test_python_methods_need_setup(pkg):
    s = pkg.TinyMPC()
    for call in (lambda: s.rollout(3), lambda: s.rollout(3, disturbance=np.zeros((2, 3, 1)), log=("x",)), lambda: s.plant_step(),
                 lambda: s.plant_step(np.zeros((2, 1))), lambda: s.set_plant_batch(np.ones((2, 2, 1)), np.ones((2, 1, 1))),
                 lambda: s.clear_plant_batch()):
        with pytest.raises(pkg.TinyMPCError) as ei:
            call()
        assert ei.value.code == pkg._lib.ERR_NOT_INITIALIZED


def test_python_methods_check_shapes_before_the_library(pkg, monkeypatch):
    """What the wrapper refuses on its own: a disturbance that is not nx x ticks x batch (rollout) or nx x batch (plant_step), ticks < 1,
    unknown log names, plant arrays that are not nx x nx x count / nx x nu x count / nx x count or differ in count. (_check_setup is stepped
    over: no handle, no device -- a call that got past the wrapper's checks would fail on the missing library handle.)"""
    s = pkg.TinyMPC()
    monkeypatch.setattr(s, "_check_setup", lambda: None)
    s.nx, s.nu, s.N, s.batch = 4, 2, 10, 3
    E = pkg._lib.ERR_INVALID_INPUT
    bad = [lambda: s.rollout(0), lambda: s.rollout(-2),
           lambda: s.rollout(5, disturbance=np.zeros((4, 5))), lambda: s.rollout(5, disturbance=np.zeros((4, 4, 3))),
           lambda: s.rollout(5, disturbance=np.zeros((3, 5, 4))), lambda: s.rollout(5, disturbance=np.zeros((4, 5, 2))),
           lambda: s.rollout(5, log=("x", "residuals")),
           lambda: s.plant_step(np.zeros(4)), lambda: s.plant_step(np.zeros((4, 2))), lambda: s.plant_step(np.zeros((3, 4))),
           lambda: s.set_plant_batch(np.ones((4, 4)), np.ones((4, 2, 3))), lambda: s.set_plant_batch(np.ones((4, 4, 3)), np.ones((2, 4, 3))),
           lambda: s.set_plant_batch(np.ones((4, 3, 3)), np.ones((4, 2, 3))), lambda: s.set_plant_batch(np.ones((4, 4, 3)), np.ones((4, 2, 2))),
           lambda: s.set_plant_batch(np.ones((4, 4, 3)), np.ones((4, 2, 3)), f=np.ones((3, 3))),
           lambda: s.set_plant_batch(np.ones((4, 4, 3)), np.ones((4, 2, 3)), f=np.ones((4, 2))),
           lambda: s.set_plant_batch(None, np.ones((4, 2, 3)))]
    for i, call in enumerate(bad):
        with pytest.raises(pkg.TinyMPCError) as ei:
            call()
        assert ei.value.code == E, i
