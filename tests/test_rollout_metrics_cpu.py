"""CPU checks of the rollout metrics' verbs (tinympc_set_rollout_metrics, tinympc_reset_rollout_metrics, tinympc_clear_rollout_metrics,
tinympc_get_rollout_metrics, tinympc_get_rollout_metrics_device_ptr): the declarations and the struct stand in the header verbatim, the
symbols are exported and typed in the ctypes table; a NULL handle is refused before anything touches a device; the Python methods refuse
a solver that was never set up and arguments of the wrong shape; the ABI version stays 1. The numpy restatement of the eight slots
(tests/rollout_metrics_cases.py) is checked against hand-computed rows here, so that the GPU tests compare against something known."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest
from conftest import ROOT

from rollout_metrics_cases import NAMES, restate

SCORE_TYPE = "typedef struct { const double *qx, *ru; double settle_tol; } tinympc_rollout_score;  /* qx: nx weights, ru: nu weights, shared by the batch */"
DECLARATIONS = {
    "tinympc_set_rollout_metrics": "int tinympc_set_rollout_metrics(tinympc_solver *s, const tinympc_rollout_score *score);  /* on (or re-weighted), and reset */",
    "tinympc_reset_rollout_metrics": "int tinympc_reset_rollout_metrics(tinympc_solver *s);                                   /* zero every row, queued on the stream */",
    "tinympc_clear_rollout_metrics": "int tinympc_clear_rollout_metrics(tinympc_solver *s);                                   /* off: steps run the plain kernel again */",
    "tinympc_get_rollout_metrics": "int tinympc_get_rollout_metrics(tinympc_solver *s, double *out);                        /* 8 x batch, synchronises */",
    "tinympc_get_rollout_metrics_device_ptr": "int tinympc_get_rollout_metrics_device_ptr(tinympc_solver *s, const double **d_rows);    /* ordered behind the handle's stream */",
}


def test_verbs_are_declared_exported_and_typed(pkg):
    header = open(os.path.join(ROOT, "include", "tinympc_hip.h")).read()
    lib, L = pkg.load_library(), pkg._lib
    assert SCORE_TYPE in header
    for name, text in DECLARATIONS.items():
        assert text in header, name
        assert hasattr(lib, name), name
        assert L.SIGNATURES[name][0] is C.c_int
    H, dp = L.Handle, L.c_double_p
    assert L.SIGNATURES["tinympc_set_rollout_metrics"][1] == [H, C.POINTER(L.RolloutScore)]
    assert L.SIGNATURES["tinympc_reset_rollout_metrics"][1] == [H]
    assert L.SIGNATURES["tinympc_clear_rollout_metrics"][1] == [H]
    assert L.SIGNATURES["tinympc_get_rollout_metrics"][1] == [H, dp]
    assert L.SIGNATURES["tinympc_get_rollout_metrics_device_ptr"][1] == [H, C.POINTER(dp)]
    # the struct of the ctypes table is the header's: two pointers and a double, in the header's order
    assert [n for n, _ in L.RolloutScore._fields_] == ["qx", "ru", "settle_tol"]
    assert C.sizeof(L.RolloutScore) == 2 * C.sizeof(C.c_void_p) + C.sizeof(C.c_double)


def test_abi_version_is_unchanged(pkg):
    header = open(os.path.join(ROOT, "include", "tinympc_hip.h")).read()
    assert "#define TINYMPC_ABI_VERSION 1" in header  # (symbols were added, nothing changed)
    assert pkg.abi_version() == 1


def test_null_handle_is_not_initialized(pkg):
    lib, L = pkg.load_library(), pkg._lib
    a = np.ones(8)
    p = a.ctypes.data_as(L.c_double_p)
    score = L.RolloutScore(p, p, 0.5)
    rows = L.c_double_p()
    E = L.ERR_NOT_INITIALIZED
    assert lib.tinympc_set_rollout_metrics(None, C.byref(score)) == E
    assert "not initialized" in L.last_error().lower()
    assert lib.tinympc_set_rollout_metrics(None, None) == E
    assert lib.tinympc_reset_rollout_metrics(None) == E
    assert lib.tinympc_clear_rollout_metrics(None) == E
    assert lib.tinympc_get_rollout_metrics(None, p) == E
    assert (a == 1.0).all()
    assert lib.tinympc_get_rollout_metrics_device_ptr(None, C.byref(rows)) == E
    assert not rows


def test_python_methods_need_setup(pkg):
    s = pkg.TinyMPC()
    for call in (lambda: s.set_rollout_metrics(), lambda: s.set_rollout_metrics(np.ones(2), np.ones(1), 0.1), lambda: s.reset_rollout_metrics(),
                 lambda: s.clear_rollout_metrics(), lambda: s.rollout_metrics(), lambda: s.rollout_metrics(device=True)):
        with pytest.raises(pkg.TinyMPCError) as ei:
            call()
        assert ei.value.code == pkg._lib.ERR_NOT_INITIALIZED


def test_python_methods_check_shapes_before_the_library(pkg, monkeypatch):
    """What the wrapper refuses on its own: weights that are not (nx,) / (nu,), a settle_tol that is no scalar. (_check_setup is stepped
    over: no handle, no device -- a call that got past the wrapper's checks would fail on the missing library handle.)"""
    s = pkg.TinyMPC()
    monkeypatch.setattr(s, "_check_setup", lambda: None)
    s.nx, s.nu, s.N, s.batch = 4, 2, 10, 3
    s.Q, s.R = np.eye(4), np.eye(2)
    E = pkg._lib.ERR_INVALID_INPUT
    bad = [lambda: s.set_rollout_metrics(qx=np.ones(3)), lambda: s.set_rollout_metrics(qx=np.ones((4, 1))), lambda: s.set_rollout_metrics(qx=np.eye(4)),
           lambda: s.set_rollout_metrics(ru=np.ones(4)), lambda: s.set_rollout_metrics(ru=np.ones((2, 3))), lambda: s.set_rollout_metrics(ru=1.0),
           lambda: s.set_rollout_metrics(np.ones(2), np.ones(4)), lambda: s.set_rollout_metrics(settle_tol=np.ones(3))]
    for i, call in enumerate(bad):
        with pytest.raises(pkg.TinyMPCError) as ei:
            call()
        assert ei.value.code == E, i


def test_the_restatement_on_a_case_done_by_hand():
    """Two instances, nx = 2, nu = 1, three steps, numbers whose sums are exact in float64."""
    x = np.zeros((2, 4, 2))
    u = np.zeros((1, 3, 2))
    x[:, :3, 0] = [[1.0, 0.5, 0.0], [2.0, 0.0, 0.25]]          # instance 0: e = x (reference 0)
    u[0, :, 0] = [1.0, -3.0, 0.5]
    x[:, :3, 1] = [[4.0, 4.0, 4.0], [0.0, 0.0, 0.0]]           # instance 1 sits on its reference (4, 0)
    it = np.array([[3, 7], [10, 2], [4, 2]], dtype=np.int32)
    st = np.array([[1, 1], [11, 1], [1, 1]], dtype=np.int32)  # (11: TINYMPC_STATUS_UNSOLVED, a tick that ran out of iterations)
    xr = np.zeros((2, 3, 2)); xr[0, :, 1] = 4.0
    ur = np.zeros((1, 3, 2))
    lo_x, hi_x = np.full((2, 2), -1.5), np.full((2, 2), 1.5)
    lo_u, hi_u = np.full((1, 2), -2.0), np.full((1, 2), 2.0)
    rows = restate(x, u, it, st, xr, ur, (lo_x, hi_x), (lo_u, hi_u), np.array([2.0, 1.0]), np.array([0.5]), 0.375)
    # instance 0: cost 2*1 + 4 + .5*1 | 2*.25 + 0 + .5*9 | 0 + .0625 + .5*.25 ; x breach 2 - 1.5, u breach 3 - 2; settle: step 2 is the last with |e| > .375
    np.testing.assert_array_equal(rows[0], [3, 6.5 + 5.0 + 0.1875, 0.5, 1.0, 17, 10, 1, 2])
    # instance 1: x[0] = 4 breaches the box by 2.5 in every step and never leaves its reference
    np.testing.assert_array_equal(rows[1], [3, 0.0, 2.5, 0.0, 11, 7, 0, 0])
    assert len(NAMES) == 8
    # accumulation: the second half continued from the first is the whole
    half = restate(x[:, :2], u[:, :1], it[:1], st[:1], xr[:, :1], ur[:, :1], (lo_x, hi_x), (lo_u, hi_u), np.array([2.0, 1.0]), np.array([0.5]), 0.375)
    rest = restate(x[:, 1:], u[:, 1:], it[1:], st[1:], xr[:, 1:], ur[:, 1:], (lo_x, hi_x), (lo_u, hi_u), np.array([2.0, 1.0]), np.array([0.5]), 0.375, start=half)
    np.testing.assert_array_equal(rest, rows)
    # families off: the breach slots stay 0; settle_tol <= 0: no settle step
    off = restate(x, u, it, st, xr, ur, None, None, np.array([2.0, 1.0]), np.array([0.5]), 0.0)
    np.testing.assert_array_equal(off[:, [2, 3, 7]], np.zeros((2, 3)))
