"""CPU checks of the rollout noise (tinympc_set_rollout_noise, tinympc_clear_rollout_noise, tinympc_get_rollout_noise,
tinympc_get_plant_state_batch): the numpy restatement of the draw (tests/rollout_noise_cases.py) against the Random123 known answers of
Philox4x32-10, so that the GPU tests compare against something known; the uniforms' ranges; the declarations and the struct stand in the
header verbatim, the symbols are exported and typed in the ctypes table; a NULL handle is refused before anything touches a device; the
Python methods refuse a solver that was never set up and arguments of the wrong shape; the ABI version stays 1."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest
from conftest import ROOT

import rollout_noise_cases as R

NOISE_TYPE = "typedef struct { const double *process, *measurement; int per_instance; unsigned long long seed, first_instance; } tinympc_rollout_noise;"
DECLARATIONS = {
    "tinympc_set_rollout_noise": "int tinympc_set_rollout_noise(tinympc_solver *s, const tinympc_rollout_noise *noise);",
    "tinympc_clear_rollout_noise": "int tinympc_clear_rollout_noise(tinympc_solver *s);",
    "tinympc_get_rollout_noise": "int tinympc_get_rollout_noise(tinympc_solver *s, unsigned long long first_tick, int ticks, double *w_out, double *v_out);",
    "tinympc_get_plant_state_batch": "int tinympc_get_plant_state_batch(tinympc_solver *s, double *x_out);",
}
# Random123's kat_vectors for philox4x32 with 10 rounds: counter, key, output
KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_the_restatement_reproduces_the_known_answers():
    for counter, key, want in KNOWN:
        got = R.philox(counter, key)
        assert tuple(int(w) for w in got) == want, (counter, key)
    # vectorised: the three counters with the third key, element by element what the scalar calls give
    cs = np.array([k[0] for k in KNOWN], dtype=np.uint64).T
    got = R.philox(tuple(cs), KNOWN[2][1])
    for i, (counter, _, _) in enumerate(KNOWN):
        assert [int(w[i]) for w in got] == [int(w) for w in R.philox(counter, KNOWN[2][1])]


def test_the_uniforms_keep_their_ranges_and_the_normal_its_bound():
    zero, ones = [np.uint64(0)] * 4, [np.uint64(0xffffffff)] * 4
    u1, u2 = R.uniforms(zero)
    assert u1 == 2.0 ** -53 and u1 > 0.0 and u2 == 0.0       # log(u1) is finite for the all-zero words
    u1, u2 = R.uniforms(ones)
    assert u1 == 1.0 and u2 == 1.0 - 2.0 ** -53 and u2 < 1.0
    assert np.sqrt(-2.0 * np.log(2.0 ** -53)) <= np.sqrt(106 * np.log(2.0)) <= 8.58
    n = R.normal(1234567890123456789, np.arange(4096, dtype=np.uint64)[:, None], np.arange(7)[None, :], 3, 1)
    assert n.shape == (4096, 7) and np.isfinite(n).all() and np.abs(n).max() <= 8.58
    assert abs(n.mean()) < 0.03 and abs(n.std() - 1.0) < 0.03   # (28,672 draws: three sigma of the mean is 0.018)
    # the counter's words and the key's halves all matter
    base = R.normal(5, 1, 2, 3, 0)
    for other in (R.normal(6, 1, 2, 3, 0), R.normal(5 + (1 << 32), 1, 2, 3, 0), R.normal(5, 2, 2, 3, 0), R.normal(5, 1, 3, 3, 0),
                  R.normal(5, 1, 2, 4, 0), R.normal(5, 1, 2, 3, 1)):
        assert other != base


def test_terms_have_the_disturbances_layout():
    sw = np.array([0.5, 0.0, 2.0])
    w = R.terms(9, sw, 0, 3, 4, 2, 5, first_instance=100)
    assert w.shape == (3, 2, 5) and (w[1] == 0.0).all()
    assert w[2, 1, 3] == 2.0 * R.normal(9, 103, 5, 2, 0)
    per = R.terms(9, np.outer(sw, np.arange(5.0)), 1, 3, 0, 2, 5)
    assert (per[:, :, 0] == 0.0).all() and per[0, 1, 4] == 2.0 * R.normal(9, 4, 1, 0, 1)
    assert (R.terms(9, None, 0, 3, 0, 2, 5) == 0.0).all()


def test_verbs_are_declared_exported_and_typed(pkg):
    header = open(os.path.join(ROOT, "include", "tinympc_hip.h")).read()
    lib, L = pkg.load_library(), pkg._lib
    assert NOISE_TYPE in header
    for name, text in DECLARATIONS.items():
        assert text in header, name
        assert hasattr(lib, name), name
        assert L.SIGNATURES[name][0] is C.c_int
    H, dp = L.Handle, L.c_double_p
    assert L.SIGNATURES["tinympc_set_rollout_noise"][1] == [H, C.POINTER(L.RolloutNoise)]
    assert L.SIGNATURES["tinympc_clear_rollout_noise"][1] == [H]
    assert L.SIGNATURES["tinympc_get_rollout_noise"][1] == [H, C.c_ulonglong, C.c_int, dp, dp]
    assert L.SIGNATURES["tinympc_get_plant_state_batch"][1] == [H, dp]
    # the struct of the ctypes table is the header's: two pointers, an int (padded to 8) and two 64-bit integers, in the header's order
    assert [n for n, _ in L.RolloutNoise._fields_] == ["process", "measurement", "per_instance", "seed", "first_instance"]
    assert [t for _, t in L.RolloutNoise._fields_] == [dp, dp, C.c_int, C.c_ulonglong, C.c_ulonglong]
    assert C.sizeof(L.RolloutNoise) == 2 * C.sizeof(C.c_void_p) + 8 + 2 * 8
    assert L.RolloutNoise.seed.offset == 2 * C.sizeof(C.c_void_p) + 8
    # the existing rollout declarations stand as they were
    assert "typedef struct { double *x_log, *u_log; int *iter_log, *status_log; } tinympc_rollout_logs;   /* any member may be NULL */" in header


def test_abi_version_is_unchanged(pkg):
    header = open(os.path.join(ROOT, "include", "tinympc_hip.h")).read()
    assert "#define TINYMPC_ABI_VERSION 1" in header  # (symbols were added, nothing changed)
    assert pkg.abi_version() == 1


def test_null_handle_is_not_initialized(pkg):
    lib, L = pkg.load_library(), pkg._lib
    a = np.ones(8)
    p = a.ctypes.data_as(L.c_double_p)
    noise = L.RolloutNoise(p, p, 0, 7, 0)
    E = L.ERR_NOT_INITIALIZED
    assert lib.tinympc_set_rollout_noise(None, C.byref(noise)) == E
    assert "not initialized" in L.last_error().lower()
    assert lib.tinympc_set_rollout_noise(None, None) == E
    assert lib.tinympc_clear_rollout_noise(None) == E
    assert lib.tinympc_get_rollout_noise(None, 0, 1, p, p) == E
    assert lib.tinympc_get_plant_state_batch(None, p) == E
    assert (a == 1.0).all()


def test_python_methods_need_setup(pkg):
    s = pkg.TinyMPC()
    for call in (lambda: s.set_rollout_noise(process=np.ones(2)), lambda: s.set_rollout_noise(), lambda: s.clear_rollout_noise(),
                 lambda: s.rollout_noise(0, 1), lambda: s.plant_state()):
        with pytest.raises(pkg.TinyMPCError) as ei:
            call()
        assert ei.value.code == pkg._lib.ERR_NOT_INITIALIZED


def test_python_methods_check_shapes_before_the_library(pkg, monkeypatch):
    """What the wrapper refuses on its own: no scales at all, scales that are neither (nx,) nor (nx, batch), the two families in different
    forms, a seed or a first_instance that is no 64-bit integer, a tick range that is none. (_check_setup is stepped over: no handle, no
    device -- a call that got past the wrapper's checks would fail on the missing library handle.)"""
    s = pkg.TinyMPC()
    monkeypatch.setattr(s, "_check_setup", lambda: None)
    s.nx, s.nu, s.N, s.batch = 4, 2, 10, 3
    E = pkg._lib.ERR_INVALID_INPUT
    bad = [lambda: s.set_rollout_noise(), lambda: s.set_rollout_noise(process=np.ones(3)), lambda: s.set_rollout_noise(process=np.ones((4, 1))),
           lambda: s.set_rollout_noise(process=np.ones((3, 4))), lambda: s.set_rollout_noise(measurement=np.ones((4, 2))),
           lambda: s.set_rollout_noise(measurement=1.0), lambda: s.set_rollout_noise(process=np.ones(4), measurement=np.ones((4, 3))),
           lambda: s.set_rollout_noise(process=np.ones(4), seed=-1), lambda: s.set_rollout_noise(process=np.ones(4), seed=2 ** 64),
           lambda: s.set_rollout_noise(process=np.ones(4), seed=1.5), lambda: s.set_rollout_noise(process=np.ones(4), first_instance=-2),
           lambda: s.set_rollout_noise(process=np.ones(4), first_instance=np.arange(3)),
           lambda: s.rollout_noise(0, 0), lambda: s.rollout_noise(-1, 2), lambda: s.rollout_noise(0.5, 2), lambda: s.rollout_noise(2 ** 32 - 1, 2)]
    for i, call in enumerate(bad):
        with pytest.raises(pkg.TinyMPCError) as ei:
            call()
        assert ei.value.code == E, i
