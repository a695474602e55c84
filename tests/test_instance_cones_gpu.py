"""Per-instance cone slopes of batched handles (tinympc_set_cone_slopes_batch and its _device form) on layout A: every instance solves what
a single-instance handle would solve after set_cone_constraints with the held structure and its own slopes -- checked against the
plain-C oracle per sampled instance (1e-9 on states and controls, equal iteration counts and status, 1e-6 on the four residuals), bit
for bit against a shared-cone twin on layout A where every instance is sent the shared slopes, through the mat-vec path (16 lanes, one
round and two), the reduced path (32 / 64 lanes), a horizon with per-knot references, with and without linear rows, across a sub-range,
the two halves of the mode in either order, warm-started ticks with re-sent slopes and device input; what no kernel carries is refused,
never solved with shared slopes, and invalid input changes nothing. instance_cone_cases.py holds the recipe, the cases and the sample
conditions, which are asserted here on the oracle's own results."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import instance_cone_cases as K
from test_instance_bounds_gpu import _DeviceArrays, _torch_gpu

pytestmark = pytest.mark.gpu

PARITY = ["rocket10", "rocket20", "rocket30", "rocket20-two-rounds", "wide32", "wide64", "rocket10-no-rows"]


def _words(s, cones, linear):
    info = s.jit_info()
    assert ("per-instance-cones" in info) == cones and ("per-instance-linear" in info) == linear, info


# ---- 1. parity with the oracle on layout A, without prepare()

@pytest.mark.parametrize("name", PARITY)
def test_each_instance_matches_the_oracle_with_its_own_slopes(pkg, name):
    prob, batch, settings, x0s, cx, cu = K.data(pkg, name)
    own, shared, other = K.reference(pkg, name)
    if name in K.CONDITIONED:
        K.assert_sample_conditions(name, settings, own, shared, other)
    s = K.solver(pkg, prob, batch, settings)
    s.set_cone_slopes_batch(cx, cu)
    assert s.launch_info()["layout"] == "A"
    _words(s, True, False)
    s.set_x0_batch(x0s)
    s.solve()
    assert s.launch_info()["layout"] == "A"
    K.assert_matches(s, own, name)
    s.reset()


# ---- 2. the shared slopes sent to every instance == the shared cones of a twin on layout A, bit for bit

@pytest.mark.parametrize("name", ["rocket10", "rocket20-two-rounds", "wide32", "rocket10-no-rows"])
def test_shared_slopes_per_instance_are_the_shared_cones_bit_for_bit(pkg, monkeypatch, name):
    prob, batch, settings, x0s, _, _ = K.data(pkg, name)
    shared = [np.repeat(np.asarray(prob.cones[k], dtype=np.float64)[:, None], batch, axis=1) for k in ("cx", "cu")]
    inst = K.solver(pkg, prob, batch, settings)    # (a handle as setup makes it: the mode puts it on layout A)
    monkeypatch.setenv("TINYMPC_LAYOUT", "A")      # the twin: shared cones on layout A, at setup and at every launch
    twin = K.solver(pkg, prob, batch, settings)
    inst.set_cone_slopes_batch(*shared)
    for rnd in range(2):  # a cold start, then a warm start
        for h in (twin, inst):
            h.set_x0_batch(x0s * (1.0 - 0.2 * rnd))
            h.solve()
        K.assert_same_bits(twin, inst)
    assert twin.launch_info()["layout"] == inst.launch_info()["layout"] == "A"
    _words(inst, True, False)
    _words(twin, False, False)
    twin.reset()
    inst.reset()


def test_turning_the_slope_half_on_moves_nothing_in_row_mode(pkg):
    """A handle in row mode (every instance sent the shared row), then the same handle with the slope half turned on with the shared
    slopes: the same kernel, the same bits."""
    prob, batch, settings, x0s, _, _ = K.data(pkg, "rocket10")
    s = K.solver(pkg, prob, batch, settings)
    rep = lambda a: np.repeat(np.asarray(a, dtype=np.float64)[..., None], batch, axis=-1)
    s.set_linear_constraints_batch(rep(prob.linear["Alin_x"]), rep(prob.linear["blin_x"]), None, None)
    s.set_x0_batch(x0s)
    s.solve()
    _words(s, False, True)
    before = K.bits(s)
    s.set_cone_slopes_batch(rep(prob.cones["cx"]), rep(prob.cones["cu"]))
    s.reset_workspace()
    s.solve()
    _words(s, True, True)
    K.assert_same_bits(before, s)
    s.reset()


# ---- 3. a sub-range on the first call: the others keep the shared slopes

def test_a_first_sub_range_leaves_the_others_on_the_shared_slopes(pkg):
    prob, batch, settings, x0s, cx, cu = K.data(pkg, "rocket10")
    lo, hi = 5, 21  # instances 5 .. 20
    s = K.solver(pkg, prob, batch, settings)
    s.set_cone_slopes_batch(cx[:, lo:hi], cu[:, lo:hi], first=lo)
    s.set_x0_batch(x0s)
    s.solve()
    _words(s, True, False)
    expect = {b: K.run(K.oracle(prob, settings, cx[:, b], cu[:, b]) if lo <= b < hi else K.oracle(prob, settings), x0s[:, b])
              for b in (0, lo - 1, lo, hi - 1, hi, batch - 1)}
    K.assert_matches(s, expect, "sub-range")
    s.reset()


# ---- 4. the two halves of the mode

def _own_rows(prob, batch):
    """Every instance's own ground plane: -z <= b_b with b_b in [0, 1]."""
    rng = np.random.default_rng(K.SEED + 1)
    Ax = np.repeat(np.asarray(prob.linear["Alin_x"], dtype=np.float64)[:, :, None], batch, axis=2)
    return Ax, rng.uniform(0.0, 1.0, (1, batch))


def test_the_two_halves_commute_and_end_separately(pkg):
    prob, batch, settings, x0s, cx, cu = K.data(pkg, "rocket10")
    own, shared, _ = K.reference(pkg, "rocket10")
    Ax, bx = _own_rows(prob, batch)
    a, b = K.solver(pkg, prob, batch, settings), K.solver(pkg, prob, batch, settings)
    a.set_linear_constraints_batch(Ax, bx, None, None)  # rows, then slopes
    a.set_cone_slopes_batch(cx, cu)
    b.set_cone_slopes_batch(cx, cu)                      # slopes, then rows
    b.set_linear_constraints_batch(Ax, bx, None, None)
    for h in (a, b):
        _words(h, True, True)
        h.set_x0_batch(x0s)
        h.solve()
        assert h.launch_info()["layout"] == "A"
    K.assert_same_bits(a, b)
    both = {}
    for i in K.sample(batch):  # ... and both are every instance's own: the oracle under instance i's row and slopes
        orc = K.oracle(prob, settings, cx[:, i], cu[:, i])
        orc.set_linear_constraints(Ax[:, :, i], bx[:, i], np.zeros((0, prob.nu)), np.zeros(0))
        orc.update_settings()
        both[i] = K.run(orc, x0s[:, i])
    K.assert_matches(a, both, "both halves")
    # the shared row verb ends the rows' half only: every instance's own slopes on the shared row
    a.set_linear_constraints(**prob.linear)
    _words(a, True, False)
    a.reset_workspace()
    a.solve()
    K.assert_matches(a, own, "slopes kept")
    # the shared cone verb ends the slopes' half only: every instance's own row on the shared slopes
    b.set_cone_constraints(**prob.cones)
    _words(b, False, True)
    b.reset_workspace()
    b.solve()
    rows_only = {}
    for i in K.sample(batch):
        orc = K.oracle(prob, settings)
        orc.set_linear_constraints(Ax[:, :, i], bx[:, i], np.zeros((0, prob.nu)), np.zeros(0))
        orc.update_settings()
        rows_only[i] = K.run(orc, x0s[:, i])
    K.assert_matches(b, rows_only, "rows kept")
    # ... and with both halves off the mode has ended
    a.set_cone_constraints(**prob.cones)
    _words(a, False, False)
    a.reset_workspace()
    a.solve()
    K.assert_matches(a, shared, "mode ended")
    a.reset()
    b.reset()


# ---- 5. warm-started ticks with the slopes re-sent between them; reset_workspace keeps the slopes

def test_slopes_re_sent_between_warm_ticks_keep_the_duals(pkg):
    prob, batch, settings, x0s, cx, cu = K.data(pkg, "rocket10")
    settings = dict(settings, max_iter=40)
    samples = K.sample(batch)
    s = K.solver(pkg, prob, batch, settings)
    orcs = {b: K.oracle(prob, settings) for b in samples}
    for tick in range(3):
        f = 1.1 ** tick
        s.set_cone_slopes_batch(cx * f, cu * f)
        s.mpc_step(x0s * (1.0 - 0.05 * tick))
        expect = {}
        for b in samples:
            K.resend(orcs[b], prob, cx[:, b] * f, cu[:, b] * f)  # (keeps the workspace, the cones' duals included)
            expect[b] = K.run(orcs[b], x0s[:, b] * (1.0 - 0.05 * tick))
        K.assert_matches(s, expect, ("tick", tick))
    s.reset_workspace()  # the ADMM state goes, mode and slopes stay
    _words(s, True, False)
    s.set_x0_batch(x0s)
    s.solve()
    f = 1.1 ** 2
    K.assert_matches(s, {b: K.run(K.oracle(prob, settings, cx[:, b] * f, cu[:, b] * f), x0s[:, b]) for b in samples}, "after reset_workspace")
    s.reset()


# ---- 6. the _device form is the host form, bit for bit

@pytest.mark.parametrize("name", ["rocket10", "wide32"])
def test_device_form_is_the_host_form_bit_for_bit(pkg, name):
    prob, batch, settings, x0s, cx, cu = K.data(pkg, name)
    host, devh = K.solver(pkg, prob, batch, settings), K.solver(pkg, prob, batch, settings)
    host.set_cone_slopes_batch(cx, cu)
    L, dev = pkg.load_library(), _DeviceArrays(pkg)
    assert L.tinympc_set_cone_slopes_batch_device(devh._h, dev.put(cx), cx.shape[0], dev.put(cu), cu.shape[0], 0, batch) == 0
    dev.free()  # (the input has been copied when the verb returns)
    handles = [host, devh]
    torch = _torch_gpu()
    if torch is not None:  # the Python method routes CUDA tensors to the _device form: (count, nc)
        th = K.solver(pkg, prob, batch, settings)
        th.set_cone_slopes_batch(*(torch.from_numpy(np.ascontiguousarray(a.T)).cuda() for a in (cx, cu)))
        handles.append(th)
    for h in handles:
        h.set_x0_batch(x0s)
        h.solve()
        _words(h, True, False)
    for h in handles[1:]:
        K.assert_same_bits(host, h)
    # host memory handed to the _device form
    hx, hu = np.asfortranarray(cx), np.asfortranarray(cu)
    assert L.tinympc_set_cone_slopes_batch_device(devh._h, C.c_void_p(hx.ctypes.data), cx.shape[0], C.c_void_p(hu.ctypes.data), cu.shape[0],
                                                  0, batch) == pkg._lib.ERR_INVALID_INPUT
    for h in handles:
        h.reset()


# ---- 7. invalid input changes nothing

def _raise(pkg, code):
    pkg._lib.check(code)


def test_invalid_arguments_change_nothing(pkg):
    prob, batch, settings, x0s, cx, cu = K.data(pkg, "rocket10")
    s, twin = K.solver(pkg, prob, batch, settings), K.solver(pkg, prob, batch, settings)  # (the twin: the same history without the bad calls)
    for h in (s, twin):
        h.set_cone_slopes_batch(cx, cu)
        h.set_x0_batch(x0s)
        h.solve()
        h.solve()  # (a warm start: the state a bad call must not touch)
    L, lib, dev = pkg.load_library(), pkg._lib, _DeviceArrays(pkg)
    E = lib.ERR_INVALID_INPUT
    ncx, ncu = cx.shape[0], cu.shape[0]

    def bad(which, value):
        a = [cx.copy(), cu.copy()]
        a[which][0, batch - 1] = value
        return a

    calls = []
    for which in (0, 1):
        for value in (np.nan, np.inf, 0.0, -0.3):
            arrays = bad(which, value)
            calls.append(lambda arrays=arrays: s.set_cone_slopes_batch(*arrays))                                       # the host form
            calls.append(lambda arrays=arrays: _raise(pkg, L.tinympc_set_cone_slopes_batch_device(                     # the _device form
                s._h, dev.put(arrays[0]), ncx, dev.put(arrays[1]), ncu, 0, batch)))
    host = [np.asfortranarray(cx), np.asfortranarray(cu)]
    two = np.asfortranarray(np.repeat(cx, 2, axis=0))
    p = [a.ctypes.data_as(lib.c_double_p) for a in host]
    raw = L.tinympc_set_cone_slopes_batch
    calls += [
        lambda: _raise(pkg, raw(s._h, two.ctypes.data_as(lib.c_double_p), 2 * ncx, p[1], ncu, 0, batch)),   # a count that differs from the structure's
        lambda: _raise(pkg, raw(s._h, p[0], ncx, None, 0, 0, batch)),
        lambda: _raise(pkg, raw(s._h, None, ncx, p[1], ncu, 0, batch)),                                    # NULL for a non-empty side
        lambda: _raise(pkg, raw(s._h, p[0], ncx, None, ncu, 0, batch)),
        lambda: _raise(pkg, raw(s._h, p[0], ncx, p[1], ncu, 0, 0)),                                        # an empty range
        lambda: _raise(pkg, raw(s._h, p[0], ncx, p[1], ncu, -1, 2)),                                       # ranges beyond the batch
        lambda: _raise(pkg, raw(s._h, p[0], ncx, p[1], ncu, batch - 1, 2)),
        lambda: _raise(pkg, L.tinympc_set_cone_slopes_batch_device(                                        # host memory handed to the _device form
            s._h, C.c_void_p(host[0].ctypes.data), ncx, C.c_void_p(host[1].ctypes.data), ncu, 0, batch)),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(pkg.TinyMPCError) as ei:
            call()
        assert ei.value.code == E, (i, ei.value)
        _words(s, True, False)
        for h in (s, twin):
            h.solve()
        K.assert_same_bits(twin, s)  # (mode, slopes, flags and ADMM state are what they were: the next solve is the twin's)
    dev.free()
    assert s.settings["en_state_soc"] and s.settings["en_input_soc"]
    s.reset()
    twin.reset()


def test_a_handle_without_cones_is_invalid_and_stays_out_of_the_mode(pkg):
    prob = pkg.problems.quadrotor(20)
    batch = 5
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho, **K.CONV)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    s.set_x0_batch(np.repeat(prob.x0[:, None], batch, axis=1))
    s.solve()
    before = K.bits(s)
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.set_cone_slopes_batch(np.ones((1, batch)), None)
    assert ei.value.code == pkg._lib.ERR_INVALID_INPUT
    _words(s, False, False)
    s.reset_workspace()
    s.solve()
    K.assert_same_bits(before, s)
    s.reset()


def test_single_instance_handle_takes_the_shared_verb(pkg):
    prob, _, settings, x0s, cx, cu = K.data(pkg, "rocket10")
    a, b = K.solver(pkg, prob, 1, settings), K.solver(pkg, prob, 1, settings)
    a.set_cone_constraints(**dict(prob.cones, cx=list(cx[:, 3]), cu=list(cu[:, 3])))
    b.set_cone_slopes_batch(cx[:, 3], cu[:, 3])  # (the arrays may lack the count axis)
    for h in (a, b):
        h.set_x0(x0s[:, 3])
        h.solve()
    K.assert_same_bits(a, b)
    _words(b, False, False)
    with pytest.raises(pkg.TinyMPCError) as ei:
        b.set_cone_slopes_batch(cx[:, 3] * np.nan, cu[:, 3])
    assert ei.value.code == pkg._lib.ERR_INVALID_INPUT
    with pytest.raises(pkg.TinyMPCError) as ei:
        b.set_cone_slopes_batch(cx[:, 3], cu[:, 3], first=1)
    assert ei.value.code == pkg._lib.ERR_INVALID_INPUT
    a.reset()
    b.reset()


# ---- 8. refusals: TINYMPC_ERR_UNSUPPORTED at solve (and at session_begin), never a solve with shared slopes

def _refused(pkg, call):
    with pytest.raises(pkg.TinyMPCError) as ei:
        call()
    assert ei.value.code == pkg._lib.ERR_UNSUPPORTED, ei.value
    assert "set_cone_slopes_batch" in str(ei.value) and "tinympc_set_cone_constraints returns to shared slopes" in str(ei.value), ei.value


def test_refusals_and_the_way_back(pkg):
    prob, batch, settings, x0s, cx, cu = K.data(pkg, "rocket10")
    own, _, _ = K.reference(pkg, "rocket10")
    L, U = pkg.load_library(), pkg._lib.ERR_UNSUPPORTED
    s = K.solver(pkg, prob, batch, settings)
    s.set_cone_slopes_batch(cx, cu)
    s.set_x0_batch(x0s)
    # per-instance rho (the model mode) ...
    s.set_rho_batch(np.full(batch, prob.rho * 1.5))
    _refused(pkg, s.solve)
    assert L.tinympc_session_begin(s._h) == U
    s.clear_model_batch()
    # ... per-instance models ...
    s.set_model_batch(*(np.repeat(m[:, :, None], batch, axis=2) for m in (prob.A, prob.B, prob.Q, prob.R)), fdyn=np.repeat(prob.fdyn[:, None], batch, axis=1))
    _refused(pkg, s.solve)
    assert L.tinympc_session_begin(s._h) == U
    s.clear_model_batch()
    # ... adaptive rho
    s.update_settings(adaptive_rho=True)
    _refused(pkg, s.solve)
    assert L.tinympc_session_begin(s._h) == U
    s.update_settings(adaptive_rho=False)
    assert L.tinympc_session_begin(s._h) == U  # (the mode itself has no session)
    # every way back taken: the mode solves, with its own slopes
    s.reset_workspace()
    s.solve()
    K.assert_matches(s, own, "after the refusals")
    s.reset()


def test_large_systems_are_refused(pkg):
    P = pkg.problems
    rng = np.random.default_rng(5)
    nx, nu, batch = 60, 12, 3
    prob = P.Problem("large", np.eye(nx) + 0.02 * rng.standard_normal((nx, nx)), 0.1 * rng.standard_normal((nx, nu)), np.eye(nx), np.eye(nu), 8, 1.0,
                     rng.standard_normal(nx))
    prob.cones = dict(Acx=[0], qcx=[3], cx=[0.5], Acu=[0], qcu=[3], cu=[0.25])
    s = K.solver(pkg, prob, batch, K.FORCED)
    s.set_cone_slopes_batch(np.full((1, batch), 0.7), np.full((1, batch), 0.3))
    s.set_x0_batch(np.repeat(prob.x0[:, None], batch, axis=1))
    _refused(pkg, s.solve)
    s.set_cone_constraints(**prob.cones)  # the way back
    s.solve()
    s.reset()
