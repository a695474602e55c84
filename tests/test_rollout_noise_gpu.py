"""Rollout noise (tinympc_set_rollout_noise and its verbs; the noisy variants of k_plant_step, k_rollout_noise): the draws against the numpy
restatement (tests/rollout_noise_cases.py) and bit-equal across layouts; a process-noise rollout is replayed bit for bit by a noise-free
handle given the regenerated terms as its disturbance; 4 ticks = 2 + 2 = four solve + plant_step ticks with an external disturbance
present, in the order (acc + w) + noise; measurement noise reaches the next solve and nothing else (a noise-free handle driven from the
host, tick by tick, reproduces every logged control and every true state; the metrics are the restatement of the true-state logs);
first_instance, per-instance scales, the true state's bookkeeping, the refusals and the seeds.

Shapes: those of tests/test_rollout_gpu.py -- its eight CASES (16 lanes at operand lengths 8 / 12 / 16, tracks, per-instance models, the
families, 32 and 64 lanes, the workgroup form), batches 37 and 300 (5 for the 84-row system), 5 ticks. One set of runs per (case, batch)
is computed once and shared by the tests that read it.

Tolerances: bit equality wherever two runs of this library are compared, and against float64 operations numpy performs one at a time.
The one bound is on the draws against the restatement, |device - numpy| <= 1e-13 x scale, derived and not measured: the draw is
sqrt(-2 log u1) cos(2 pi u2) with u1, u2 exact; the device's log and cos are within a few ulp (the ROCm device library documents 1 and 2
ulp), its sqrt is correctly rounded, |n| <= 8.58 with ulp(8.58) = 1.8e-15, so a draw is within about 1e-14 of the exact value; ten times
that is left for the host's libm. A wrong Philox word moves a draw by O(1). (The refusal of a step whose tick would reach 2^32 cannot be
reached here: no verb sets the tick, and 2^32 steps are not a test.)"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import rollout_noise_cases as R
from rollout_metrics_cases import NAMES, as_rows, restate
from test_rollout_gpu import PARAMS, SETTINGS, TICKS, Setup, _assert_logs_equal, _assert_unchanged, _final, _layout_env, _quad, _snapshot, _x0s
from test_rollout_metrics_gpu import SETTLE_TOL, _operands, _weights

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15  # (both halves of the key are in use)
DRAW_TOL = 1e-13


def _scales(nx):
    """Process and measurement standard deviations per row: the disturbance's size of tests/test_rollout_gpu.py, the reference example's
    0.01 for the sensor; rows differ, so a row taken for another shows."""
    return 1e-3 * (1.0 + np.arange(nx) % 3), 0.01 * (1.0 + np.arange(nx) % 2)


def _assert_equal_dicts(a, b, tag=""):
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg="%s %s" % (tag, k))


def _advance(su, h):
    if su.case.tracks:
        h.advance_ref_step(1)


_RUNS = {}


def _run(pkg, name, batch):
    key = (name, batch)
    if key in _RUNS:
        return _RUNS[key]
    su = Setup(pkg, name, batch)
    prob = su.prob
    nx = prob.nx
    sw, sv = _scales(nx)
    out = dict(su=su, sw=sw, sv=sv)
    with _layout_env(su.case.layout_env):
        # a: process and measurement noise, scored, all logs; a2: the same again (the seed is all there is); a3: another seed
        a, a2, a3 = su.handle(), su.handle(), su.handle()
        for h, seed in ((a, SEED), (a2, SEED), (a3, SEED + 1)):
            h.set_rollout_metrics(settle_tol=SETTLE_TOL)
            h.set_rollout_noise(process=sw, measurement=sv, seed=seed)
        out["layout"] = a.launch_info()["layout"]
        out["a_logs"], out["a2_logs"], out["a3_logs"] = a.rollout(TICKS), a2.rollout(TICKS), a3.rollout(TICKS)
        out["a_rows"] = as_rows(a.rollout_metrics())
        out["a_replay"] = a.rollout_noise(0, TICKS)
        out["a_state"] = a.plant_state()
        a.solve()
        out["a_final"] = _final(a)
        # h: no noise, driven from the host with a's logs and replay, tick by tick
        h = su.handle(auto_advance=False)
        x, w, v = out["a_logs"]["x"], out["a_replay"]["w"], out["a_replay"]["v"]
        hu = np.zeros((prob.nu, TICKS, batch))
        hi, hs = np.zeros((TICKS, batch), dtype=np.int32), np.zeros((TICKS, batch), dtype=np.int32)
        hx = np.zeros((nx, TICKS + 1, batch))
        hx[:, 0, :] = x[:, 0, :]
        for t in range(TICKS):
            h.set_x0_batch(x[:, t, :] + v[:, t - 1, :] if t else x[:, 0, :])  # the measurement: one add
            h.solve()
            st = h.get_stats_batch()
            hu[:, t, :], hi[t], hs[t] = h.get_first_controls_batch(), st["iter"], st["status"]
            h.set_x0_batch(x[:, t, :])  # the true state
            h.plant_step(w[:, t, :])
            hx[:, t + 1, :] = h.plant_state()
            _advance(su, h)
        h.set_x0_batch(x[:, TICKS, :] + v[:, TICKS - 1, :])  # what a's x0 holds after the rollout, if the next solve is to agree
        h.solve()
        out["h"] = dict(x=hx, u=hu, iter=hi, status=hs)
        out["h_final"] = _final(h)
        # b: process noise alone; c: no noise, b's regenerated terms as the disturbance
        b, c = su.handle(), su.handle()
        for g in (b, c):
            g.set_rollout_metrics(settle_tol=SETTLE_TOL)
        b.set_rollout_noise(process=sw, seed=SEED)
        out["b_logs"] = b.rollout(TICKS)
        out["b_replay"] = b.rollout_noise(0, TICKS)
        out["c_logs"] = c.rollout(TICKS, disturbance=out["b_replay"]["w"])
        for tag, g in (("b", b), ("c", c)):
            out[tag + "_rows"] = as_rows(g.rollout_metrics())
            out[tag + "_state"] = g.plant_state()
            g.solve()
            out[tag + "_final"] = _final(g)
        # d: 4 ticks at once; e: 2 + 2; f: four solve + plant_step ticks -- both families, scored, an external disturbance present
        d, e, f = su.handle(), su.handle(), su.handle(auto_advance=False)
        for g in (d, e, f):
            g.set_rollout_metrics(settle_tol=SETTLE_TOL)
            g.set_rollout_noise(process=sw, measurement=sv, seed=SEED)
        w4 = np.asfortranarray(su.w[:, :4, :])
        out["d_logs"] = d.rollout(4, disturbance=w4)
        e1 = e.rollout(2, disturbance=np.asfortranarray(w4[:, :2, :]))
        e2 = e.rollout(2, disturbance=np.asfortranarray(w4[:, 2:, :]))
        out["e_logs"] = dict(x=np.concatenate([e1["x"][:, :2], e2["x"]], axis=1), u=np.concatenate([e1["u"], e2["u"]], axis=1),
                             iter=np.concatenate([e1["iter"], e2["iter"]]), status=np.concatenate([e1["status"], e2["status"]]))
        out["e_seam"] = (e1["x"][:, 2, :], e2["x"][:, 0, :])
        fu = np.zeros((prob.nu, 4, batch))
        for t in range(4):
            f.solve()
            fu[:, t, :] = f.get_first_controls_batch()
            f.plant_step(w4[:, t, :])
            _advance(su, f)
        out["f_u"] = fu
        out["d_replay"] = d.rollout_noise(0, 4)
        for tag, g in (("d", d), ("e", e), ("f", f)):
            out[tag + "_rows"] = as_rows(g.rollout_metrics())
            out[tag + "_state"] = g.plant_state()
            g.solve()
            out[tag + "_final"] = _final(g)
        # k: the order (acc + w) + noise -- no noise, d's measurements and true states from the host, the external disturbance through the
        # plant step, the regenerated process term added here
        k = su.handle(auto_advance=False)
        x, w, v = out["d_logs"]["x"], out["d_replay"]["w"], out["d_replay"]["v"]
        kx = np.zeros((nx, 5, batch))
        kx[:, 0, :] = x[:, 0, :]
        for t in range(4):
            k.set_x0_batch(x[:, t, :] + v[:, t - 1, :] if t else x[:, 0, :])
            k.solve()
            k.set_x0_batch(x[:, t, :])
            k.plant_step(w4[:, t, :])
            kx[:, t + 1, :] = k.plant_state() + w[:, t, :]
            _advance(su, k)
        out["k_x"] = kx
        # z: scales per instance, zeros for the even instances; p: no noise at all
        z, p = su.handle(), su.handle()
        mask = (np.arange(batch) % 2).astype(np.float64)
        z.set_rollout_noise(process=sw[:, None] * mask[None, :], measurement=sv[:, None] * mask[None, :], seed=SEED)
        out["z_logs"] = z.rollout(TICKS, disturbance=su.w)
        out["z_replay"] = z.rollout_noise(0, TICKS)
        out["p_logs"] = p.rollout(TICKS, disturbance=su.w)
        # q: noise on and off again: the plain kernel, from the state x0 holds
        q = su.handle()
        q.set_rollout_noise(process=sw, measurement=sv, seed=SEED)
        q.clear_rollout_noise()
        out["q_logs"] = q.rollout(TICKS, disturbance=su.w)
        for g in (a, a2, a3, h, b, c, d, e, f, k, z, p, q):
            g.reset()
    _RUNS[key] = out
    return out


# ------------------------------------------------------------------------------------------------ 1. the draws
@pytest.mark.parametrize("name,batch", PARAMS)
def test_draws_match_the_restatement(pkg, name, batch):
    run = _run(pkg, name, batch)
    nx = run["su"].prob.nx
    worst = 0.0
    for key, scales, stream in (("w", run["sw"], 0), ("v", run["sv"], 1)):
        dev = run["a_replay"][key]
        ref = R.terms(SEED, scales, stream, nx, 0, TICKS, batch)
        assert dev.shape == ref.shape == (nx, TICKS, batch)
        err = np.abs(dev - ref) / scales[:, None, None]
        worst = max(worst, float(err.max()))
        assert (err <= DRAW_TOL).all(), (key, float(err.max()))
        assert (np.abs(dev) <= 8.58 * scales[:, None, None]).all() and (dev != 0.0).mean() > 0.99
    print("draws %s batch %d (layout %s): worst |device - numpy| / scale = %.3e (bound %.0e)" % (name, batch, run["layout"], worst, DRAW_TOL))
    # the zero columns of per-instance scales are zeros, the others the shared draws: the same counters
    np.testing.assert_array_equal(run["z_replay"]["w"][:, :, 0::2], 0.0)
    np.testing.assert_array_equal(run["z_replay"]["w"][:, :, 1::2], run["a_replay"]["w"][:, :, 1::2])
    np.testing.assert_array_equal(run["z_replay"]["v"][:, :, 1::2], run["a_replay"]["v"][:, :, 1::2])
    # a family that is off yields zeros
    np.testing.assert_array_equal(run["b_replay"]["v"], 0.0)
    np.testing.assert_array_equal(run["b_replay"]["w"], run["a_replay"]["w"])


@pytest.mark.parametrize("batch", [37, 300])
def test_draws_do_not_depend_on_the_layout(pkg, batch):
    d, m = _run(pkg, "quadrotor20_d", batch), _run(pkg, "quadrotor20_models", batch)
    assert d["layout"] == "D" and m["layout"] != "D"
    _assert_equal_dicts(d["a_replay"], m["a_replay"])


# ------------------------------------------------------------------------------------------------ 2. process noise is replayable
@pytest.mark.parametrize("name,batch", PARAMS)
def test_process_noise_is_replayed_by_its_regenerated_terms(pkg, name, batch):
    run = _run(pkg, name, batch)
    _assert_logs_equal(run["b_logs"], run["c_logs"])
    np.testing.assert_array_equal(run["b_state"], run["c_state"])
    np.testing.assert_array_equal(run["b_state"], run["b_logs"]["x"][:, TICKS, :])  # (without measurement noise x0 is the true state)
    _assert_equal_dicts(run["b_final"], run["c_final"])
    np.testing.assert_array_equal(run["b_rows"], run["c_rows"])
    assert np.abs(run["b_logs"]["x"] - run["p_logs"]["x"]).max() > 1e-4  # (the noise is one)


# ------------------------------------------------------------------------------------------------ 3. accumulation and order
@pytest.mark.parametrize("name,batch", PARAMS)
def test_ticks_accumulate_and_the_noise_comes_behind_the_disturbance(pkg, name, batch):
    run = _run(pkg, name, batch)
    _assert_logs_equal(run["d_logs"], run["e_logs"])
    np.testing.assert_array_equal(run["e_seam"][0], run["e_seam"][1])  # (the second half starts from the first half's true state)
    np.testing.assert_array_equal(run["d_logs"]["u"], run["f_u"])
    for other in ("e", "f"):
        np.testing.assert_array_equal(run["d_state"], run[other + "_state"], err_msg=other)
        np.testing.assert_array_equal(run["d_rows"], run[other + "_rows"], err_msg=other)
        _assert_equal_dicts(run["d_final"], run[other + "_final"], other)
    np.testing.assert_array_equal(run["d_state"], run["d_logs"]["x"][:, 4, :])
    np.testing.assert_array_equal(run["d_rows"][:, 0], np.full(batch, 4))
    # (acc + w) + noise: the plain step with the external disturbance, then the regenerated term
    np.testing.assert_array_equal(run["d_logs"]["x"], run["k_x"])
    # the ticks of the replay are the handle's: the first four draws of the five-tick run with this seed
    np.testing.assert_array_equal(run["d_replay"]["w"], run["a_replay"]["w"][:, :4, :])


# ------------------------------------------------------------------------------------------------ 4. measurement noise
@pytest.mark.parametrize("name,batch", PARAMS)
def test_measurement_noise_reaches_the_next_solve_and_nothing_else(pkg, name, batch):
    run = _run(pkg, name, batch)
    su, logs, h = run["su"], run["a_logs"], run["h"]
    # every logged control, iteration count and status is the solve of x[t] + v[t-1]; every true state the plant step of x[t] with w[t]
    _assert_logs_equal(logs, h)
    np.testing.assert_array_equal(logs["x"][:, 0, :], su.x0s)
    np.testing.assert_array_equal(run["a_state"], logs["x"][:, TICKS, :])
    # x0 afterwards is x[T] + v[T-1]: one more solve on both
    _assert_equal_dicts(run["a_final"], run["h_final"])
    # the measurement matters (the controls of the process-only run differ) and the metrics score the true state
    assert (logs["u"][:, 1:, :] != run["b_logs"]["u"][:, 1:, :]).any()
    np.testing.assert_array_equal(logs["u"][:, 0, :], run["b_logs"]["u"][:, 0, :])  # (the first tick's measurement is x0 itself)
    xr, ur, xb, ub = _operands(su, TICKS, batch)
    qx, ru = _weights(su.prob)
    want = restate(logs["x"], logs["u"], logs["iter"], logs["status"], xr, ur, xb, ub, qx, ru, SETTLE_TOL)
    for i, k in enumerate(NAMES):
        np.testing.assert_array_equal(run["a_rows"][:, i], want[:, i], err_msg=k)


# ------------------------------------------------------------------------------------------------ 5. first_instance
def test_a_shard_draws_what_its_instances_draw_unsharded(pkg):
    whole = _run(pkg, "quadrotor20_d", 300)["a_replay"]
    prob, s = _quad(pkg, 37)
    sw, sv = _scales(prob.nx)
    s.set_rollout_noise(process=sw, measurement=sv, seed=SEED, first_instance=100)
    part = s.rollout_noise(0, TICKS)
    for k in ("w", "v"):
        np.testing.assert_array_equal(part[k], whole[k][:, :, 100:137], err_msg=k)
    # ... and in the steps themselves: process noise from first_instance 100 is the disturbance of instances 100 .. 136
    s.set_rollout_noise(process=sw, seed=SEED, first_instance=100)
    _, t = _quad(pkg, 37)
    _assert_logs_equal(s.rollout(TICKS), t.rollout(TICKS, disturbance=np.asfortranarray(whole["w"][:, :, 100:137])))
    # ticks further on: any range can be regenerated
    later = s.rollout_noise(3, 2)["w"]
    np.testing.assert_array_equal(later, whole["w"][:, 3:5, 100:137])
    s.reset()
    t.reset()


# ------------------------------------------------------------------------------------------------ 6. per-instance scales
@pytest.mark.parametrize("name,batch", PARAMS)
def test_instances_with_zero_scales_log_what_a_handle_without_noise_logs(pkg, name, batch):
    run = _run(pkg, name, batch)
    z, p = run["z_logs"], run["p_logs"]
    for k in ("x", "u", "iter", "status"):
        np.testing.assert_array_equal(z[k][..., 0::2], p[k][..., 0::2], err_msg=k)
    assert (z["x"][..., 1::2] != p["x"][..., 1::2]).any() and (z["u"][..., 1::2] != p["u"][..., 1::2]).any()
    # ... and a handle that turned the noise on and off again logs what one that never did logs
    _assert_logs_equal(run["q_logs"], p)


# ------------------------------------------------------------------------------------------------ 7. the true state's bookkeeping
@pytest.mark.parametrize("batch", [37, 300])
def test_writes_of_x0_restart_the_true_state_and_clear_continues_from_it(pkg, batch):
    prob, s = _quad(pkg, batch)
    sw, sv = _scales(prob.nx)
    x0s = _x0s(prob, batch)
    np.testing.assert_array_equal(s.plant_state(), x0s)  # (no noise: x0 itself)
    s.set_rollout_noise(measurement=sv, seed=SEED)
    np.testing.assert_array_equal(s.plant_state(), x0s)  # (just turned on: the true state is what x0 holds)
    first = s.rollout(2)
    assert (s.plant_state() == first["x"][:, 2, :]).all()
    # the whole batch from outside: the true state restarts there
    fresh = _x0s(prob, batch, seed=11)
    s.set_x0_batch(fresh)
    np.testing.assert_array_equal(s.plant_state(), fresh)
    second = s.rollout(2)
    np.testing.assert_array_equal(second["x"][:, 0, :], fresh)
    # a range from outside: those instances restart, the others keep their true state (not their measurement)
    part = _x0s(prob, 5, seed=12)
    s.set_x0_batch(part, first=3)
    want = second["x"][:, 2, :].copy()
    want[:, 3:8] = part
    np.testing.assert_array_equal(s.plant_state(), want)
    third = s.rollout(2)
    np.testing.assert_array_equal(third["x"][:, 0, :], want)
    # mpc_step brings its own x0
    own = _x0s(prob, batch, seed=13)
    s.mpc_step(own)
    np.testing.assert_array_equal(s.plant_state(), own)
    # the ticks went on over all of this: 6 steps so far
    fourth = s.rollout(2)
    v = s.rollout_noise(6, 2)["v"]
    assert np.abs(v - R.terms(SEED, sv, 1, prob.nx, 6, 2, batch)).max() <= DRAW_TOL * sv.max()
    # clear: x0 is the true state as read before it, and the loop goes on from there on the plain kernel
    truth = s.plant_state()
    np.testing.assert_array_equal(truth, fourth["x"][:, 2, :])
    s.clear_rollout_noise()
    np.testing.assert_array_equal(s.plant_state(), truth)
    _, twin = _quad(pkg, batch)
    for hdl in (s, twin):
        hdl.reset_workspace()
    twin.set_x0_batch(truth)
    _assert_logs_equal(s.rollout(2), twin.rollout(2))
    # measurement noise replaced by process noise alone: the same hand-over
    s.set_rollout_noise(measurement=sv, seed=SEED)
    s.rollout(2)
    truth = s.plant_state()
    s.set_rollout_noise(process=sw, seed=SEED)
    np.testing.assert_array_equal(s.plant_state(), truth)
    np.testing.assert_array_equal(s.rollout(1)["x"][:, 0, :], truth)
    s.reset()
    twin.reset()


# ------------------------------------------------------------------------------------------------ 8. refusals change nothing
def test_refusals_change_nothing(pkg):
    batch = 37
    lib, L = pkg.load_library(), pkg._lib
    prob, s = _quad(pkg, batch)
    _, twin = _quad(pkg, batch)
    nx = prob.nx
    dp = lambda a: a.ctypes.data_as(L.c_double_p)
    sw, sv = _scales(nx)
    sw, sv = np.ascontiguousarray(sw), np.ascontiguousarray(sv)
    out_w, out_v = np.full((nx, TICKS, batch), -7.0, order="F"), np.full((nx, TICKS, batch), -7.0, order="F")
    for h in (s, twin):
        h.solve()
    snap = _snapshot(s)
    state = s.plant_state()
    E = L.ERR_INVALID_INPUT
    # while the noise is off: get and clear
    assert lib.tinympc_get_rollout_noise(s._h, 0, TICKS, dp(out_w), dp(out_v)) == E
    assert "noise is off" in L.last_error()
    assert lib.tinympc_clear_rollout_noise(s._h) == E
    assert lib.tinympc_get_plant_state_batch(s._h, None) == E
    # a NULL struct, both arrays NULL, scales that are negative or not finite (in either array, per instance too), an index beyond 2^32
    neg, nan, inf = sw.copy(), sv.copy(), sw.copy()
    neg[nx - 1], nan[2], inf[0] = -1e-9, np.nan, np.inf
    per = np.asfortranarray(np.repeat(sv[:, None], batch, axis=1))
    per[nx - 1, batch - 1] = -1.0
    bad = [None, L.RolloutNoise(None, None, 0, 1, 0), L.RolloutNoise(dp(neg), None, 0, 1, 0), L.RolloutNoise(dp(sw), dp(nan), 0, 1, 0),
           L.RolloutNoise(dp(inf), dp(sv), 0, 1, 0), L.RolloutNoise(None, dp(per), 1, 1, 0), L.RolloutNoise(dp(sw), dp(sv), 0, 1, 2 ** 32 - batch + 1),
           L.RolloutNoise(dp(sw), None, 0, 1, 2 ** 64 - 1)]

    def refused(tag):
        for i, n in enumerate(bad):
            assert lib.tinympc_set_rollout_noise(s._h, C.byref(n) if n is not None else None) == E, (tag, i)

    refused("off")
    assert lib.tinympc_get_rollout_noise(s._h, 0, TICKS, dp(out_w), dp(out_v)) == E  # (still off)
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.set_rollout_noise(process=-sw)
    assert ei.value.code == E
    assert (out_w == -7.0).all() and (out_v == -7.0).all()
    _assert_unchanged(s, snap, "off")
    np.testing.assert_array_equal(s.plant_state(), state)
    # the largest first_instance that fits is taken
    s.set_rollout_noise(process=sw, seed=SEED, first_instance=2 ** 32 - batch)
    top = s.rollout_noise(0, 1)["w"]
    assert np.abs(top - R.terms(SEED, sw, 0, nx, 0, 1, batch, first_instance=2 ** 32 - batch)).max() <= DRAW_TOL * sw.max()
    s.clear_rollout_noise()
    # on: a refused call leaves the scales, the seed and the tick as they are
    for h in (s, twin):
        h.set_rollout_noise(process=sw, measurement=sv, seed=SEED)
        h.rollout(2, log=())
    before = s.rollout_noise(0, TICKS)
    refused("on")
    for ticks in (0, -3):
        assert lib.tinympc_get_rollout_noise(s._h, 0, ticks, dp(out_w), dp(out_v)) == E, ticks
    assert lib.tinympc_get_rollout_noise(s._h, 2 ** 32 - 1, 2, dp(out_w), dp(out_v)) == E
    assert lib.tinympc_get_rollout_noise(s._h, 2 ** 64 - 1, 2, dp(out_w), dp(out_v)) == E
    assert lib.tinympc_get_plant_state_batch(s._h, None) == E
    assert (out_w == -7.0).all() and (out_v == -7.0).all()
    assert lib.tinympc_get_rollout_noise(s._h, 0, TICKS, None, None) == 0  # (either output may be NULL: nothing to do)
    _assert_equal_dicts(s.rollout_noise(0, TICKS), before)
    np.testing.assert_array_equal(s.plant_state(), twin.plant_state())
    _assert_logs_equal(s.rollout(2), twin.rollout(2))  # (the same tick, the same scales, the same true state)
    s.solve()
    twin.solve()
    a, b = _snapshot(s), _snapshot(twin)
    _assert_equal_dicts(a[0], b[0])
    s.reset()
    twin.reset()


def test_single_instance_handles_and_sessions_are_refused(pkg):
    lib, L = pkg.load_library(), pkg._lib
    prob = pkg.problems.cartpole(10, True)
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, rho=prob.rho, **SETTINGS)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    s.set_x0(prob.x0)
    s.solve()
    before = (s.get_solution(), s.get_stats())
    sw = np.ones(prob.nx)
    dp = lambda a: a.ctypes.data_as(L.c_double_p)
    noise = L.RolloutNoise(dp(sw), dp(sw), 0, 1, 0)
    out = np.full((prob.nx, 1, 1), -7.0)
    calls = (lambda: lib.tinympc_set_rollout_noise(s._h, C.byref(noise)), lambda: lib.tinympc_clear_rollout_noise(s._h),
             lambda: lib.tinympc_get_rollout_noise(s._h, 0, 1, dp(out), dp(out)), lambda: lib.tinympc_get_plant_state_batch(s._h, dp(out)))
    for i, call in enumerate(calls):
        assert call() == L.ERR_UNSUPPORTED, i
        assert "batched handles outside a session only" in L.last_error(), i
    after = (s.get_solution(), s.get_stats())
    np.testing.assert_array_equal(before[0]["controls"], after[0]["controls"])
    assert before[1]["iter"] == after[1]["iter"]
    s.session_begin()
    u_in = s.session_step(prob.x0)
    for i, call in enumerate(calls):
        assert call() == L.ERR_UNSUPPORTED, i
    np.testing.assert_array_equal(s.session_step(prob.x0).shape, u_in.shape)  # (the session is still open and answers)
    s.session_end()
    assert (out == -7.0).all()
    s.reset()


# ------------------------------------------------------------------------------------------------ 9. seeds
@pytest.mark.parametrize("name,batch", PARAMS)
def test_the_seed_is_all_there_is(pkg, name, batch):
    run = _run(pkg, name, batch)
    _assert_logs_equal(run["a_logs"], run["a2_logs"])
    assert (run["a_logs"]["x"][:, 1:, :] != run["a3_logs"]["x"][:, 1:, :]).mean() > 0.99
    np.testing.assert_array_equal(run["a_logs"]["x"][:, 0, :], run["a3_logs"]["x"][:, 0, :])
