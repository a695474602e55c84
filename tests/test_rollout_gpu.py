"""Closed-loop rollout on the device (tinympc_rollout_batch and its _device form, tinympc_plant_step_batch, tinympc_set_plant_batch,
tinympc_clear_plant_batch): `ticks` ticks queued in one call are, bit for bit, the same ticks issued one by one (solve + plant step, with
a read-back after every tick); the plant step is x+ = A_b x + B_b u + f_b + w against numpy; every logged tick is the oracle's solve of the
logged state; disturbance and logs from device memory, NULL log members, the plant override and the refusals.

Shapes: batches 37 and 300 (no multiple of a wavefront's instances; 300 is beyond the zero-copy tick), 5 ticks; one case per kernel
family the plant step sits behind -- 16 lanes on the default layout and on layout D, tracks with auto-advance after prepare(),
per-instance models, the cone / linear families, 32 and 64 lanes, and a layout-M system with nx > 64 (the workgroup form of the plant
step). One rollout per (case, batch) is computed once and shared by the tests that read it.

Tolerances: bit equality wherever two runs of this library are compared; rtol 1e-12 / atol 1e-15 for the plant step against numpy (whose
summation order differs: tests/test_session_gpu.py gives its plant step the same); TOL = 1e-9 relative against the oracle, the project's."""
from __future__ import annotations

import contextlib
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest
from conftest import rel_err

import pyoracle as O
from test_hip_families import make as _make_families
from test_instance_bounds_gpu import _DeviceArrays, _torch_gpu
from test_instance_models_gpu import _models, _set_models
from test_instance_refs_gpu import _wide
from test_large_systems_gpu import _system
from test_ref_track_gpu import _tracks, _windows

pytestmark = pytest.mark.gpu

TOL = 1e-9
TICKS = 5
SETTINGS = dict(max_iter=100, abs_pri_tol=1e-4, abs_dua_tol=1e-4)
ROCKET_SETTINGS = dict(max_iter=100, abs_pri_tol=2e-3, abs_dua_tol=1e-4)
TRACK_T = 8  # shorter than N + TICKS: the held last knot is crossed


@dataclasses.dataclass
class Case:
    problem: object                  # P -> Problem
    settings: dict = dataclasses.field(default_factory=lambda: dict(SETTINGS))
    layout_env: str | None = None    # TINYMPC_LAYOUT while the handles are set up and run
    tracks: bool = False
    models: bool = False
    families: bool = False
    layout: str | None = None        # what launch_info() must report
    batches: tuple = (37, 300)


class _Pkg:
    """What test_large_systems_gpu._system wants of the package: its problems."""

    def __init__(self, problems):
        self.problems = problems


CASES = {
    "cartpole10": Case(lambda P: P.cartpole(10, True)),
    "quadrotor20_d": Case(lambda P: P.quadrotor(20), layout_env="D", layout="D"),
    "quadrotor20_tracks": Case(lambda P: P.quadrotor(20), layout_env="D", tracks=True, layout="D"),
    "quadrotor20_models": Case(lambda P: P.quadrotor(20), models=True),
    "rocket10_families": Case(lambda P: P.rocket(10, with_linear=True), settings=dict(ROCKET_SETTINGS), families=True),
    "wide32": Case(lambda P: _wide(P, 24, 8, 10)),
    "wide64": Case(lambda P: _wide(P, 48, 16, 6)),
    "large70_m": Case(lambda P: _system(_Pkg(P), 70, 14, 10, 84, True), layout="M", batches=(5,)),
}
PARAMS = [(name, b) for name, c in CASES.items() for b in c.batches]


@contextlib.contextmanager
def _layout_env(value):
    old = os.environ.get("TINYMPC_LAYOUT")
    if value is not None:
        os.environ["TINYMPC_LAYOUT"] = value
    try:
        yield
    finally:
        if value is not None:
            if old is None:
                del os.environ["TINYMPC_LAYOUT"]
            else:
                os.environ["TINYMPC_LAYOUT"] = old


def _x0s(prob, batch, seed=2):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(prob.x0[:, None] + 0.1 * rng.standard_normal((prob.nx, batch)) * np.maximum(np.abs(prob.x0[:, None]), 0.5))


def _disturbance(prob, batch, ticks=TICKS, seed=5):
    return np.asfortranarray(1e-3 * np.random.default_rng(seed).standard_normal((prob.nx, ticks, batch)))


def _sample(batch):
    return sorted({0, 1, batch // 2, batch - 2, batch - 1})


class Setup:
    """Everything a case's handles share: the problem, x0, the disturbance, tracks / models where the case has them."""

    def __init__(self, pkg, name, batch):
        self.pkg, self.name, self.batch = pkg, name, batch
        self.case = CASES[name]
        self.prob = self.case.problem(pkg.problems)
        self.x0s = _x0s(self.prob, batch)
        self.w = _disturbance(self.prob, batch)
        self.X = self.U = self.M = None
        if self.case.tracks:
            self.X, self.U = _tracks(self.prob, batch, TRACK_T, TRACK_T)
        if self.case.models:
            self.M = _models(self.prob, batch, seed=7, fdyn=True)

    def handle(self, auto_advance=True):
        pkg, prob, c = self.pkg, self.prob, self.case
        if c.families:
            s = _make_families(pkg, prob, c.settings, batch=self.batch)
        else:
            s = pkg.TinyMPC()
            s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=self.batch, rho=prob.rho, fdyn=prob.fdyn, **c.settings)
            if prob.has_bounds():
                s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
            if prob.x_ref is not None:
                s.set_x_ref(prob.x_ref)
                s.set_u_ref(prob.u_ref)
        if c.models:
            _set_models(s, self.M)
        if c.tracks:
            s.set_x_ref_track_batch(self.X)
            s.set_u_ref_track_batch(self.U)
            s.prepare()
            if auto_advance:
                s.set_ref_auto_advance(1)
        s.set_x0_batch(self.x0s)
        return s

    def plant(self, b):
        if self.M is not None:
            return self.M.A[:, :, b], self.M.B[:, :, b], self.M.f[:, b]
        f = self.prob.fdyn if self.prob.fdyn is not None else np.zeros(self.prob.nx)
        return self.prob.A, self.prob.B, f

    def oracle(self, b):
        pb = self.M.problem(self.prob, b) if self.M is not None else self.prob
        return O.OraclePort(pb).load_problem(pb, self.case.settings)


def _final(s):
    sol, st = s.get_solution_batch(), s.get_stats_batch()
    return dict(states=sol["states"].copy(), controls=sol["controls"].copy(), **{k: np.array(v).copy() for k, v in st.items()})


_RUNS = {}


def _run(pkg, name, batch):
    """One rollout and its twin, ticks issued one by one, per (case, batch); computed once, never changed."""
    key = (name, batch)
    if key in _RUNS:
        return _RUNS[key]
    su = Setup(pkg, name, batch)
    prob = su.prob
    with _layout_env(su.case.layout_env):
        r, v, m = su.handle(), su.handle(auto_advance=False), su.handle()
        layout = r.launch_info()["layout"]
        logs = r.rollout(TICKS, disturbance=su.w)
        # the twin: solve, read back, plant step, (tracks) advance -- a synchronisation and copies after every tick
        tu = np.zeros((prob.nu, TICKS, batch))
        ti, ts = np.zeros((TICKS, batch), dtype=np.int32), np.zeros((TICKS, batch), dtype=np.int32)
        for t in range(TICKS):
            v.solve()
            st = v.get_stats_batch()
            tu[:, t, :] = v.get_first_controls_batch()
            ti[t], ts[t] = st["iter"], st["status"]
            v.plant_step(su.w[:, t, :])
            if su.case.tracks:
                v.advance_ref_step(1)
        steps = (r.get_ref_step_batch().copy(), v.get_ref_step_batch().copy())
        r.solve()
        v.solve()
        out = dict(su=su, layout=layout, logs=logs, twin=dict(u=tu, iter=ti, status=ts), steps=steps, final=(_final(r), _final(v)),
                   u_mpc_step=np.stack([m.mpc_step(logs["x"][:, t, :]) for t in range(TICKS)], axis=1), jit=r.jit_info())
        for h in (r, v, m):
            h.reset()
    _RUNS[key] = out
    return out


# ------------------------------------------------------------------------------------------------ 1. the rollout is its ticks, one by one
@pytest.mark.parametrize("name,batch", PARAMS)
def test_rollout_equals_ticks_issued_one_by_one(pkg, name, batch):
    run = _run(pkg, name, batch)
    su, logs, twin = run["su"], run["logs"], run["twin"]
    print("rollout %s batch %d: layout %s (%s), gpu_ms %.3f, iterations per tick %s"
          % (name, batch, run["layout"], run["jit"], logs["gpu_ms"], logs["iter"].mean(axis=1)))
    if su.case.layout:
        assert run["layout"] == su.case.layout
    assert logs["x"].shape == (su.prob.nx, TICKS + 1, batch) and logs["u"].shape == (su.prob.nu, TICKS, batch)
    assert logs["iter"].shape == (TICKS, batch) and logs["status"].shape == (TICKS, batch)
    np.testing.assert_array_equal(logs["u"], twin["u"])
    np.testing.assert_array_equal(logs["iter"], twin["iter"])
    np.testing.assert_array_equal(logs["status"], twin["status"])
    assert logs["iter"].min() >= 1 and logs["gpu_ms"] > 0.0
    np.testing.assert_array_equal(logs["x"][:, 0, :], su.x0s)
    # the ADMM state, x0 and the tracks' steps afterwards: one more solve on both
    fr, fv = run["final"]
    for k in fr:
        np.testing.assert_array_equal(fr[k], fv[k], err_msg=k)
    np.testing.assert_array_equal(run["steps"][0], run["steps"][1])
    if su.case.tracks:
        np.testing.assert_array_equal(run["steps"][0], np.full(batch, TICKS, dtype=np.int32))
    # a third handle driven through mpc_step and FED the logged states (there is no getter for x0: the twin above never shows the state
    # it holds, this one is given the log's): tick 0, and every tick after it, returns the logged first controls bit for bit
    np.testing.assert_array_equal(logs["u"], run["u_mpc_step"])


# ------------------------------------------------------------------------------------------------ 2. the plant arithmetic
@pytest.mark.parametrize("name,batch", PARAMS)
def test_plant_step_is_the_plant(pkg, name, batch):
    run = _run(pkg, name, batch)
    su, x, u = run["su"], run["logs"]["x"], run["logs"]["u"]
    worst = 0.0
    for b in range(batch):
        A, B, f = su.plant(b)
        want = A @ x[:, :TICKS, b] + B @ u[:, :, b] + f[:, None] + su.w[:, :, b]
        worst = max(worst, float(np.max(np.abs(x[:, 1:, b] - want) / (1e-15 + 1e-12 * np.abs(want)))))
        np.testing.assert_allclose(x[:, 1:, b], want, rtol=1e-12, atol=1e-15, err_msg="instance %d" % b)
    print("plant %s batch %d: worst |error| / (atol + rtol |want|) = %.3f" % (name, batch, worst))


# ------------------------------------------------------------------------------------------------ 3. every logged tick against the oracle
@pytest.mark.parametrize("name,batch", PARAMS)
def test_logged_ticks_match_the_oracle(pkg, name, batch):
    run = _run(pkg, name, batch)
    su, logs = run["su"], run["logs"]
    N = su.prob.N
    for b in _sample(batch):
        orc = su.oracle(b)  # warm-started from tick to tick, as the handle is
        for t in range(TICKS):
            orc.set_x0(logs["x"][:, t, b])
            if su.case.tracks:
                wx, wu = _windows(su.X[:, :, b:b + 1], su.U[:, :, b:b + 1], [t], N)
                orc.set_x_ref(wx[:, :, 0])
                orc.set_u_ref(wu[:, :, 0])
            orc.solve()
            ost = orc.stats()
            err = rel_err(logs["u"][:, t, b], orc.solution()[1][:, 0])
            print("oracle %s batch %d instance %d tick %d: iter %d (oracle %d) status %d (oracle %d) rel_err u0 %.2e"
                  % (name, batch, b, t, logs["iter"][t, b], ost["iter"], logs["status"][t, b], ost["status"], err))
            assert logs["iter"][t, b] == ost["iter"], (b, t)
            assert logs["status"][t, b] == ost["status"], (b, t)
            assert err < TOL, (b, t, err)


# ------------------------------------------------------------------------------------------------ helpers of the device forms
class _Device(_DeviceArrays):
    """_DeviceArrays with buffers of any dtype, filled from numpy as the bytes lie, and read back."""

    def put_raw(self, a):
        h = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(h.nbytes, 8)) == 0
        self.ptrs.append(p)
        assert self.hip.hipMemcpy(p, C.c_void_p(h.ctypes.data), h.nbytes, 1) == 0  # hipMemcpyHostToDevice
        return p

    def get_raw(self, p, like):
        out = np.empty_like(np.ascontiguousarray(like))
        assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), p, out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return out


def _quad(pkg, batch, settings=SETTINGS):
    P = pkg.problems
    prob = P.quadrotor(20)
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho, **settings)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    s.set_x0_batch(_x0s(prob, batch))
    return prob, s


def _assert_logs_equal(a, b, keys=("x", "u", "iter", "status")):
    for k in keys:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)


def _from_tensors(out):
    """(batch, ticks, rows) / (batch, ticks) tensors -> the host form's (rows, ticks, batch) / (ticks, batch) arrays."""
    return {k: np.ascontiguousarray(t.cpu().numpy()).T for k, t in out.items()}


# ------------------------------------------------------------------------------------------------ 4. disturbance
@pytest.mark.parametrize("batch", [37, 300])
def test_disturbance_from_host_device_and_zero(pkg, batch):
    run = _run(pkg, "quadrotor20_d", batch)  # (the host form with this disturbance)
    su = run["su"]
    with _layout_env("D"):
        torch = _torch_gpu()
        if torch is not None:
            d = su.handle()
            wt = torch.from_numpy(np.ascontiguousarray(su.w.T)).cuda()  # (batch, ticks, nx): the same memory
            got = d.rollout(TICKS, disturbance=wt)
            _assert_logs_equal(run["logs"], _from_tensors(got))
            d.reset()
        # ... and from device memory filled through the HIP runtime (torch or not), through the C verb
        d = su.handle()
        dev = _Device(pkg)
        L = pkg._lib
        shapes = dict(x=np.zeros((batch, TICKS + 1, su.prob.nx)), u=np.zeros((batch, TICKS, su.prob.nu)),
                      iter=np.zeros((batch, TICKS), dtype=np.int32), status=np.zeros((batch, TICKS), dtype=np.int32))
        ptrs = {k: dev.put_raw(a) for k, a in shapes.items()}
        logs = L.RolloutLogs(ptrs["x"], ptrs["u"], ptrs["iter"], ptrs["status"])
        assert pkg.load_library().tinympc_rollout_batch_device(d._h, TICKS, dev.put(su.w), C.byref(logs)) == 0
        d.synchronize()
        _assert_logs_equal(run["logs"], {k: dev.get_raw(ptrs[k], shapes[k]).T for k in shapes})
        dev.free()
        d.reset()
        # w = 0 passed explicitly is no disturbance
        a, b = su.handle(), su.handle()
        la, lb = a.rollout(TICKS), b.rollout(TICKS, disturbance=np.zeros_like(su.w))
        _assert_logs_equal(la, lb)
        assert np.abs(la["x"] - run["logs"]["x"]).max() > 1e-4  # (the disturbance of the shared run is one)
        a.reset()
        b.reset()


# ------------------------------------------------------------------------------------------------ 5. plant override
@pytest.mark.parametrize("batch", [37, 300])
def test_plant_override(pkg, batch):
    prob, s = _quad(pkg, batch)
    _, plain = _quad(pkg, batch)
    rng = np.random.default_rng(17)
    nx, nu = prob.nx, prob.nu
    Ap = prob.A[:, :, None] + 5e-3 * rng.uniform(-1, 1, (nx, nx, batch))
    Bp = prob.B[:, :, None] * rng.uniform(0.8, 1.2, (nx, nu, batch))
    fp = 1e-3 * rng.standard_normal((nx, batch))
    w = _disturbance(prob, batch)
    cache = s.get_cache_batch()
    layout = s.launch_info()["layout"]
    E = pkg._lib.ERR_INVALID_INPUT
    for bad in (lambda: s.set_plant_batch(Ap[:, :, :5], Bp[:, :, :5], first=2),                    # the first call names the whole batch
                lambda: s.set_plant_batch(Ap, Bp, first=1),                                         # beyond the batch
                lambda: s.set_plant_batch(np.where(np.arange(batch) == 3, np.nan, Ap), Bp),        # finite values
                lambda: s.set_plant_batch(Ap, Bp, f=np.where(np.arange(batch) == batch - 1, np.inf, fp))):
        with pytest.raises(pkg.TinyMPCError) as ei:
            bad()
        assert ei.value.code == E
    # a refused override is no override: the model's own plant
    ref = plain.rollout(TICKS, disturbance=w)
    _assert_logs_equal(ref, s.rollout(TICKS, disturbance=w))
    for h in (s, plain):
        h.reset_workspace()
        h.set_x0_batch(_x0s(prob, batch))
    s.set_plant_batch(Ap, Bp, f=fp)
    lo, hi = batch // 3, batch // 3 + 7  # a sub-range replaces only its range (and, without f, its affine term is zero)
    A2, B2 = Ap[:, :, lo:hi] + 1e-3, Bp[:, :, lo:hi] * 1.05
    s.set_plant_batch(A2, B2, first=lo)
    Ap[:, :, lo:hi], Bp[:, :, lo:hi], fp[:, lo:hi] = A2, B2, 0.0
    got = s.rollout(TICKS, disturbance=w)
    for b in range(batch):
        want = Ap[:, :, b] @ got["x"][:, :TICKS, b] + Bp[:, :, b] @ got["u"][:, :, b] + fp[:, b:b + 1] + w[:, :, b]
        np.testing.assert_allclose(got["x"][:, 1:, b], want, rtol=1e-12, atol=1e-15, err_msg="instance %d" % b)
    assert np.abs(got["x"] - ref["x"]).max() > 1e-4  # (the override is one)
    # the controller is untouched
    after = s.get_cache_batch()
    for k in cache:
        np.testing.assert_array_equal(cache[k], after[k], err_msg=k)
    assert s.launch_info()["layout"] == layout
    # from device memory: the same bits
    torch = _torch_gpu()
    if torch is not None:
        d = _quad(pkg, batch)[1]
        tt = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).T)).cuda()
        d.set_plant_batch(tt(Ap), tt(Bp), f=tt(fp))
        _assert_logs_equal(got, d.rollout(TICKS, disturbance=w))
        with pytest.raises(pkg.TinyMPCError) as ei:
            d.set_plant_batch(tt(np.where(np.arange(batch) == 1, np.inf, Ap)), tt(Bp))
        assert ei.value.code == E
        d.reset()
    # cleared: the bits of a handle that never had one
    s.clear_plant_batch()
    for h in (s, plain):
        h.reset_workspace()
        h.set_x0_batch(_x0s(prob, batch))
    _assert_logs_equal(plain.rollout(TICKS, disturbance=w), s.rollout(TICKS, disturbance=w))
    s.reset()
    plain.reset()


# ------------------------------------------------------------------------------------------------ 6. the _device form
@pytest.mark.parametrize("batch", [37, 300])
def test_device_form_logs_into_caller_memory(pkg, batch):
    """Logs in torch tensors where torch sees the GPU, in device memory from the HIP runtime otherwise; read after a synchronisation of
    the handle's stream (the call returns once the work is queued). Sentinels show that every element was written."""
    run = _run(pkg, "quadrotor20_d", batch)
    su = run["su"]
    nx, nu, N = su.prob.nx, su.prob.nu, su.prob.N
    torch = _torch_gpu()
    dev = _Device(pkg)
    with _layout_env("D"):
        d = su.handle()
        other = _quad(pkg, batch)[1]
        if torch is not None:
            out = dict(x=torch.full((batch, TICKS + 1, nx), -7.0, dtype=torch.float64, device="cuda"),
                       u=torch.full((batch, TICKS, nu), -7.0, dtype=torch.float64, device="cuda"),
                       iter=torch.full((batch, TICKS), -7, dtype=torch.int32, device="cuda"),
                       status=torch.full((batch, TICKS), -7, dtype=torch.int32, device="cuda"))
            wt = torch.from_numpy(np.ascontiguousarray(su.w.T)).cuda()
            assert d.rollout(TICKS, disturbance=wt, out=out) is out
            d.synchronize()
            torch.cuda.synchronize()
            got = _from_tensors(out)
            other.set_x_ref_track_batch(out["x"])  # a rollout's x log is a track: handed as it is to another handle
        else:
            shapes = dict(x=np.full((batch, TICKS + 1, nx), -7.0), u=np.full((batch, TICKS, nu), -7.0),
                          iter=np.full((batch, TICKS), -7, dtype=np.int32), status=np.full((batch, TICKS), -7, dtype=np.int32))
            ptrs = {k: dev.put_raw(a) for k, a in shapes.items()}
            logs = pkg._lib.RolloutLogs(ptrs["x"], ptrs["u"], ptrs["iter"], ptrs["status"])
            lib = pkg.load_library()
            assert lib.tinympc_rollout_batch_device(d._h, TICKS, dev.put(su.w), C.byref(logs)) == 0
            d.synchronize()
            got = {k: dev.get_raw(ptrs[k], shapes[k]).T for k in shapes}
            assert lib.tinympc_set_x_ref_track_batch_device(other._h, ptrs["x"], nx, TICKS + 1, 0, batch) == 0
        _assert_logs_equal(run["logs"], got)
        other.solve()
        byhand = _quad(pkg, batch)[1]
        byhand.set_x_ref_batch(_windows(run["logs"]["x"], np.zeros((nu, 1, batch)), np.zeros(batch, dtype=int), N)[0])
        byhand.solve()
        np.testing.assert_array_equal(other.get_solution_batch()["controls"], byhand.get_solution_batch()["controls"])
        dev.free()
        for h in (d, other, byhand):
            h.reset()


# ------------------------------------------------------------------------------------------------ 7. NULL log members
def test_each_log_member_may_be_null(pkg):
    batch = 37
    run = _run(pkg, "quadrotor20_d", batch)
    su = run["su"]
    with _layout_env("D"):
        for drop in ("x", "u", "iter", "status"):
            keep = tuple(k for k in ("x", "u", "iter", "status") if k != drop)
            h = su.handle()
            got = h.rollout(TICKS, disturbance=su.w, log=keep)
            assert drop not in got
            _assert_logs_equal(run["logs"], got, keys=keep)
            h.reset()
        h = su.handle()  # no logs at all: the state still moves
        lib = pkg.load_library()
        w = np.asfortranarray(su.w)
        assert lib.tinympc_rollout_batch(h._h, TICKS, w.ctypes.data_as(pkg._lib.c_double_p), None, None) == 0
        h.solve()
        for k, val in run["final"][0].items():
            np.testing.assert_array_equal(_final(h)[k], val, err_msg=k)
        h.reset()


# ------------------------------------------------------------------------------------------------ 8. refusals change nothing
def _snapshot(s):
    return _final(s), s.get_ref_step_batch().copy()


def _assert_unchanged(s, snap, tag):
    now = _snapshot(s)
    for k in snap[0]:
        np.testing.assert_array_equal(snap[0][k], now[0][k], err_msg="%s %s" % (tag, k))
    np.testing.assert_array_equal(snap[1], now[1], err_msg=str(tag))


def test_refusals_change_nothing(pkg):
    batch = 37
    lib, L = pkg.load_library(), pkg._lib
    prob, s = _quad(pkg, batch)
    _, twin = _quad(pkg, batch)
    X, U = _tracks(prob, batch, TRACK_T, TRACK_T)
    for h in (s, twin):
        h.set_x_ref_track_batch(X)
        h.set_ref_step_batch(np.arange(batch) % 3)
        h.set_ref_auto_advance(1)
        h.solve()
    snap = _snapshot(s)
    nx, nu = prob.nx, prob.nu
    sent = dict(x=np.full((nx, TICKS + 1, batch), -7.0, order="F"), u=np.full((nu, TICKS, batch), -7.0, order="F"),
                iter=np.full((TICKS, batch), -7, dtype=np.int32, order="F"), status=np.full((TICKS, batch), -7, dtype=np.int32, order="F"))
    logs = L.RolloutLogs(*[sent[k].ctypes.data for k in ("x", "u", "iter", "status")])
    ms = C.c_float(-1.0)
    w = _disturbance(prob, batch)
    wp = w.ctypes.data_as(L.c_double_p)

    def untouched(tag):
        assert ms.value == -1.0, tag
        for k, a in sent.items():
            assert (a == -7).all(), (tag, k)
        _assert_unchanged(s, snap, tag)

    for ticks in (0, -3):
        assert lib.tinympc_rollout_batch(s._h, ticks, wp, C.byref(logs), C.byref(ms)) == L.ERR_INVALID_INPUT
        assert lib.tinympc_rollout_batch_device(s._h, ticks, None, None) == L.ERR_INVALID_INPUT
        untouched(("ticks", ticks))
    # host memory handed to the _device form: the disturbance, a log
    assert lib.tinympc_rollout_batch_device(s._h, TICKS, C.c_void_p(w.ctypes.data), None) == L.ERR_INVALID_INPUT
    assert "device memory" in L.last_error()
    assert lib.tinympc_rollout_batch_device(s._h, TICKS, None, C.byref(logs)) == L.ERR_INVALID_INPUT
    untouched("host memory")
    # ranges beyond the batch
    A, B = np.repeat(prob.A[:, :, None], batch, axis=2), np.repeat(prob.B[:, :, None], batch, axis=2)
    for first, count in ((1, batch), (-1, batch), (0, 0), (0, batch + 1)):
        a, b = np.asfortranarray(A), np.asfortranarray(B)
        assert lib.tinympc_set_plant_batch(s._h, a.ctypes.data_as(L.c_double_p), b.ctypes.data_as(L.c_double_p), None, first, count) == L.ERR_INVALID_INPUT
    untouched("plant range")
    # a tick of zero iterations writes no control
    s.update_settings(max_iter=0)
    assert lib.tinympc_rollout_batch(s._h, TICKS, wp, C.byref(logs), C.byref(ms)) == L.ERR_INVALID_INPUT
    assert "max_iter" in L.last_error()
    s.update_settings(max_iter=SETTINGS["max_iter"])
    untouched("max_iter")
    # x0 too: one more solve on the handle and on its twin, which saw none of the refused calls
    s.solve()
    twin.solve()
    a, b = _snapshot(s), _snapshot(twin)
    for k in a[0]:
        np.testing.assert_array_equal(a[0][k], b[0][k], err_msg=k)
    np.testing.assert_array_equal(a[1], b[1])
    s.reset()
    twin.reset()


def test_single_instance_handles_and_sessions_are_refused(pkg):
    lib, L = pkg.load_library(), pkg._lib
    P = pkg.problems
    prob = P.cartpole(10, True)
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, rho=prob.rho, **SETTINGS)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    s.set_x0(prob.x0)
    s.solve()
    before = (s.get_solution(), s.get_stats())
    A, B = np.asfortranarray(prob.A), np.asfortranarray(prob.B)
    calls = (lambda: lib.tinympc_rollout_batch(s._h, TICKS, None, None, None), lambda: lib.tinympc_rollout_batch_device(s._h, TICKS, None, None),
             lambda: lib.tinympc_plant_step_batch(s._h, None),
             lambda: lib.tinympc_set_plant_batch(s._h, A.ctypes.data_as(L.c_double_p), B.ctypes.data_as(L.c_double_p), None, 0, 1))
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
    s.reset()


def test_a_configuration_the_launch_refuses_is_refused_before_tick_0(pkg):
    """Per-instance goals with a shared cone: no kernel carries them, and a solve says so. The rollout returns the launch's own code and
    message and has queued nothing: gpu_ms and the logs hold their sentinels, the solution and the statistics their bits."""
    batch = 37
    lib, L = pkg.load_library(), pkg._lib
    prob, s = _quad(pkg, batch)
    s.solve()
    snap = _final(s)
    s.set_u_ref_batch(0.05 * np.random.default_rng(3).standard_normal((prob.nu, batch)))
    s.set_cone_constraints(np.array([0]), np.array([3]), np.array([0.5]), np.array([0]), np.array([2]), np.array([1.0]))
    s.update_settings(en_state_soc=1)
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.solve()
    assert ei.value.code == L.ERR_UNSUPPORTED
    message = str(ei.value).split(": ", 1)[1]
    nx, nu = prob.nx, prob.nu
    sent = dict(x=np.full((nx, TICKS + 1, batch), -7.0, order="F"), u=np.full((nu, TICKS, batch), -7.0, order="F"),
                iter=np.full((TICKS, batch), -7, dtype=np.int32, order="F"), status=np.full((TICKS, batch), -7, dtype=np.int32, order="F"))
    logs = L.RolloutLogs(*[sent[k].ctypes.data for k in ("x", "u", "iter", "status")])
    ms = C.c_float(-1.0)
    assert lib.tinympc_rollout_batch(s._h, TICKS, None, C.byref(logs), C.byref(ms)) == L.ERR_UNSUPPORTED
    assert L.last_error() == message and "per-instance references" in message
    assert lib.tinympc_rollout_batch_device(s._h, TICKS, None, None) == L.ERR_UNSUPPORTED
    assert L.last_error() == message
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.rollout(TICKS)
    assert ei.value.code == L.ERR_UNSUPPORTED
    assert ms.value == -1.0
    for k, a in sent.items():
        assert (a == -7).all(), k
    now = _final(s)
    for k in snap:
        np.testing.assert_array_equal(snap[k], now[k], err_msg=k)
    s.reset()
