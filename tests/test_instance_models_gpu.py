"""Per-instance models of batched handles (tinympc_set_model_batch and its _device form, tinympc_clear_model_batch,
tinympc_get_cache_batch): every instance solves what a single-instance handle set up with its own (A, B, fdyn, Q, R) would solve --
checked against the oracle per instance, with caches bit-identical to that single-instance handle's, bit for bit against the shared-model
handle where the models coincide, together with per-instance references and bounds, across partial ranges, closed-loop ticks, device
input and sharding; and the configurations no kernel carries are refused, never solved with the shared model.

Models are seeded perturbations of the project's problems: B and the Q, R diagonals scaled entry by entry within +-15 %, A moved by at
most 1e-2 per entry, fdyn non-zero where a case says so. TOL and the sample are the sibling files'; a seed that put a sampled instance on
a termination edge against the oracle would be changed here and said so (none had to be)."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np
import pytest
from conftest import rel_err

import pyoracle as O
from test_instance_bounds_gpu import _DeviceArrays, _bounds, _refs, _torch_gpu, _wide, _x0s

pytestmark = pytest.mark.gpu

TOL = 1e-9
CACHE_TOL = 1e-11  # (test_hip_parity.py: test_precompute_kernel_matches_reference_cache)
SETTINGS = dict(max_iter=100, abs_pri_tol=1e-4, abs_dua_tol=1e-4)

CASES = {  # name -> (problem, batch, non-zero fdyn?)
    "quadrotor50": (lambda P: P.quadrotor(50), 1301, False),
    "cartpole20": (lambda P: P.cartpole(20, True), 37, True),
    "wide32": (lambda P: _wide(P, 24, 8, 20), 37, True),
    "wide64": (lambda P: _wide(P, 48, 16, 12), 21, False),
    "quadrotor120": (lambda P: P.quadrotor(120), 70, True),
}


@dataclasses.dataclass
class Models:
    A: np.ndarray  # nx x nx x batch
    B: np.ndarray  # nx x nu x batch
    Q: np.ndarray  # nx x nx x batch (diagonal)
    R: np.ndarray  # nu x nu x batch (diagonal)
    f: np.ndarray | None  # nx x batch

    def verb(self, lo=0, hi=None):
        """What set_model_batch takes for instances [lo, hi): A, B, Q, R and the fdyn keyword."""
        cut = lambda a: np.ascontiguousarray(a[..., lo:hi])
        return (cut(self.A), cut(self.B), cut(self.Q), cut(self.R)), dict(fdyn=None if self.f is None else cut(self.f))

    def problem(self, prob, b):
        """The problem instance b solves: the handle's horizon, rho, bounds and references with instance b's model."""
        return dataclasses.replace(prob, A=self.A[:, :, b].copy(), B=self.B[:, :, b].copy(), Q=self.Q[:, :, b].copy(), R=self.R[:, :, b].copy(),
                                   fdyn=None if self.f is None else self.f[:, b].copy())


def _models(prob, batch, seed=1, fdyn=False):
    rng = np.random.default_rng(1000 + seed)
    nx, nu = prob.nx, prob.nu
    A = prob.A[:, :, None] + 1e-2 * rng.uniform(-1.0, 1.0, (nx, nx, batch))
    B = prob.B[:, :, None] * rng.uniform(0.85, 1.15, (nx, nu, batch))
    Q = np.zeros((nx, nx, batch))
    R = np.zeros((nu, nu, batch))
    Q[np.arange(nx), np.arange(nx), :] = np.diag(prob.Q)[:, None] * rng.uniform(0.85, 1.15, (nx, batch))
    R[np.arange(nu), np.arange(nu), :] = np.diag(prob.R)[:, None] * rng.uniform(0.85, 1.15, (nu, batch))
    f = 2e-3 * rng.standard_normal((nx, batch)) if fdyn else None
    return Models(A, B, Q, R, f)


def _shared_models(prob, batch):
    rep = lambda a: np.repeat(np.asarray(a, dtype=np.float64)[..., None], batch, axis=-1)
    return Models(rep(prob.A), rep(prob.B), rep(prob.Q), rep(prob.R), None if prob.fdyn is None else rep(prob.fdyn))


def _solver(pkg, prob, batch, settings=SETTINGS):
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho, fdyn=prob.fdyn, **settings)
    if prob.has_bounds():
        s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if prob.x_ref is not None:
        s.set_x_ref(prob.x_ref)
    if prob.u_ref is not None:
        s.set_u_ref(prob.u_ref)
    return s


def _set_models(s, M, lo=0, hi=None):
    args, kw = M.verb(lo, hi)
    s.set_model_batch(*args, first=lo, **kw)


def _oracle(pb, settings=SETTINGS):
    return O.OraclePort(pb).load_problem(pb, settings)


def _sample(batch):
    return sorted({0, 1, batch // 2, batch - 2, batch - 1})


def _check(s, orcs, x0s, tag):
    sol, st = s.get_solution_batch(), s.get_stats_batch()
    for b, orc in orcs.items():
        orc.set_x0(x0s[:, b])
        orc.solve()
        ex, eu = rel_err(sol["states"][:, :, b], orc.solution()[0]), rel_err(sol["controls"][:, :, b], orc.solution()[1])
        print("models %s instance %d: iter %d (oracle %d) status %d (oracle %d) rel_err x %.2e u %.2e"
              % (tag, b, st["iter"][b], orc.stats()["iter"], st["status"][b], orc.stats()["status"], ex, eu))
        assert st["iter"][b] == orc.stats()["iter"], (tag, b)
        assert st["status"][b] == orc.stats()["status"], (tag, b)
        assert ex < TOL and eu < TOL, (tag, b, ex, eu)


def _same(a, b):
    sa, sb = a.get_solution_batch(), b.get_solution_batch()
    np.testing.assert_array_equal(sa["states"], sb["states"])
    np.testing.assert_array_equal(sa["controls"], sb["controls"])
    ta, tb = a.get_stats_batch(), b.get_stats_batch()
    for k in ta:  # iterations, status, the four residuals
        np.testing.assert_array_equal(ta[k], tb[k])


@pytest.mark.parametrize("case", list(CASES))
def test_each_instance_matches_the_oracle_with_its_own_model(pkg, case):
    prob, batch, fdyn = CASES[case][0](pkg.problems), CASES[case][1], CASES[case][2]
    M = _models(prob, batch, fdyn=fdyn)
    s = _solver(pkg, prob, batch)
    _set_models(s, M)
    samples = _sample(batch)
    orcs = {b: _oracle(M.problem(prob, b)) for b in samples}
    sols = []
    for rnd in range(3):  # a cold start, then two warm starts
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        s.set_x0_batch(x0s)
        s.solve()
        _check(s, orcs, x0s, (case, rnd))
        sols.append(s.get_solution_batch()["states"])
    # the models matter: the same x0 under the shared model gives another trajectory (the states, not the controls: a control sequence
    # that sits on its bounds throughout, as the cartpole's does from these x0, is the same under both models)
    ref = _solver(pkg, prob, batch)
    ref.set_x0_batch(_x0s(prob, batch, 1.0, seed=0))
    ref.solve()
    for b in samples:
        assert rel_err(ref.get_solution_batch()["states"][:, :, b], sols[0][:, :, b]) > 1e-6, b
    assert s.launch_info()["layout"] == "A"
    assert "per-instance-models" in s.jit_info(), s.jit_info()
    assert "per-instance-models" not in ref.jit_info()
    s.reset()
    ref.reset()


@pytest.mark.parametrize("case,precompute", [("quadrotor50", None), ("quadrotor50", "lds"), ("cartpole20", None), ("cartpole20", "lds"),
                                             ("wide32", None), ("wide64", None)])
def test_caches_equal_single_instance_setups(pkg, monkeypatch, case, precompute):
    """get_cache_batch of an instance == get_cache of a single-instance handle set up with its model (both precompute kernels: the
    register-resident one, the one-workgroup one through TINYMPC_PRECOMPUTE=lds and through nu > 4), and both agree with the oracle."""
    if precompute:
        monkeypatch.setenv("TINYMPC_PRECOMPUTE", precompute)
    prob, batch, fdyn = CASES[case][0](pkg.problems), CASES[case][1], CASES[case][2]
    M = _models(prob, batch, seed=2, fdyn=fdyn)
    s = _solver(pkg, prob, batch)
    shared = s.get_cache()
    rep = s.get_cache_batch(1, 3)  # without the mode: the shared cache, repeated
    for n in ("Kinf", "Pinf", "Quu_inv", "AmBKt"):
        for j in range(3):
            np.testing.assert_array_equal(rep[n][:, :, j], shared[n])
    assert list(rep["riccati_iters"]) == [shared["riccati_iters"]] * 3
    _set_models(s, M)
    whole = s.get_cache_batch()
    for b in _sample(batch):
        pb = M.problem(prob, b)
        one = pkg.TinyMPC()
        one.setup(pb.A, pb.B, pb.Q, pb.R, pb.N, rho=pb.rho, fdyn=pb.fdyn)
        c1 = one.get_cache()
        cb = s.get_cache_batch(b, 1)
        orc = O.OraclePort(pb)
        for n in ("Kinf", "Pinf", "Quu_inv", "AmBKt"):
            np.testing.assert_array_equal(cb[n][:, :, 0], c1[n], err_msg="%s instance %d" % (n, b))
            np.testing.assert_array_equal(whole[n][:, :, b], c1[n])
            e = rel_err(cb[n][:, :, 0], orc.get(n))
            print("cache %s %s instance %d %s: rel_err against the oracle %.2e" % (case, precompute, b, n, e))
            assert e < CACHE_TOL, (n, b, e)
        assert cb["riccati_iters"][0] == whole["riccati_iters"][b] == c1["riccati_iters"] == orc.stats()["riccati_iters"], b
        one.reset()
    np.testing.assert_array_equal(s.get_cache()["Pinf"], shared["Pinf"])  # the single-model verb keeps addressing the shared cache
    s.reset()


@pytest.mark.parametrize("case", list(CASES))
def test_equal_models_are_bit_identical_to_the_shared_handle(pkg, monkeypatch, case):
    prob, batch = CASES[case][0](pkg.problems), min(CASES[case][1], 300)
    monkeypatch.setenv("TINYMPC_LAYOUT", "A")
    shared = _solver(pkg, prob, batch)
    monkeypatch.delenv("TINYMPC_LAYOUT", raising=False)
    inst = _solver(pkg, prob, batch)
    _set_models(inst, _shared_models(prob, batch))
    for rnd in range(3):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        for h in (shared, inst):
            h.set_x0_batch(x0s)
            h.solve()
        _same(shared, inst)
    assert shared.launch_info()["layout"] == inst.launch_info()["layout"] == "A"
    assert "per-instance-models" not in shared.jit_info() and "per-instance-models" in inst.jit_info()
    shared.reset()
    inst.reset()


@pytest.mark.parametrize("refs,bounds", [("goal", "box"), ("trajectory", "box"), ("goal", "knot"), ("trajectory", "knot")])
def test_combined_with_per_instance_references_and_bounds(pkg, refs, bounds):
    P = pkg.problems
    prob, batch = P.quadrotor(50), 301
    M = _models(prob, batch, seed=3, fdyn=True)
    s = _solver(pkg, prob, batch)
    (vx, vu), (X, U) = _refs(prob, batch, refs, seed=3)
    verb, full = _bounds(prob, batch, bounds, seed=4)
    s.set_x_ref_batch(vx)
    _set_models(s, M)  # (any order)
    s.set_bound_constraints_batch(*verb)
    s.set_u_ref_batch(vu)
    samples = _sample(batch)
    orcs = {}
    for b in samples:
        pb = dataclasses.replace(M.problem(prob, b), x_min=full[0][:, :, b], x_max=full[1][:, :, b], u_min=full[2][:, :, b], u_max=full[3][:, :, b])
        orcs[b] = _oracle(pb)
        orcs[b].set_x_ref(X[:, :, b])
        orcs[b].set_u_ref(U[:, :, b])
    for rnd in range(2):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        s.set_x0_batch(x0s)
        s.solve()
        _check(s, orcs, x0s, (refs, bounds, rnd))
    info = s.jit_info()
    assert "per-instance-refs" in info and "per-instance-bounds" in info and "per-instance-models" in info, info
    assert s.launch_info()["layout"] == "A"  # (goals and boxes too: the models run on layout A whatever the form)
    s.reset()


def test_partial_ranges_second_call_and_clear(pkg, monkeypatch):
    P = pkg.problems
    prob, batch = P.quadrotor(50), 200
    M, M2 = _models(prob, batch, seed=5), _models(prob, batch, seed=6, fdyn=True)
    s = _solver(pkg, prob, batch)
    _set_models(s, M, 10, 60)
    _set_models(s, M2, 55, 57)  # a second call over a sub-range
    monkeypatch.setenv("TINYMPC_LAYOUT", "A")
    shared = _solver(pkg, prob, batch)
    monkeypatch.delenv("TINYMPC_LAYOUT", raising=False)
    inside = {b: _oracle((M2 if 55 <= b < 57 else M).problem(prob, b)) for b in (10, 30, 54, 55, 56, 57, 59)}
    outside = [b for b in range(batch) if not 10 <= b < 60]
    for rnd in range(2):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        for h in (s, shared):
            h.set_x0_batch(x0s)
            h.solve()
        _check(s, inside, x0s, ("partial", rnd))
        a, b = s.get_solution_batch(), shared.get_solution_batch()
        np.testing.assert_array_equal(a["states"][:, :, outside], b["states"][:, :, outside])
        np.testing.assert_array_equal(a["controls"][:, :, outside], b["controls"][:, :, outside])
        np.testing.assert_array_equal(s.get_stats_batch()["iter"][outside], shared.get_stats_batch()["iter"][outside])
        np.testing.assert_array_equal(s.get_stats_batch()["residuals"][:, outside], shared.get_stats_batch()["residuals"][:, outside])
    # kept across reset_workspace, update_settings and the shared reference / bound verbs
    s.reset_workspace()
    s.update_settings(max_iter=80)
    s.set_u_ref(np.zeros((prob.nu, prob.N - 1)))
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    assert "per-instance-models" in s.jit_info()
    settings = dict(SETTINGS, max_iter=80)
    x0s = _x0s(prob, batch)
    s.set_x0_batch(x0s)
    s.solve()
    _check(s, {b: _oracle((M2 if 55 <= b < 57 else M).problem(prob, b), settings) for b in (10, 56, 59)}, x0s, "after reset")
    # clear_model_batch: every instance on the shared model again, as a handle that never had the mode
    s.clear_model_batch()
    assert "per-instance-models" not in s.jit_info()
    ref = _solver(pkg, prob, batch, settings)
    ref.set_u_ref(np.zeros((prob.nu, prob.N - 1)))
    for h in (s, ref):
        h.reset_workspace()
        h.set_x0_batch(x0s)
        h.solve()
    _same(s, ref)
    assert s.launch_info()["layout"] == ref.launch_info()["layout"]
    for h in (s, shared, ref):
        h.reset()


@pytest.mark.parametrize("batch", [64, 300])
def test_closed_loop_with_each_instances_own_plant(pkg, batch):
    """Four ticks of mpc_step_batch, every instance's state advanced by its OWN plant x+ = A_b x + B_b u + fdyn_b; against per-instance
    oracles warm-started from tick to tick, and against the three verbs a tick stands for."""
    P = pkg.problems
    prob = P.quadrotor(50)
    settings = dict(max_iter=50, abs_pri_tol=1e-4, abs_dua_tol=1e-4)
    M = _models(prob, batch, seed=7, fdyn=True)
    s, v = _solver(pkg, prob, batch, settings), _solver(pkg, prob, batch, settings)
    for h in (s, v):
        _set_models(h, M)
    samples = _sample(batch)
    orcs = {b: _oracle(M.problem(prob, b), settings) for b in samples}
    x = _x0s(prob, batch)
    for k in range(4):
        u = s.mpc_step(x)
        v.set_x0_batch(x)
        v.solve()
        np.testing.assert_array_equal(u, v.get_first_controls_batch())
        st = s.get_stats_batch()
        for b, orc in orcs.items():
            orc.set_x0(x[:, b])
            orc.solve()
            assert st["iter"][b] == orc.stats()["iter"], (k, b)
            assert rel_err(u[:, b], orc.solution()[1][:, 0]) < TOL, (k, b)
        x = np.asfortranarray(np.einsum("ijb,jb->ib", M.A, x) + np.einsum("ijb,jb->ib", M.B, u) + M.f)
    assert "per-instance-models" in s.jit_info() and s.launch_info()["layout"] == "A"
    s.reset()
    v.reset()


def test_device_input_matches_host_input(pkg):
    P = pkg.problems
    prob, batch = P.quadrotor(50), 300
    x0s = _x0s(prob, batch)
    torch = _torch_gpu()
    L, E = pkg.load_library(), pkg._lib.ERR_INVALID_INPUT
    dev = _DeviceArrays(pkg)
    for fdyn in (True, False):
        M = _models(prob, batch, seed=8, fdyn=fdyn)
        h, d = _solver(pkg, prob, batch), _solver(pkg, prob, batch)
        _set_models(h, M)
        assert L.tinympc_set_model_batch_device(d._h, dev.put(M.A), dev.put(M.B), dev.put(M.f) if fdyn else None, dev.put(M.Q), dev.put(M.R),
                                                0, batch) == 0
        dev.free()  # (the copies have completed when the verb returns)
        handles = [h, d]
        if torch is not None:  # the Python method's tensor form: (count, cols, rows)
            t = _solver(pkg, prob, batch)
            tt = lambda a: torch.from_numpy(np.ascontiguousarray(a.T)).cuda()
            t.set_model_batch(tt(M.A), tt(M.B), tt(M.Q), tt(M.R), fdyn=tt(M.f) if fdyn else None)
            handles.append(t)
        for q in handles:
            q.set_x0_batch(x0s)
            q.solve()
        for q in handles[1:]:
            assert "per-instance-models" in q.jit_info()
            _same(h, q)
            ca, cb = h.get_cache_batch(), q.get_cache_batch()
            for n in ca:
                np.testing.assert_array_equal(ca[n], cb[n])
        for q in handles:
            q.reset()
    # host memory through the device verb is refused, and so is any one device pointer that is host memory
    s = _solver(pkg, prob, batch)
    buf = np.zeros(prob.nx * prob.nx * 4)
    hp = C.c_void_p(buf.ctypes.data)
    f = L.tinympc_set_model_batch_device
    assert f(s._h, hp, hp, hp, hp, hp, 0, 4) == E
    good = [dev.put(np.zeros((prob.nx, prob.nx, 4))) for _ in range(5)]
    for i in range(5):
        args = list(good)
        args[i] = hp
        assert f(s._h, *args, 0, 4) == E
    dev.free()
    if torch is not None:  # tensors the library cannot read correctly are refused, not reinterpreted
        nx, nu = prob.nx, prob.nu
        z = lambda *sh: torch.zeros(sh, dtype=torch.float64).cuda()
        good = [z(4, nx, nx), z(4, nu, nx), z(4, nx, nx), z(4, nu, nu)]
        for i, bad in ((0, torch.zeros((4, nx, nx), dtype=torch.int64).cuda()), (1, z(4, nx, nu)), (2, z(4, nx, 2 * nx)[:, :, ::2]), (3, z(3, nu, nu))):
            args = list(good)
            args[i] = bad
            with pytest.raises(pkg.TinyMPCError) as ei:
                s.set_model_batch(*args)
            assert ei.value.code == E
        with pytest.raises(pkg.TinyMPCError) as ei:  # mixed host and device
            s.set_model_batch(good[0], good[1], np.zeros((nx, nx, 4)), good[3])
        assert ei.value.code == E
    assert "per-instance-models" not in s.jit_info()
    s.reset()


def test_two_shards_equal_one_handle(pkg):
    P = pkg.problems
    prob, n = P.quadrotor(50), 402
    M = _models(prob, n, seed=9, fdyn=True)
    x0s = _x0s(prob, n)
    whole = _solver(pkg, prob, n)
    _set_models(whole, M)
    whole.set_x0_batch(x0s)
    whole.solve()
    h = n // 2
    for lo, hi in ((0, h), (h, n)):
        part = _solver(pkg, prob, hi - lo)
        args, kw = M.verb(lo, hi)
        part.set_model_batch(*args, **kw)
        part.set_x0_batch(np.asfortranarray(x0s[:, lo:hi]))
        part.solve()
        np.testing.assert_array_equal(part.get_solution_batch()["controls"], whole.get_solution_batch(lo, hi - lo)["controls"])
        np.testing.assert_array_equal(part.get_solution_batch()["states"], whole.get_solution_batch(lo, hi - lo)["states"])
        np.testing.assert_array_equal(part.get_stats_batch()["iter"], whole.get_stats_batch()["iter"][lo:hi])
        np.testing.assert_array_equal(part.get_cache_batch()["Pinf"], whole.get_cache_batch(lo, hi - lo)["Pinf"])
        part.reset()
    whole.reset()


def test_single_instance_handle_acts_on_instance_zero(pkg):
    P = pkg.problems
    prob = P.quadrotor(50)
    M = _models(prob, 1, seed=10, fdyn=True)
    s = _solver(pkg, prob, 1)
    _set_models(s, M)
    assert "per-instance-models" in s.jit_info() and s.launch_info()["layout"] == "A"
    pb = M.problem(prob, 0)
    orc = _oracle(pb)
    xr = 0.1 * np.ones((prob.nx, prob.N))
    for rnd in range(3):
        if rnd == 2:  # a reference set on the single-instance handle after the mode began reaches the instance's rows
            s.set_x_ref(xr)
            orc.set_x_ref(xr)
        x0 = prob.x0 * (1.0 - 0.3 * rnd)
        s.set_x0(x0)
        s.solve()
        orc.set_x0(x0)
        orc.solve()
        assert s.get_stats()["iter"] == orc.stats()["iter"], rnd
        assert rel_err(s.get_solution()["controls"], orc.solution()[1]) < TOL, rnd
        assert rel_err(s.get_solution()["states"], orc.solution()[0]) < TOL, rnd
    s.clear_model_batch()
    assert "per-instance-models" not in s.jit_info()
    s.reset()


def _expect_unsupported(pkg, s):
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.solve()
    assert ei.value.code == pkg._lib.ERR_UNSUPPORTED
    assert "per-instance models" in str(ei.value) and "tinympc_clear_model_batch" in str(ei.value), str(ei.value)


def test_refusals_and_recovery(pkg):
    P = pkg.problems
    prob, batch = P.quadrotor(20), 64
    M = _models(prob, batch, seed=11)
    # adaptive rho, set after the models
    s = _solver(pkg, prob, batch)
    _set_models(s, M)
    s.set_x0_batch(_x0s(prob, batch))
    s.solve()
    s.update_settings(adaptive_rho=1)
    _expect_unsupported(pkg, s)
    s.clear_model_batch()  # shared again: the adaptive-rho kernel may run
    s.solve()
    s.reset()
    # cone constraints set after the models
    s = _solver(pkg, prob, batch)
    _set_models(s, M)
    s.set_x0_batch(_x0s(prob, batch))
    s.set_cone_constraints(np.array([0]), np.array([3]), np.array([0.5]), np.array([0]), np.array([2]), np.array([1.0]))
    s.update_settings(en_state_soc=1)
    _expect_unsupported(pkg, s)
    s.set_x_ref_batch(np.zeros((prob.nx, batch)))  # with per-instance references on too, the message names both
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.solve()
    assert "per-instance references" in str(ei.value) and "per-instance models" in str(ei.value)
    s.set_x_ref(np.zeros((prob.nx, prob.N)))
    s.clear_model_batch()
    s.solve()
    s.reset()
    # nx + nu > 64 (layout M)
    rng = np.random.default_rng(3)
    nx, nu, N = 60, 8, 6
    big = P.Problem("big", np.eye(nx) + 0.01 * rng.standard_normal((nx, nx)), 0.1 * rng.standard_normal((nx, nu)), np.eye(nx), np.eye(nu), N, 2.0,
                    rng.standard_normal(nx))
    s = _solver(pkg, big, 4)
    _set_models(s, _shared_models(big, 4))
    s.set_x0_batch(np.zeros((nx, 4), order="F"))
    _expect_unsupported(pkg, s)
    s.clear_model_batch()
    s.solve()
    s.reset()


def test_invalid_arguments_are_refused(pkg):
    P = pkg.problems
    prob, batch = P.quadrotor(20), 64
    s = _solver(pkg, prob, batch)
    L, E = pkg.load_library(), pkg._lib.ERR_INVALID_INPUT
    buf = np.zeros(prob.nx * prob.nx * batch)
    p = buf.ctypes.data_as(pkg._lib.c_double_p)
    f = L.tinympc_set_model_batch
    assert f(s._h, p, p, p, p, p, batch - 2, 4) == E    # range beyond the batch
    assert f(s._h, p, p, p, p, p, -1, 2) == E           # negative first
    assert f(s._h, p, p, p, p, p, 0, 0) == E            # count < 1
    assert f(s._h, p, p, p, p, p, 0, -1) == E
    for i in (0, 1, 3, 4):                              # NULL A, B, Q, R (fdyn may be NULL)
        args = [p, p, p, p, p]
        args[i] = None
        assert f(s._h, *args, 0, 4) == E
        assert L.tinympc_set_model_batch_device(s._h, *[None if j == i else C.c_void_p(buf.ctypes.data) for j in range(5)], 0, 4) == E
    assert L.tinympc_get_cache_batch(s._h, p, p, p, p, None, batch - 1, 2) == E
    nx, nu = prob.nx, prob.nu
    with pytest.raises(pkg.TinyMPCError) as ei:  # a wrong shape
        s.set_model_batch(np.zeros((nx + 1, nx, 4)), np.zeros((nx, nu, 4)), np.zeros((nx, nx, 4)), np.zeros((nu, nu, 4)))
    assert ei.value.code == E
    with pytest.raises(pkg.TinyMPCError) as ei:  # counts that differ
        s.set_model_batch(np.zeros((nx, nx, 4)), np.zeros((nx, nu, 3)), np.zeros((nx, nx, 4)), np.zeros((nu, nu, 4)))
    assert ei.value.code == E
    # nothing of it switched the handle to per-instance mode
    assert "per-instance-models" not in s.jit_info()
    x0s = _x0s(prob, batch)
    ref = _solver(pkg, prob, batch)
    for h in (s, ref):
        h.set_x0_batch(x0s)
        h.solve()
    _same(s, ref)
    s.reset()
    ref.reset()
