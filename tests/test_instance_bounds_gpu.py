"""Per-instance box bounds of batched handles (tinympc_set_bound_constraints_batch and its _device form): every instance solves what it
would solve alone after set_bound_constraints with its own bounds -- checked against the oracle per instance, bit for bit against the
shared-bounds handle where the bounds coincide, together with per-instance references, across partial ranges, mode switches, the enable
flags, closed-loop ticks, device input and sharding; and the configurations no kernel carries are refused, never solved with the shared
bounds."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest
from conftest import rel_err

import pyoracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-9
SETTINGS = dict(max_iter=100, abs_pri_tol=1e-4, abs_dua_tol=1e-4)


def _wide(P, nx, nu, N):
    rng = np.random.default_rng(nx * 100 + nu)
    A = np.eye(nx) + 0.03 * rng.standard_normal((nx, nx))
    B = 0.1 * rng.standard_normal((nx, nu))
    prob = P.Problem("wide", A, B, np.diag(rng.uniform(1, 10, nx)), np.diag(rng.uniform(0.5, 2, nu)), N, 2.0, rng.standard_normal(nx))
    prob.u_min, prob.u_max = np.full(nu, -0.3), np.full(nu, 0.3)
    prob.x_min, prob.x_max = np.full(nx, -2.0), np.full(nx, 2.0)
    return prob


CASES = {  # name -> (problem, batch)
    "quadrotor50": (lambda P: P.quadrotor(50), 1301),
    "quadrotor30": (lambda P: P.quadrotor(30), 1301),
    "cartpole20": (lambda P: P.cartpole(20, True), 37),
    "wide32": (lambda P: _wide(P, 24, 8, 20), 37),
    "wide64": (lambda P: _wide(P, 48, 16, 12), 21),
    "quadrotor120": (lambda P: P.quadrotor(120), 70),
}
# boxes on layout D: compiled in (quadrotor N=50), or run-time specialised (the others; not with TINYMPC_JIT=0)
BOX_ON_D = {"1": {"quadrotor50", "quadrotor30", "wide32", "wide64"}, "0": {"quadrotor50"}}


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


def _bounds(prob, batch, form, seed=1):
    """Random per-instance limits inside the shared ones (finite where the shared ones are not), tight enough on the inputs to bind.
    -> (what the verb takes: four arrays, the per-instance expanded nx x N x batch / nu x (N-1) x batch bounds)."""
    rng = np.random.default_rng(seed)
    nx, nu, N = prob.nx, prob.nu, prob.N
    xmn, xmx, umn, umx = (b[:, 0] for b in prob.expanded_bounds())

    def inside(lo, hi, dim, frac):
        lo = np.where(np.abs(lo) > 1e10, -3.0, lo)
        hi = np.where(np.abs(hi) > 1e10, 3.0, hi)
        return (lo[:, None] * rng.uniform(*frac, (dim, batch)), hi[:, None] * rng.uniform(*frac, (dim, batch)))

    xl, xh = inside(xmn, xmx, nx, (0.4, 0.75))
    ul, uh = inside(umn, umx, nu, (0.15, 0.5))
    if form == "box":
        full = (np.repeat(xl[:, None, :], N, axis=1), np.repeat(xh[:, None, :], N, axis=1),
                np.repeat(ul[:, None, :], N - 1, axis=1), np.repeat(uh[:, None, :], N - 1, axis=1))
        return (xl, xh, ul, uh), full
    ph = rng.uniform(0, 6, batch)
    fx = 1.0 + 0.3 * np.sin(0.4 * np.arange(N)[:, None] + ph[None, :])  # N x batch, below 1 / 0.75
    fu = fx[: N - 1]
    full = (xl[:, None, :] * fx[None], xh[:, None, :] * fx[None], ul[:, None, :] * fu[None], uh[:, None, :] * fu[None])
    return full, full


def _refs(prob, batch, form, seed=1):
    rng = np.random.default_rng(seed)
    nx, nu, N = prob.nx, prob.nu, prob.N
    gx, gu = 0.4 * rng.standard_normal((nx, batch)), 0.05 * rng.standard_normal((nu, batch))
    if form == "goal":
        return (gx, gu), (np.repeat(gx[:, None, :], N, axis=1), np.repeat(gu[:, None, :], N - 1, axis=1))
    t = np.linspace(0.0, 1.0, N)
    X = gx[:, None, :] * (1.0 + 0.5 * np.sin(3.0 * t + np.arange(nx)[:, None]))[:, :, None]
    U = gu[:, None, :] * np.cos(2.0 * t[: N - 1])[None, :, None]
    return (X, U), (X, U)


def _x0s(prob, batch, scale=1.0, seed=2):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(prob.x0[:, None] * scale + 0.2 * rng.standard_normal((prob.nx, batch)))


def _oracle(prob, full, b, Xb=None, Ub=None, settings=SETTINGS):
    """The oracle of instance b: the problem with instance b's expanded bounds (and references)."""
    pb = dataclasses.replace(prob, x_min=full[0][:, :, b], x_max=full[1][:, :, b], u_min=full[2][:, :, b], u_max=full[3][:, :, b])
    orc = O.OraclePort(pb).load_problem(pb, settings)
    if Xb is not None:
        orc.set_x_ref(Xb)
    if Ub is not None:
        orc.set_u_ref(Ub)
    return orc


def _check(s, orcs, x0s, tag):
    sol, st = s.get_solution_batch(), s.get_stats_batch()
    for b, orc in orcs.items():
        orc.set_x0(x0s[:, b])
        orc.solve()
        assert st["iter"][b] == orc.stats()["iter"], (tag, b)
        assert st["status"][b] == orc.stats()["status"], (tag, b)
        assert rel_err(sol["states"][:, :, b], orc.solution()[0]) < TOL, (tag, b)
        assert rel_err(sol["controls"][:, :, b], orc.solution()[1]) < TOL, (tag, b)


def _binds(s, full, samples, tag):
    """The controls of the sampled instances respect their OWN bounds, at least one of them touches its own bound, and at least one
    would break another sampled instance's tighter bound: the solve did not run on shared (or someone else's) bounds."""
    u = s.get_solution_batch()["controls"]
    umin, umax = full[2], full[3]
    touched = broken = False
    for b in samples:
        assert np.all(u[:, :, b] <= umax[:, :, b] + 1e-12) and np.all(u[:, :, b] >= umin[:, :, b] - 1e-12), (tag, b)
        touched |= bool(np.any(np.abs(u[:, :, b] - umax[:, :, b]) < 1e-12) or np.any(np.abs(u[:, :, b] - umin[:, :, b]) < 1e-12))
        for c in samples:
            if c != b:
                broken |= bool(np.any(u[:, :, b] > umax[:, :, c] + 1e-9) or np.any(u[:, :, b] < umin[:, :, c] - 1e-9))
    assert touched and broken, tag


def _sample(batch):
    return sorted({0, 1, batch // 2, batch - 2, batch - 1})


@pytest.mark.parametrize("jit", ["1", "0"])
@pytest.mark.parametrize("form", ["box", "knot"])
@pytest.mark.parametrize("case", list(CASES))
def test_each_instance_matches_the_oracle_with_its_own_bounds(pkg, monkeypatch, case, form, jit):
    monkeypatch.setenv("TINYMPC_JIT", jit)
    prob, batch = CASES[case][0](pkg.problems), CASES[case][1]
    s = _solver(pkg, prob, batch)
    verb, full = _bounds(prob, batch, form)
    s.set_bound_constraints_batch(*verb)
    samples = _sample(batch)
    orcs = {b: _oracle(prob, full, b) for b in samples}
    for rnd in range(3):  # a cold start, then two warm starts
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        s.set_x0_batch(x0s)
        s.solve()
        _check(s, orcs, x0s, (case, form, rnd))
        if rnd == 0:
            _binds(s, full, samples, (case, form))
    info = s.jit_info()
    assert "per-instance-bounds" in info and "per-instance-refs" not in info, info
    if form == "knot":
        assert s.launch_info()["layout"] == "A"
    elif case in BOX_ON_D[jit]:  # a batch layout D serves: the boxes run there
        assert s.launch_info()["layout"] == "D" and "goal" in info and "refused" not in info, info
        assert ("compiled-in" in info) == (case == "quadrotor50"), info
    s.reset()


@pytest.mark.parametrize("case", ["quadrotor50-box", "quadrotor30-box", "wide32-box", "quadrotor50", "cartpole20", "wide64", "quadrotor120"])
def test_per_instance_equal_to_shared_is_bit_identical(pkg, monkeypatch, case):
    """Every instance given the shared bounds: the same numbers as the shared-bounds handle on the same layout -- D for boxes (one per
    instance, the goal form), A for bounds per knot."""
    P = pkg.problems
    box = case.endswith("-box")
    name = case.replace("-box", "")
    prob, batch = CASES[name][0](P), CASES[name][1] if box else min(CASES[name][1], 300)
    _, full = _bounds(prob, 1, "box" if box else "knot", seed=5)
    prob.x_min, prob.x_max, prob.u_min, prob.u_max = (a[:, :, 0] if not box else a[:, 0, 0] for a in full)
    if not box:
        monkeypatch.setenv("TINYMPC_LAYOUT", "A")
    shared = _solver(pkg, prob, batch)
    monkeypatch.delenv("TINYMPC_LAYOUT", raising=False)
    inst = _solver(pkg, prob, batch)
    if box:
        inst.set_bound_constraints_batch(*(np.repeat(a[:, 0, :], batch, axis=1) for a in full))
    else:
        inst.set_bound_constraints_batch(*(np.repeat(a, batch, axis=2) for a in full))
    for rnd in range(3):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        for h in (shared, inst):
            h.set_x0_batch(x0s)
            h.solve()
        a, b = shared.get_solution_batch(), inst.get_solution_batch()
        sa, sb = shared.get_stats_batch(), inst.get_stats_batch()
        np.testing.assert_array_equal(a["states"], b["states"])
        np.testing.assert_array_equal(a["controls"], b["controls"])
        for k in sa:
            np.testing.assert_array_equal(sa[k], sb[k])
    assert shared.launch_info()["layout"] == inst.launch_info()["layout"] == ("D" if box else "A")
    assert "per-instance-bounds" not in shared.jit_info() and "per-instance-bounds" in inst.jit_info()
    shared.reset()
    inst.reset()


@pytest.mark.parametrize("refs,bounds,layout", [("goal", "box", "D"), ("trajectory", "box", "A"), ("goal", "knot", "A"),
                                                ("trajectory", "knot", "A")])
def test_combined_with_per_instance_references(pkg, refs, bounds, layout):
    P = pkg.problems
    prob, batch = P.quadrotor(50), 1301  # (a batch layout D serves)
    s = _solver(pkg, prob, batch)
    (vx, vu), (X, U) = _refs(prob, batch, refs, seed=3)
    verb, full = _bounds(prob, batch, bounds, seed=4)
    s.set_x_ref_batch(vx)
    s.set_bound_constraints_batch(*verb)  # (either order)
    s.set_u_ref_batch(vu)
    samples = _sample(batch)
    orcs = {b: _oracle(prob, full, b, X[:, :, b], U[:, :, b]) for b in samples}
    for rnd in range(2):
        x0s = _x0s(prob, batch, 1.0 - 0.3 * rnd, seed=rnd)
        s.set_x0_batch(x0s)
        s.solve()
        _check(s, orcs, x0s, (refs, bounds, rnd))
    info = s.jit_info()
    assert "per-instance-refs" in info and "per-instance-bounds" in info, info
    assert s.launch_info()["layout"] == layout
    s.reset()


def test_partial_ranges_return_to_shared_and_enable_flags(pkg):
    P = pkg.problems
    prob, batch = P.quadrotor(50), 200
    s = _solver(pkg, prob, batch)
    (bl, bh, cl, ch), fb = _bounds(prob, batch, "box", seed=7)
    kn, fk = _bounds(prob, batch, "knot", seed=8)
    s.set_bound_constraints_batch(bl[:, 10:60], bh[:, 10:60], cl[:, 10:60], ch[:, 10:60], first=10)
    s.set_bound_constraints_batch(*(a[:, :, 100:130] for a in kn), first=100)
    s.set_bound_constraints_batch(bl[:, 55:57], bh[:, 55:57], cl[:, 55:57], ch[:, 55:57], first=55)  # overrides a part of the first range
    shared = tuple(np.repeat(a[:, :, None], batch, axis=2) for a in prob.expanded_bounds())
    want = tuple(a.copy() for a in shared)
    for w, a, k in zip(want, fb, fk):
        w[:, :, 10:60] = a[:, :, 10:60]
        w[:, :, 100:130] = k[:, :, 100:130]
    samples = [0, 9, 10, 30, 55, 56, 59, 60, 99, 100, 129, 130, 199]
    orcs = {b: _oracle(prob, want, b) for b in samples}
    x0s = _x0s(prob, batch)
    s.set_x0_batch(x0s)
    s.solve()
    _check(s, orcs, x0s, "partial")
    assert s.launch_info()["layout"] == "A"  # (one range per knot: the whole batch on layout A)
    # kept across reset_workspace, update_settings and the shared reference verbs
    s.reset_workspace()
    s.update_settings(max_iter=80)
    s.set_u_ref(np.zeros((prob.nu, prob.N - 1)))
    settings = dict(SETTINGS, max_iter=80)
    orcs = {b: _oracle(prob, want, b, settings=settings) for b in samples}
    s.solve()
    _check(s, orcs, x0s, "after reset")
    # the enable flags switch a family off for every instance (and back on)
    for flags in (dict(en_state_bound=0, en_input_bound=1), dict(en_state_bound=1, en_input_bound=0), dict(en_state_bound=1, en_input_bound=1)):
        s.update_settings(**flags)
        st = dict(settings, **flags)
        orcs = {b: _oracle(prob, want, b, settings=st) for b in (0, 30, 56, 100, 129)}
        s.reset_workspace()
        s.solve()
        _check(s, orcs, x0s, flags)
    # set_bound_constraints returns every instance to shared bounds
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    assert "per-instance-bounds" not in s.jit_info()
    ref = _solver(pkg, prob, batch, settings)
    for h in (s, ref):
        h.reset_workspace()
        h.set_x0_batch(x0s)
        h.solve()
    np.testing.assert_array_equal(s.get_solution_batch()["controls"], ref.get_solution_batch()["controls"])
    s.reset()
    ref.reset()


def _library_hip_runtime(pkg):
    """The path of the HIP runtime the library is linked against, as this process mapped it (torch may carry a runtime of its own)."""
    pkg.load_library()
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    own = sorted(p for p in paths if "/torch/" not in p)
    assert own, paths
    return own[0]


class _DeviceArrays:
    """Device memory of the current HIP device, filled from numpy through the HIP runtime the library itself uses (so that the device
    verb is exercised whether or not torch sees the GPU)."""

    def __init__(self, pkg):
        import ctypes as C
        self.C = C
        self.hip = C.CDLL(_library_hip_runtime(pkg))
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.ptrs = []

    def put(self, a):
        """a (rows x [cols x] count, the verb's column-major layout) -> a device pointer holding the same bytes."""
        C = self.C
        h = np.ascontiguousarray(np.asarray(a, dtype=np.float64).T)
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), h.nbytes) == 0
        self.ptrs.append(p)
        assert self.hip.hipMemcpy(p, C.c_void_p(h.ctypes.data), h.nbytes, 1) == 0  # hipMemcpyHostToDevice
        return p

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


def _torch_gpu():
    try:
        import torch
    except ImportError:
        return None
    return torch if torch.cuda.is_available() else None


@pytest.mark.parametrize("batch", [256, 4096])
def test_closed_loop_with_moving_boxes_from_device(pkg, batch):
    """8 ticks of mpc_step_batch; every tick each instance's box moves and is re-sent through the _device form -- from a torch tensor
    where torch sees the GPU, from device memory filled through the HIP runtime otherwise."""
    torch = _torch_gpu()
    P = pkg.problems
    prob = P.quadrotor(50)
    T = 8
    settings = dict(max_iter=50, abs_pri_tol=1e-4, abs_dua_tol=1e-4)
    rng = np.random.default_rng(11)
    width = rng.uniform(0.1, 0.3, (prob.nu, batch))
    s = _solver(pkg, prob, batch, settings)
    L = pkg.load_library()
    dev = _DeviceArrays(pkg)
    samples = [0, batch // 3, batch - 1]
    x = _x0s(prob, batch)
    xl, xh = np.full((prob.nx, batch), -4.0), np.full((prob.nx, batch), 4.0)
    orcs = {}  # one oracle per sampled instance, warm-started from tick to tick like the handle
    for k in range(T):
        uh = width * (1.0 + 0.5 * np.sin(0.7 * k + np.arange(batch)[None, :]))  # each instance's box moves every tick
        ul = -uh
        if torch is not None:
            s.set_bound_constraints_batch(*(torch.from_numpy(np.ascontiguousarray(a.T)).cuda() for a in (xl, xh, ul, uh)))  # (count, rows)
        else:
            assert L.tinympc_set_bound_constraints_batch_device(s._h, *(dev.put(a) for a in (xl, xh, ul, uh)), 1, 0, batch) == 0
            dev.free()  # (the copies have completed when the verb returns)
        u = s.mpc_step(x)
        if k == 0:
            info = s.jit_info()
            assert "per-instance-bounds" in info, info
        st = s.get_stats_batch()
        for b in samples:
            full = tuple(np.repeat(a[:, None, b:b + 1], n, axis=1) for a, n in ((xl, prob.N), (xh, prob.N), (ul, prob.N - 1), (uh, prob.N - 1)))
            if b not in orcs:
                orcs[b] = _oracle(prob, full, 0, settings=settings)
            orc = orcs[b]
            orc.set_bound_constraints(*(f[:, :, 0] for f in full))
            orc.set_x0(x[:, b])
            orc.solve()
            assert st["iter"][b] == orc.stats()["iter"], (k, b)
            assert rel_err(u[:, b], orc.solution()[1][:, 0]) < TOL, (k, b)
            assert np.all(np.abs(u[:, b]) <= uh[:, b] + 1e-12), (k, b)
        x = np.asfortranarray(prob.A @ x + prob.B @ u)
    s.reset()


def test_device_input_matches_host_input(pkg):
    import ctypes as C
    P = pkg.problems
    prob, batch = P.quadrotor(50), 300
    x0s = _x0s(prob, batch)
    torch = _torch_gpu()
    L, E = pkg.load_library(), pkg._lib.ERR_INVALID_INPUT
    dev = _DeviceArrays(pkg)
    out = []
    for form, cols in (("box", 1), ("knot", prob.N)):
        verb, _ = _bounds(prob, batch, form, seed=6)
        h, d = _solver(pkg, prob, batch), _solver(pkg, prob, batch)
        h.set_bound_constraints_batch(*verb)
        assert L.tinympc_set_bound_constraints_batch_device(d._h, *(dev.put(a) for a in verb), cols, 0, batch) == 0
        handles = [h, d]
        if torch is not None:  # the Python method's tensor form: (count, [N,] rows)
            t = _solver(pkg, prob, batch)
            t.set_bound_constraints_batch(*(torch.from_numpy(np.ascontiguousarray(a.T)).cuda() for a in verb))
            handles.append(t)
        for q in handles:
            q.set_x0_batch(x0s)
            q.solve()
        for q in handles[1:]:
            assert "per-instance-bounds" in q.jit_info()
            np.testing.assert_array_equal(h.get_solution_batch()["states"], q.get_solution_batch()["states"])
            np.testing.assert_array_equal(h.get_solution_batch()["controls"], q.get_solution_batch()["controls"])
            np.testing.assert_array_equal(h.get_stats_batch()["iter"], q.get_stats_batch()["iter"])
        out.append(h.get_solution_batch()["controls"])
        for q in handles:
            q.reset()
    dev.free()
    assert not np.array_equal(out[0], out[1])
    # host memory through the device verb is refused, and so is any one device pointer that is host memory
    s = _solver(pkg, prob, batch)
    buf = np.zeros(prob.nx * batch)
    hp = C.c_void_p(buf.ctypes.data)
    assert L.tinympc_set_bound_constraints_batch_device(s._h, hp, hp, hp, hp, 1, 0, 4) == E
    good = [dev.put(np.zeros((r, batch))) for r in (prob.nx, prob.nx, prob.nu, prob.nu)]
    assert L.tinympc_set_bound_constraints_batch_device(s._h, good[0], good[1], good[2], hp, 1, 0, 4) == E
    dev.free()
    if torch is not None:  # tensors the library cannot read correctly are refused, not reinterpreted
        good = [torch.zeros((batch, r), dtype=torch.float64).cuda() for r in (prob.nx, prob.nx, prob.nu, prob.nu)]
        for i, bad in ((0, torch.zeros((batch, prob.nx), dtype=torch.int64).cuda()), (2, torch.zeros((prob.nu, batch), dtype=torch.float64).cuda()),
                       (1, torch.zeros((batch, 2 * prob.nx), dtype=torch.float64).cuda()[:, ::2])):
            args = list(good)
            args[i] = bad
            with pytest.raises(pkg.TinyMPCError) as ei:
                s.set_bound_constraints_batch(*args)
            assert ei.value.code == E
    assert "per-instance-bounds" not in s.jit_info()
    s.reset()


def test_two_shards_equal_one_handle(pkg):
    P = pkg.problems
    prob, n = P.quadrotor(50), 402
    for form in ("box", "knot"):
        verb, _ = _bounds(prob, n, form, seed=9)
        x0s = _x0s(prob, n)
        whole = _solver(pkg, prob, n)
        whole.set_bound_constraints_batch(*verb)
        whole.set_x0_batch(x0s)
        whole.solve()
        h = n // 2
        for lo, hi in ((0, h), (h, n)):
            part = _solver(pkg, prob, hi - lo)
            part.set_bound_constraints_batch(*(np.ascontiguousarray(a[..., lo:hi]) for a in verb))
            part.set_x0_batch(np.asfortranarray(x0s[:, lo:hi]))
            part.solve()
            np.testing.assert_array_equal(part.get_solution_batch()["controls"], whole.get_solution_batch(lo, hi - lo)["controls"])
            np.testing.assert_array_equal(part.get_stats_batch()["iter"], whole.get_stats_batch()["iter"][lo:hi])
            part.reset()
        whole.reset()


def test_batch_one_is_the_shared_verb(pkg):
    P = pkg.problems
    prob = P.quadrotor(50)
    for form in ("box", "knot"):
        verb, full = _bounds(prob, 1, form, seed=10)
        a, b = _solver(pkg, prob, 1), _solver(pkg, prob, 1)
        a.set_bound_constraints_batch(*verb)
        b.set_bound_constraints(*(f[:, :, 0] for f in full))
        for q in (a, b):
            q.set_x0(prob.x0)
            q.solve()
        np.testing.assert_array_equal(a.get_solution()["controls"], b.get_solution()["controls"])
        assert "per-instance-bounds" not in a.jit_info()
        a.reset()
        b.reset()


def _expect_unsupported(pkg, s, what="per-instance bounds"):
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.solve()
    assert ei.value.code == pkg._lib.ERR_UNSUPPORTED
    assert what in str(ei.value)


def test_refusals_and_recovery(pkg):
    P = pkg.problems
    prob, batch = P.quadrotor(20), 64
    verb, _ = _bounds(prob, batch, "box")
    # adaptive rho, set after the bounds
    s = _solver(pkg, prob, batch)
    s.set_bound_constraints_batch(*verb)
    s.set_x0_batch(_x0s(prob, batch))
    s.solve()
    s.update_settings(adaptive_rho=1)
    _expect_unsupported(pkg, s)
    # with per-instance references on too, their refusal comes first
    s.set_x_ref_batch(np.zeros((prob.nx, batch)))
    _expect_unsupported(pkg, s, "per-instance references")
    s.set_x_ref(np.zeros((prob.nx, prob.N)))
    _expect_unsupported(pkg, s)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)  # shared again: the adaptive-rho kernel may run
    s.solve()
    s.reset()
    # cone constraints set after the bounds, then cleared with the shared verb
    s = _solver(pkg, prob, batch)
    s.set_bound_constraints_batch(*verb)
    s.set_x0_batch(_x0s(prob, batch))
    s.set_cone_constraints(np.array([0]), np.array([3]), np.array([0.5]), np.array([0]), np.array([2]), np.array([1.0]))
    s.update_settings(en_state_soc=1)
    _expect_unsupported(pkg, s)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    s.solve()
    s.reset()
    # nx + nu > 64 (layout M)
    rng = np.random.default_rng(3)
    nx, nu, N = 60, 8, 6
    big = P.Problem("big", np.eye(nx) + 0.01 * rng.standard_normal((nx, nx)), 0.1 * rng.standard_normal((nx, nu)), np.eye(nx), np.eye(nu), N, 2.0,
                    rng.standard_normal(nx))
    s = _solver(pkg, big, 4)
    s.set_bound_constraints_batch(np.full((nx, 4), -1.0), np.full((nx, 4), 1.0), np.full((nu, 4), -1.0), np.full((nu, 4), 1.0))
    s.set_x0_batch(np.zeros((nx, 4), order="F"))
    _expect_unsupported(pkg, s)
    s.set_bound_constraints(np.full(nx, -1.0), np.full(nx, 1.0), np.full(nu, -1.0), np.full(nu, 1.0))
    s.solve()
    s.reset()


def test_invalid_arguments_are_refused(pkg):
    import ctypes as C
    P = pkg.problems
    prob, batch = P.quadrotor(20), 64
    s = _solver(pkg, prob, batch)
    L, E = pkg.load_library(), pkg._lib.ERR_INVALID_INPUT
    N = prob.N
    buf = np.zeros(prob.nx * N * batch)
    p = buf.ctypes.data_as(pkg._lib.c_double_p)
    f = L.tinympc_set_bound_constraints_batch
    assert f(s._h, p, p, p, p, N + 1, 0, 4) == E        # cols neither N nor 1
    assert f(s._h, p, p, p, p, N - 1, 0, 4) == E
    assert f(s._h, p, p, p, p, 1, batch - 2, 4) == E    # range beyond the batch
    assert f(s._h, p, p, p, p, 1, -1, 2) == E           # negative first
    assert f(s._h, p, p, p, p, 1, 0, -1) == E           # negative count
    for i in range(4):                                  # NULL
        args = [p, p, p, p]
        args[i] = None
        assert f(s._h, *args, 1, 0, 4) == E
        assert L.tinympc_set_bound_constraints_batch_device(s._h, *[None if j == i else C.c_void_p(buf.ctypes.data) for j in range(4)], 1, 0, 4) == E
    with pytest.raises(pkg.TinyMPCError) as ei:
        s.set_bound_constraints_batch(np.zeros((prob.nx + 1, 4)), np.zeros((prob.nx, 4)), np.zeros((prob.nu, 4)), np.zeros((prob.nu, 4)))
    assert ei.value.code == E
    with pytest.raises(pkg.TinyMPCError) as ei:  # mixed forms
        s.set_bound_constraints_batch(np.zeros((prob.nx, 4)), np.zeros((prob.nx, N, 4)), np.zeros((prob.nu, 4)), np.zeros((prob.nu, 4)))
    assert ei.value.code == E
    # nothing of it switched the handle to per-instance mode
    assert "per-instance-bounds" not in s.jit_info()
    x0s = _x0s(prob, batch)
    ref = _solver(pkg, prob, batch)
    for h in (s, ref):
        h.set_x0_batch(x0s)
        h.solve()
    np.testing.assert_array_equal(s.get_solution_batch()["controls"], ref.get_solution_batch()["controls"])
    s.reset()
    ref.reset()
