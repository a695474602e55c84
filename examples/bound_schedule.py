"""A bound schedule: 512 quadrotors whose input limits RAMP UP over the horizon, each at its own rate -- a fleet leaving a standstill
with actuators that are only allowed a fraction of their authority at first (knot 0) and all of it from some knot on. Every instance's
limits differ per knot and per instance: one call, set_bound_constraints_batch with nu x (N-1) x batch input limits.

    python bound_schedule.py [--no-prepare]
The handle is set up on the throughput layout (TINYMPC_LAYOUT=D, unless the environment names another) and calls prepare(), which
welcomes run-time specialised kernels: the schedules then run on layout D's per-knot bounds form (every wavefront's own clamp rows in
its LDS region). With --no-prepare the same solve runs on layout A; the results agree to rounding and the kernel line says which ran."""
import os
import sys

import numpy as np
from _common import TinyMPC, problems

prepare = "--no-prepare" not in sys.argv[1:]
os.environ.setdefault("TINYMPC_LAYOUT", "D")

prob = problems.quadrotor(20)
batch = 512
nx, nu, N = prob.nx, prob.nu, prob.N
rng = np.random.default_rng(0)

# shared limits u_min / u_max (hover-relative thrust); instance b may use the fraction f_b(k) of them at knot k:
# 15 % at knot 0, rising linearly to 100 % after `rise` knots -- a slow fleet (rise = 16) to a fast one (rise = 3)
xmn, xmx, umn, umx = prob.expanded_bounds()  # nx x N, nu x (N-1)
rise = rng.uniform(3.0, 16.0, batch)
frac = np.clip(0.15 + 0.85 * np.arange(N - 1)[:, None] / rise[None, :], 0.0, 1.0)  # (N-1) x batch
u_lo = np.asfortranarray(umn[:, :, None] * frac[None])
u_hi = np.asfortranarray(umx[:, :, None] * frac[None])
x_lo = np.asfortranarray(np.repeat(xmn[:, :, None], batch, axis=2))
x_hi = np.asfortranarray(np.repeat(xmx[:, :, None], batch, axis=2))

solver = TinyMPC()
solver.setup(prob.A, prob.B, prob.Q, prob.R, N, batch=batch, rho=prob.rho, max_iter=200, abs_pri_tol=1e-4, abs_dua_tol=1e-4)
solver.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
if prepare:
    solver.prepare()
solver.set_bound_constraints_batch(x_lo, x_hi, u_lo, u_hi)  # one column per knot: every instance's own schedule

# every vehicle starts 0.8 m to 1.5 m from the origin it is asked to reach: the first controls want more than the early limits allow
x0 = np.zeros((nx, batch), order="F")
x0[:3] = rng.uniform(0.8, 1.5, (3, batch)) * rng.choice([-1.0, 1.0], (3, batch))
solver.set_x0_batch(x0)
solver.solve()
print("kernel:", solver.launch_info()["layout"], "|", solver.jit_info())

u = solver.get_solution_batch()["controls"]  # nu x (N-1) x batch
it = solver.get_stats_batch()["iter"]
assert np.all(u <= u_hi + 1e-12) and np.all(u >= u_lo - 1e-12), "a control left its instance's schedule"
at_limit = (np.abs(u - u_hi) < 1e-12) | (np.abs(u - u_lo) < 1e-12)
slow, fast = rise > 12.0, rise < 5.0
print(f"iterations: {it.mean():.1f} on average, {it.max()} at most")
print(f"controls at their scheduled limit: {at_limit.any(axis=0).sum(axis=0).mean():.1f} of {N - 1} knots on average; "
      f"slow fleet (rise > 12 knots, {slow.sum()} vehicles) {at_limit[:, :, slow].any(axis=0).sum(axis=0).mean():.1f}, "
      f"fast fleet (rise < 5, {fast.sum()}) {at_limit[:, :, fast].any(axis=0).sum(axis=0).mean():.1f}")
print(f"largest first control: {np.abs(u[:, 0, :]).max():.4f} (15 % of the shared limit: {0.15 * np.abs(umx[:, 0]).max():.4f})")
assert at_limit[:, 0, :].any(), "no vehicle used all of its first knot's authority"
assert at_limit[:, :, slow].any(axis=0).sum(axis=0).mean() > at_limit[:, :, fast].any(axis=0).sum(axis=0).mean(), "the slower ramps bind for longer"
solver.reset()
