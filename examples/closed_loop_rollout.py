"""Closed-loop rollout on the device: 512 quadrotors, each following its own figure-eight under process noise, for 120 ticks -- in ONE
call. Every instance's track is uploaded once and moves by auto-advance; the plant x+ = A x + B u + w runs on the device behind each
tick's solve (rollout), so no state, control or statistic crosses to the host until the logs come back at the end. The host loop this
replaces -- mpc_step, a plant step in numpy, the next tick -- is examples/track_following.py.

    python closed_loop_rollout.py [--prepare]
--prepare: set up on the throughput layout (TINYMPC_LAYOUT=D, unless the environment names another) and call prepare(): the tracks then
run on layout D's per-instance trajectory form instead of layout A. The same rollout; the kernel line says which ran."""
import os
import sys

import numpy as np
from _common import TinyMPC, problems

prepare = "--prepare" in sys.argv[1:]
if prepare:
    os.environ.setdefault("TINYMPC_LAYOUT", "D")

prob = problems.quadrotor(20)
batch, ticks = 512, 120
T = ticks + prob.N
nx, nu, N = prob.nx, prob.nu, prob.N
rng = np.random.default_rng(0)

# a figure-eight in x / y at constant height, one phase and size per instance; states 0..2 are the position, 6..8 its velocity
phase, size = rng.uniform(0.0, 2.0 * np.pi, batch), rng.uniform(0.2, 0.5, batch)
w = 2.0 * np.pi / 150.0  # one lap in 150 knots
t = w * np.arange(T)[:, None] + phase[None, :]
dt = prob.A[0, 6]  # (the model's time step: position += dt * velocity)
tracks = np.zeros((nx, T, batch), order="F")
tracks[0] = size * np.sin(t)
tracks[1] = size * np.sin(t) * np.cos(t)
tracks[6] = size * np.cos(t) * w / dt
tracks[7] = size * np.cos(2.0 * t) * w / dt

solver = TinyMPC()
solver.setup(prob.A, prob.B, prob.Q, prob.R, N, batch=batch, rho=prob.rho, max_iter=30)
solver.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
solver.set_x_ref_track_batch(tracks)  # the one upload: nx x T x batch
solver.set_ref_auto_advance(1)        # every tick moves every instance one knot on, after its solve
if prepare:
    solver.prepare()
print("kernel:", solver.launch_info()["layout"], "|", solver.jit_info())

solver.set_x0_batch(np.asfortranarray(tracks[:, 0, :]))  # every quadrotor starts on its curve
noise = np.asfortranarray(rng.standard_normal((nx, ticks, batch)) * np.where(np.arange(nx) < 3, 2e-3, 1e-2)[:, None, None])
log = solver.rollout(ticks, disturbance=noise)  # x (nx, ticks+1, batch), u (nu, ticks, batch), iter / status (ticks, batch)

err = np.linalg.norm(log["x"][:2, 1:, :] - tracks[:2, 1:ticks + 1, :], axis=0)  # ticks x batch: the state after tick k belongs to knot k+1
for k in (0, 9, 29, 59, ticks - 1):
    print(f"tick {k:3d}: tracking error {err[k].mean():.4f} m, {log['iter'][k].mean():.1f} iterations on average")
print(f"{ticks} ticks of {batch} instances: {log['gpu_ms']:.2f} ms on the device, {1e3 * log['gpu_ms'] / ticks:.1f} us per tick; "
      f"tracking error over the last 30 ticks {err[-30:].mean():.4f} m (curve size {size.mean():.2f} m on average)")
assert np.array_equal(solver.get_ref_step_batch(), np.full(batch, ticks))
assert np.isfinite(log["x"]).all() and err[-30:].mean() < 0.1
solver.reset()
