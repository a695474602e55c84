"""Reference tracks: 512 quadrotors, each following its own figure-eight with its own phase. Every instance's whole trajectory (T = 300
knots) is uploaded ONCE and kept on the device; a control tick is one mpc_step -- x0 up, first controls down -- and the library moves
every instance one knot along its track after the tick's solve (set_ref_auto_advance). Some instances are sent back to the start of
their track mid-run (set_ref_step_batch on a sub-range: an RL environment that resets), the others carry on.

    python track_following.py [--prepare]
--prepare: the handle is set up on the throughput layout (TINYMPC_LAYOUT=D, unless the environment names another) and calls
prepare(), which welcomes run-time specialised kernels: the tracks then run on layout D's per-instance trajectory form (the wavefront's
own reference rows in its LDS region) instead of layout A. The same loop, the same results to rounding; the kernel line says which ran."""
import os
import sys

import numpy as np
from _common import TinyMPC, problems

prepare = "--prepare" in sys.argv[1:]
if prepare:
    os.environ.setdefault("TINYMPC_LAYOUT", "D")

prob = problems.quadrotor(20)
batch, T, ticks = 512, 300, 120
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
solver.set_ref_auto_advance(1)        # every mpc_step moves every instance one knot on, after its solve
if prepare:
    solver.prepare()  # (behind the track verbs: the kernel for tracks is decided, and specialised, here and not in the first tick)
print("kernel:", solver.launch_info()["layout"], "|", solver.jit_info())

x = np.asfortranarray(tracks[:, 0, :])  # every quadrotor starts on its curve
reset_at, reset = 60, slice(100, 164)
err = []
for k in range(ticks):
    if k == reset_at:  # 64 instances start their lap again from where they are
        solver.set_ref_step_batch(np.zeros(reset.stop - reset.start, dtype=np.int32), first=reset.start)
    steps = solver.get_ref_step_batch() if k in (0, reset_at, ticks - 1) else None
    u = solver.mpc_step(x)
    if steps is not None:
        print(f"tick {k:3d}: steps {steps[0]} (instance 0) / {steps[reset.start]} (instance {reset.start}); "
              f"iterations {solver.get_stats_batch()['iter'].mean():.1f} on average")
    x = np.asfortranarray(prob.A @ x + prob.B @ u)
    now = np.full(batch, k + 1)  # the knot the new state belongs to, kept on the host: the loop reads nothing back but the controls
    if k >= reset_at:
        now[reset] = k + 1 - reset_at
    now = np.minimum(now, T - 1)
    err.append(np.linalg.norm(x[:2, :] - tracks[:2, now, np.arange(batch)], axis=0))
err = np.array(err)
others = np.ones(batch, dtype=bool)
others[reset] = False
print(f"position error over the last 30 ticks: {err[-30:, others].mean():.4f} m (instances that never reset), "
      f"{err[-30:, reset].mean():.4f} m (the {reset.stop - reset.start} that did); curve size {size.mean():.2f} m on average")
assert np.array_equal(solver.get_ref_step_batch()[others], np.full(others.sum(), ticks))
assert np.array_equal(solver.get_ref_step_batch()[reset], np.full(reset.stop - reset.start, ticks - reset_at))
solver.reset()
