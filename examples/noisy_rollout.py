"""A noisy sensor, swept on the device: the reference's closed-loop cartpole example (interactive_cartpole.m hands its solver the state
plus 0.01 randn, "add measurement noise") as a batch -- `--levels` sensor noise levels times `--realisations` seeded realisations each,
ONE handle and ONE scored rollout. set_rollout_noise draws the noise in the plant step itself (one standard deviation per instance and
state row, no nx x ticks x batch array drawn on the host and uploaded); the controller reads the noisy measurement, the plant carries the
true state on, and the rollout metrics (set_rollout_metrics) score the TRUE state. The rollout is called with log=(): 64 bytes per
instance come back. The example prints the mean closed-loop cost and the mean settle step against the level, then regenerates one
instance's measurement noise (rollout_noise) and checks its size.

    python noisy_rollout.py [--levels 6] [--realisations 64] [--ticks 300] [--top 0.08] [--seed 1]"""
import argparse

import numpy as np
from _common import TinyMPC, problems

ap = argparse.ArgumentParser()
ap.add_argument("--levels", type=int, default=6, help="noise levels: 0, then --top halved level by level")
ap.add_argument("--realisations", type=int, default=64, help="instances per level")
ap.add_argument("--ticks", type=int, default=300, help="closed-loop ticks")
ap.add_argument("--top", type=float, default=0.08, help="the largest standard deviation of the sensor noise (the reference's example: 0.01)")
ap.add_argument("--seed", type=int, default=1)
a = ap.parse_args()

cart = problems.cartpole(20, True)
levels = np.concatenate([[0.0], a.top * 0.5 ** np.arange(a.levels - 2, -1, -1)])
batch = a.levels * a.realisations
level_of = np.repeat(levels, a.realisations)                       # instance b measures with level_of[b]
sv = np.tile(level_of[None, :], (cart.nx, 1))                      # ... on every state row
x0 = np.tile(cart.x0[:, None], (1, batch))                         # all from the problem's own offset

solver = TinyMPC()
solver.setup(cart.A, cart.B, cart.Q, cart.R, cart.N, batch=batch, rho=cart.rho, max_iter=100, abs_pri_tol=1e-3, abs_dua_tol=1e-3)
solver.set_bound_constraints(cart.x_min, cart.x_max, cart.u_min, cart.u_max)
solver.set_x0_batch(x0)
solver.set_rollout_metrics(settle_tol=0.05)                        # weights: the diagonals of Q and R
solver.set_rollout_noise(measurement=sv, seed=a.seed)              # the sensor; process= would disturb the plant itself
ms = solver.rollout(a.ticks, log=())["gpu_ms"]
m = solver.rollout_metrics()
truth = solver.plant_state()                                       # the state the plant holds, not the last measurement
v = solver.rollout_noise(0, a.ticks)["v"]                          # what the steps added to the measurements, regenerated
solver.reset()

cost = m["cost"].reshape(a.levels, a.realisations)
settle = m["settle"].reshape(a.levels, a.realisations)
for i, lv in enumerate(levels):
    print(f"level {lv:8.5f}: cost {cost[i].mean():12.4f}  (min {cost[i].min():12.4f}, max {cost[i].max():12.4f})  "
          f"settled after tick {settle[i].mean():7.1f}  |x| at the end {np.abs(truth[:, i * a.realisations:(i + 1) * a.realisations]).max():.4f}")
print(f"{batch} cartpoles x {a.ticks} ticks: {ms:.2f} ms on the device, {8 * 8 * batch} bytes of scores read back, no disturbance uploaded "
      f"(a drawn one would be {8 * cart.nx * a.ticks * batch} bytes)")

# the regenerated noise is the levels': zero where the level is zero, its sample deviation the level elsewhere
assert np.array_equal(m["steps"], np.full(batch, a.ticks))
assert (v[:, :, :a.realisations] == 0.0).all() and np.ptp(cost[0]) == 0.0  # (level 0: every realisation is the noise-free loop)
for i, lv in enumerate(levels[1:], start=1):
    sd = v[:, :, i * a.realisations:(i + 1) * a.realisations].std()
    assert abs(sd / lv - 1.0) < 5.0 / np.sqrt(cart.nx * a.ticks * a.realisations), (lv, sd)
print("self-check passed")
