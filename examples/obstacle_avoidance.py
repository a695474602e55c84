"""Obstacle avoidance for a small fleet: 64 quadrotors in closed loop, each flying to its OWN goal (set_x_ref_batch) past its OWN
obstacle, a vertical cylinder across its straight path. A cylinder is not convex to stay out of; every tick each vehicle replaces it
by the half-space that touches it at the point nearest to the vehicle's previous prediction -- n'(p - c) >= r, i.e. one row
-n'p <= -(r + n'c) on the position states -- and the fleet's rows go up in one call (set_linear_constraints_batch: the row count belongs
to the batch, the values to the vehicle; the ADMM state, the row's duals included, stays warm). One mpc_step per tick."""
import numpy as np
from _common import TinyMPC, problems

prob = problems.quadrotor(20)
batch, ticks, radius, margin = 64, 160, 0.35, 0.15
nx, nu, N = prob.nx, prob.nu, prob.N  # (margin: 40 ADMM iterations meet a state constraint on the slack copy, the rollout only nearly)
rng = np.random.default_rng(0)

# every vehicle starts at rest left of the origin and flies 2.4 m to the right; its obstacle sits near the middle, a little off its path
start = np.zeros((nx, batch), order="F")
start[0], start[1], start[2] = -1.2, rng.uniform(-0.8, 0.8, batch), rng.uniform(-0.2, 0.2, batch)
goal = start.copy()
goal[0] = 1.2
centre = np.stack([rng.uniform(-0.2, 0.2, batch), start[1] + rng.uniform(-0.12, 0.12, batch)])  # (2, batch): x, y of the cylinder's axis

solver = TinyMPC()
solver.setup(prob.A, prob.B, prob.Q, prob.R, N, batch=batch, rho=prob.rho, max_iter=40)
solver.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
solver.set_x_ref_batch(goal)  # (nx, batch): one goal per vehicle, held over the horizon


def half_spaces(path):
    """path: the predicted x / y positions, (2, N, batch). -> the verb's arrays: Alin_x (1, nx, batch), blin_x (1, batch)."""
    d = path - centre[:, None, :]
    k = np.argmin(np.linalg.norm(d, axis=0), axis=0)  # the knot that comes closest to the axis
    n = d[:, k, np.arange(batch)]
    n = n / np.maximum(np.linalg.norm(n, axis=0), 1e-9)
    A = np.zeros((1, nx, batch), order="F")
    A[0, 0], A[0, 1] = -n[0], -n[1]
    b = -(radius + margin + np.sum(n * centre, axis=0))
    return A, b[None, :]


x = start.copy()
path = np.repeat(x[:2, None, :], N, axis=1)  # no prediction yet: the vehicle's own position
closest = np.full(batch, np.inf)
for k in range(ticks):
    A, b = half_spaces(path)
    solver.set_linear_constraints_batch(A, b, None, None)  # this tick's rows, one per vehicle
    u = solver.mpc_step(x)
    if k == 0:
        print("kernel:", solver.launch_info()["layout"], "|", solver.jit_info())
    path = solver.get_solution_batch()["states"][:2]
    x = np.asfortranarray(prob.A @ x + prob.B @ u)
    closest = np.minimum(closest, np.linalg.norm(x[:2] - centre, axis=0))
    if k % 40 == 0 or k == ticks - 1:
        print(f"tick {k:3d}: distance to goal {np.linalg.norm(x[:3] - goal[:3], axis=0).mean():.3f} m on average, "
              f"iterations {solver.get_stats_batch()['iter'].mean():.1f}")

blocked = np.abs(centre[1] - start[1]) < radius  # the straight line would have passed through the cylinder
print(f"closest approach to the obstacle's axis: {closest.min():.3f} m at worst, {closest.mean():.3f} m on average (radius {radius} m); "
      f"{int(blocked.sum())} of {batch} straight paths were blocked")
print(f"final distance to goal: {np.linalg.norm(x[:3] - goal[:3], axis=0).max():.3f} m at worst")
assert blocked.all() and closest.min() > radius, "a vehicle cut through its obstacle"
assert np.linalg.norm(x[:3] - goal[:3], axis=0).max() < 0.1, "a vehicle did not reach its goal"
solver.reset()
