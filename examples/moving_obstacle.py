"""A MOVING obstacle for every vehicle of a small fleet: the 64 quadrotors of obstacle_avoidance.py, each flying to its own goal, but
each cylinder now drifts across its vehicle's path at a known constant velocity. One plane held over the horizon cannot state that:
the cylinder is somewhere else at every knot. With rows per knot (set_linear_constraints_knots_batch) knot i of the horizon gets the
half-space that touches the cylinder WHERE IT WILL BE at knot i, linearised about the previous prediction of that moment (the previous
solution shifted by one tick). One call sends the fleet's N rows per vehicle, one mpc_step solves the tick; the ADMM state, the rows'
duals included, stays warm. Beside the result the script prints what one plane per horizon (set_linear_constraints_batch, the cylinder
where it is NOW, touched at the knot of closest approach) gives on the same scene -- without asserting anything about it."""
import numpy as np
from _common import TinyMPC, problems

prob = problems.quadrotor(20)
batch, ticks, radius = 64, 200, 0.35
vmax, meet = 0.6, (35, 50)              # the fleet cruises at 0.6 m/s (0.03 m per tick): every vehicle passes the middle of the scene in these ticks
margin, speed, iters = 0.25, 0.025, 40  # (m; the cylinder's m per tick: up to 0.5 m, more than its radius, within one 20-knot horizon; ADMM iterations per tick)
# (chosen on the GPU: with these the rows per knot keep every vehicle 0.38 m or more from its axis, while one plane per horizon lets 6 of
# the 64 into their cylinder; at margin 0.15 both let vehicles in, 31 and 28 -- 40 ADMM iterations meet a state row on the slack copy, the
# rollout only nearly; at 0.015 m per tick and margin 0.15 the rows per knot hold, 0.359 m, and one plane lets 3 in)
nx, nu, N = prob.nx, prob.nu, prob.N


def scene():
    """Starts, goals, and every cylinder's axis at tick 0 with its velocity per tick: it starts beside the path and crosses it."""
    rng = np.random.default_rng(0)
    start = np.zeros((nx, batch), order="F")
    start[0], start[1], start[2] = -1.2, rng.uniform(-0.8, 0.8, batch), rng.uniform(-0.2, 0.2, batch)
    goal = start.copy()
    goal[0] = 1.2
    side = np.where(np.arange(batch) % 2 == 0, 1.0, -1.0)  # from the left or from the right of the path
    vel = np.stack([np.zeros(batch), -side * speed * rng.uniform(0.7, 1.0, batch)])
    when = rng.uniform(*meet, batch)                       # the tick at which the axis lies on the vehicle's straight path: as it flies past
    centre0 = np.stack([rng.uniform(-0.2, 0.2, batch), start[1] + rng.uniform(-0.1, 0.1, batch)]) - vel * when
    return start, goal, centre0, vel


def planes(path, centres):
    """path (2, K, batch): predicted x / y positions; centres (2, K, batch): the axis at the same moments. -> A (1, nx, K, batch),
    b (1, K, batch): the half-space -n'p <= -(r + margin + n'c) per knot and vehicle, n pointing from the axis to the prediction."""
    d = path - centres
    n = d / np.maximum(np.linalg.norm(d, axis=0, keepdims=True), 1e-9)
    A = np.zeros((1, nx) + path.shape[1:], order="F")
    A[0, 0], A[0, 1] = -n[0], -n[1]
    return A, -(radius + margin + np.sum(n * centres, axis=0))[None]


def fly(per_knot, report=False):
    """The closed loop with rows per knot, or with one plane per vehicle held over the horizon. -> (closest approach to the moving axis
    per vehicle, final distance to the goal per vehicle)."""
    start, goal, centre0, vel = scene()
    solver = TinyMPC()
    solver.setup(prob.A, prob.B, prob.Q, prob.R, N, batch=batch, rho=prob.rho, max_iter=iters)
    x_min, x_max = prob.x_min.copy(), prob.x_max.copy()
    x_min[6:9], x_max[6:9] = -vmax, vmax                                  # a speed limit on every axis
    solver.set_bound_constraints(x_min, x_max, prob.u_min, prob.u_max)
    solver.set_x_ref_batch(goal)
    x = start.copy()
    path = np.repeat(x[:2, None, :], N, axis=1)  # no prediction yet: the vehicle's own position
    closest = np.full(batch, np.inf)
    for k in range(ticks):
        when = k + np.arange(N)                                           # the moment of every knot of this tick's horizon
        centres = centre0[:, None, :] + vel[:, None, :] * when[None, :, None]
        if per_knot:
            A, b = planes(path, centres)                                  # knot i: the cylinder where it will be at knot i
            solver.set_linear_constraints_knots_batch(A, b, None, None)   # N rows per vehicle, one call
        else:
            i = np.argmin(np.linalg.norm(path - centres[:, :1], axis=0), axis=0)  # the cylinder where it is now, one plane
            A, b = planes(path[:, i, np.arange(batch)][:, None, :], centres[:, :1])
            solver.set_linear_constraints_batch(A[:, :, 0], b[:, 0], None, None)
        u = solver.mpc_step(x)
        if report and k == 0:
            print("kernel:", solver.launch_info()["layout"], "|", solver.jit_info())
        pred = solver.get_solution_batch()["states"][:2]
        path = np.concatenate([pred[:, 1:], pred[:, -1:]], axis=1)        # the same moments seen from the next tick
        x = np.asfortranarray(prob.A @ x + prob.B @ u)
        closest = np.minimum(closest, np.linalg.norm(x[:2] - (centre0 + vel * (k + 1)), axis=0))
        if report and (k % 50 == 0 or k == ticks - 1):
            print(f"tick {k:3d}: distance to goal {np.linalg.norm(x[:3] - goal[:3], axis=0).mean():.3f} m on average, "
                  f"iterations {solver.get_stats_batch()['iter'].mean():.1f}")
    solver.reset()
    return closest, np.linalg.norm(x[:3] - goal[:3], axis=0)


if __name__ == "__main__":
    closest, miss = fly(per_knot=True, report=True)
    print(f"rows per knot: closest approach to the moving axis {closest.min():.3f} m at worst, {closest.mean():.3f} m on average "
          f"(radius {radius} m); final distance to goal {miss.max():.3f} m at worst")
    one_c, one_m = fly(per_knot=False)
    print(f"one plane per horizon, same scene: closest approach {one_c.min():.3f} m at worst, {int((one_c <= radius).sum())} of {batch} "
          f"vehicles inside their cylinder at some tick; final distance to goal {one_m.max():.3f} m at worst")
    assert closest.min() > radius, "a vehicle entered its cylinder"
    assert miss.max() < 0.1, "a vehicle did not reach its goal"
