"""Obstacles on a track: the 64 quadrotors and drifting cylinders of moving_obstacle.py, but no vehicle flies to a goal any more -- each
follows its OWN time-stamped track (the straight line from its start to its end point at cruise speed, uploaded once and kept on the
device: set_x_ref_track_batch + set_ref_auto_advance) and has to leave it where its cylinder crosses it. Every tick sends the fleet's
half-spaces, one row per knot and vehicle, linearised about the previous prediction (set_linear_constraints_knots_batch), and one
mpc_step solves the tick.

The handle is set up on the throughput layout (TINYMPC_LAYOUT=D, unless the environment names another) and calls prepare(): per-instance
rows AND per-instance tracks then run on layout D together -- the families' kernel with every wavefront's rows per knot and its window
of the track in its own LDS region -- where they fit. Rows per knot beside a track fit up to N=17 for this vehicle, hence the horizon of
16 knots; --one-plane sends one plane per vehicle and tick instead (set_linear_constraints_batch, the cylinder where it is now: a form
that holds horizons up to 22 beside a track), and is told what it gives on the same scene without asserting anything about it.

    python obstacle_on_track.py [--one-plane] [--margin M] [--iters K]"""
import os
import sys

os.environ.setdefault("TINYMPC_LAYOUT", "D")

import numpy as np  # noqa: E402
from _common import TinyMPC, problems  # noqa: E402


def _arg(name, default, kind=float):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv[1:] else default


prob = problems.quadrotor(16)
batch, ticks, radius = 64, 130, 0.35
vmax, meet, lap = 0.6, (35, 50), 80     # the track runs its 2.4 m in 80 ticks (0.03 m per tick); the cylinder crosses it in these ticks
margin, speed, iters = _arg("--margin", 0.25), 0.025, _arg("--iters", 40, int)  # (m; the cylinder's m per tick; ADMM iterations per tick)
# (chosen on the GPU: with these the rows per knot keep every vehicle 0.47 m or more from its axis and every vehicle ends within 0.05 m of
# its track's end, up to 1.13 m off the track on the way round; at margin 0.15 a vehicle enters its cylinder -- 40 ADMM iterations meet a
# state row on the slack copy, the rollout only nearly, as in moving_obstacle.py; --one-plane at margin 0.25 lets 9 of the 64 in)
nx, nu, N = prob.nx, prob.nu, prob.N
T = lap + 1                             # knots of a track: past its end a window holds the last one (the end point, at rest)


def scene():
    """Starts, end points, and every cylinder's axis at tick 0 with its velocity per tick (moving_obstacle.py's scene, draw for draw)."""
    rng = np.random.default_rng(0)
    start = np.zeros((nx, batch), order="F")
    start[0], start[1], start[2] = -1.2, rng.uniform(-0.8, 0.8, batch), rng.uniform(-0.2, 0.2, batch)
    goal = start.copy()
    goal[0] = 1.2
    side = np.where(np.arange(batch) % 2 == 0, 1.0, -1.0)
    vel = np.stack([np.zeros(batch), -side * speed * rng.uniform(0.7, 1.0, batch)])
    when = rng.uniform(*meet, batch)
    centre0 = np.stack([rng.uniform(-0.2, 0.2, batch), start[1] + rng.uniform(-0.1, 0.1, batch)]) - vel * when
    return start, goal, centre0, vel


def tracks_of(start, goal):
    """nx x T x batch: where every vehicle should be at every tick, and how fast (states 0..2 position, 6..8 velocity)."""
    s = (np.arange(T) / lap)[None, :, None]
    tr = np.asfortranarray(start[:, None, :] + (goal - start)[:, None, :] * s)
    dt = prob.A[0, 6]  # (the model's time step: position += dt * velocity)
    tr[6:9, :-1] = ((goal - start)[:3] / lap / dt)[:, None, :]
    tr[6:9, -1] = 0.0
    return tr


def planes(path, centres):
    """path, centres (2, K, batch) -> A (1, nx, K, batch), b (1, K, batch): -n'p <= -(r + margin + n'c), n from the axis to the prediction."""
    d = path - centres
    n = d / np.maximum(np.linalg.norm(d, axis=0, keepdims=True), 1e-9)
    A = np.zeros((1, nx) + path.shape[1:], order="F")
    A[0, 0], A[0, 1] = -n[0], -n[1]
    return A, -(radius + margin + np.sum(n * centres, axis=0))[None]


def fly(per_knot):
    start, goal, centre0, vel = scene()
    tracks = tracks_of(start, goal)
    solver = TinyMPC()
    solver.setup(prob.A, prob.B, prob.Q, prob.R, N, batch=batch, rho=prob.rho, max_iter=iters)
    x_min, x_max = prob.x_min.copy(), prob.x_max.copy()
    x_min[6:9], x_max[6:9] = -vmax, vmax
    solver.set_bound_constraints(x_min, x_max, prob.u_min, prob.u_max)
    solver.set_x_ref_track_batch(tracks)  # the one upload
    solver.set_ref_auto_advance(1)        # every mpc_step moves every vehicle one knot along its track, after its solve
    x = start.copy()
    path = np.repeat(x[:2, None, :], N, axis=1)
    closest, off_track = np.full(batch, np.inf), np.zeros(batch)
    for k in range(ticks):
        centres = centre0[:, None, :] + vel[:, None, :] * (k + np.arange(N))[None, :, None]
        if per_knot:
            A, b = planes(path, centres)
            solver.set_linear_constraints_knots_batch(A, b, None, None)
        else:
            i = np.argmin(np.linalg.norm(path - centres[:, :1], axis=0), axis=0)
            A, b = planes(path[:, i, np.arange(batch)][:, None, :], centres[:, :1])
            solver.set_linear_constraints_batch(A[:, :, 0], b[:, 0], None, None)
        if k == 0:
            solver.prepare()  # (behind the first rows: the kernel for rows on tracks is decided, and specialised, here)
            print("kernel:", solver.launch_info()["layout"], "|", solver.jit_info())
        u = solver.mpc_step(x)
        pred = solver.get_solution_batch()["states"][:2]
        path = np.concatenate([pred[:, 1:], pred[:, -1:]], axis=1)
        x = np.asfortranarray(prob.A @ x + prob.B @ u)
        closest = np.minimum(closest, np.linalg.norm(x[:2] - (centre0 + vel * (k + 1)), axis=0))
        off_track = np.maximum(off_track, np.linalg.norm(x[:3] - tracks[:3, min(k + 1, T - 1)], axis=0))
        if k % 40 == 0 or k == ticks - 1:
            print(f"tick {k:3d}: {np.linalg.norm(x[:3] - tracks[:3, min(k + 1, T - 1)], axis=0).mean():.3f} m from the track on average, "
                  f"iterations {solver.get_stats_batch()['iter'].mean():.1f}")
    assert np.array_equal(solver.get_ref_step_batch(), np.full(batch, ticks))
    solver.reset()
    return closest, off_track, np.linalg.norm(x[:3] - goal[:3], axis=0)


if __name__ == "__main__":
    per_knot = "--one-plane" not in sys.argv[1:]
    closest, off_track, miss = fly(per_knot)
    print(f"{'rows per knot' if per_knot else 'one plane per tick'} on a track: closest approach to the moving axis {closest.min():.3f} m at worst, "
          f"{closest.mean():.3f} m on average (radius {radius} m), {int((closest <= radius).sum())} of {batch} vehicles inside their cylinder at "
          f"some tick; furthest from the track {off_track.max():.3f} m; final distance to the track's end {miss.max():.3f} m at worst")
    if per_knot:
        assert closest.min() > radius, "a vehicle entered its cylinder"
        assert miss.max() < 0.1, "a vehicle did not reach the end of its track"
