"""A cone sweep in one launch: ONE rocket landing (N = 10) and ONE initial state under a batch of glide-slope and thrust-cone slopes
(set_cone_slopes_batch: the cone structure belongs to the batch, every instance gets its own slope values). Prints the iterations each
pair of slopes needs and how far the predicted trajectory ends from the pad -- what used to take one handle and one launch per pair."""
import argparse

import numpy as np
from _common import TinyMPC, problems

ap = argparse.ArgumentParser()
ap.add_argument("--count", type=int, default=32, help="number of slope pairs on the grid")
ap.add_argument("--lo", type=float, default=0.4, help="smallest slope, as a multiple of the problem's own")
ap.add_argument("--hi", type=float, default=2.5, help="largest slope, as a multiple of the problem's own")
a = ap.parse_args()

rocket = problems.rocket(10)
scale = np.geomspace(a.lo, a.hi, a.count)
glide = np.asarray(rocket.cones["cx"])[:, None] * scale[None, :]         # (1, count): the state cone, steeper to the right
thrust = np.asarray(rocket.cones["cu"])[:, None] * scale[None, ::-1]     # (1, count): the input cone, wider to the left
solver = TinyMPC()
solver.setup(rocket.A, rocket.B, rocket.Q, rocket.R, rocket.N, batch=a.count, rho=rocket.rho, fdyn=rocket.fdyn, max_iter=500,
             abs_pri_tol=1e-3, abs_dua_tol=1e-3)
solver.set_bound_constraints(rocket.x_min, rocket.x_max, rocket.u_min, rocket.u_max)
solver.set_x_ref(rocket.x_ref)
solver.set_u_ref(rocket.u_ref)
solver.set_cone_constraints(**rocket.cones)                 # the structure, and the slopes of whoever is not named below
solver.set_linear_constraints(**rocket.linear)
solver.set_cone_slopes_batch(glide, thrust)                 # instance b solves the landing under glide[:, b] and thrust[:, b]
solver.set_x0_batch(np.tile(rocket.x0[:, None], (1, a.count)))  # the same initial state for every instance
ms = solver.solve_timed()
stats, sol = solver.get_stats_batch(), solver.get_solution_batch()
miss = np.linalg.norm(sol["states"][:3, -1, :] - rocket.x_ref[:3, -1, None], axis=0)  # end of the horizon against the reference there
for b in range(a.count):
    ok = stats["status"][b] == 1
    print(f"glide slope {glide[0, b]:6.3f} thrust slope {thrust[0, b]:6.3f}: {stats['iter'][b]:4d} iterations, touchdown error {miss[b]:7.4f} m"
          f"{'' if ok else '  (not converged)'}")
print(f"{a.count} slope pairs in {ms:.2f} ms, one launch ({solver.jit_info().strip()})")
solver.reset()
