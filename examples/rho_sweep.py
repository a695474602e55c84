"""A rho sweep in one launch: ONE quadrotor problem and ONE initial state under a batch of ADMM penalties on a log grid
(set_rho_batch: every instance of the batch gets its own rho, and with it its own LQR cache). Prints the iterations each rho needs to
reach the tolerances and the rho that needs the fewest -- what used to take one handle and one launch per candidate."""
import argparse

import numpy as np
from _common import TinyMPC, problems

ap = argparse.ArgumentParser()
ap.add_argument("--count", type=int, default=64, help="number of rho values on the grid")
ap.add_argument("--lo", type=float, default=0.1, help="smallest rho, as a multiple of the problem's own")
ap.add_argument("--hi", type=float, default=10.0, help="largest rho, as a multiple of the problem's own")
a = ap.parse_args()

quad = problems.quadrotor(50)
rhos = quad.rho * np.geomspace(a.lo, a.hi, a.count)
solver = TinyMPC()
solver.setup(quad.A, quad.B, quad.Q, quad.R, quad.N, batch=a.count, rho=quad.rho, max_iter=500, abs_pri_tol=1e-3, abs_dua_tol=1e-3)
solver.set_bound_constraints(quad.x_min, quad.x_max, quad.u_min, quad.u_max)
solver.set_rho_batch(rhos)                                   # instance b solves the problem with rho = rhos[b]
solver.set_x0_batch(np.tile(quad.x0[:, None], (1, a.count)))  # the same initial state for every instance
ms = solver.solve_timed()
stats = solver.get_stats_batch()
iters, solved = stats["iter"], stats["status"] == 1
for rho, it, ok in zip(solver.get_rho_batch(), iters, solved):
    print(f"rho {rho:9.4f}: {it:4d} iterations{'' if ok else '  (not converged)'}")
if solved.any():
    best = int(np.argmin(np.where(solved, iters, np.iinfo(np.int32).max)))
    print(f"best rho {rhos[best]:.4f} ({iters[best]} iterations; the problem's own rho {quad.rho:g}); {a.count} candidates in {ms:.2f} ms, one launch")
else:
    print(f"best rho: none of the {a.count} candidates converged within {solver.settings['max_iter']} iterations")
solver.reset()
