"""Scoring a rollout on the device: a rho sweep judged by what the controller achieves in closed loop, not by the iterations of one
solve (rho_sweep.py). ONE quadrotor problem and ONE initial state under a batch of ADMM penalties (set_rho_batch); every candidate
drives the same plant for `--ticks` ticks with a cap on the iterations per tick, and the rollout metrics (set_rollout_metrics) keep a
closed-loop cost, the worst bound violation, the iterations and the settle step per instance ON THE DEVICE: the rollout is called with
log=(), and 64 bytes per instance come back instead of every state of every tick. The example prints the table and the best rho, then
repeats the run with logs and checks the best candidate's score against numpy.

    python rollout_scores.py [--count 64] [--ticks 100] [--max-iter 10]"""
import argparse

import numpy as np
from _common import TinyMPC, problems

ap = argparse.ArgumentParser()
ap.add_argument("--count", type=int, default=64, help="number of rho values on the grid")
ap.add_argument("--ticks", type=int, default=100, help="closed-loop ticks per candidate")
ap.add_argument("--max-iter", type=int, default=10, help="ADMM iterations a tick may spend")
ap.add_argument("--lo", type=float, default=0.05, help="smallest rho, as a multiple of the problem's own")
ap.add_argument("--hi", type=float, default=20.0, help="largest rho, as a multiple of the problem's own")
a = ap.parse_args()

quad = problems.quadrotor(20)
rhos = quad.rho * np.geomspace(a.lo, a.hi, a.count)
qx, ru = np.diag(quad.Q).copy(), np.diag(quad.R).copy()
x0 = np.tile((2.0 * quad.x0)[:, None], (1, a.count))  # twice the problem's own offset: the first ticks lean on the input bounds


def candidates():
    s = TinyMPC()
    s.setup(quad.A, quad.B, quad.Q, quad.R, quad.N, batch=a.count, rho=quad.rho, max_iter=a.max_iter, abs_pri_tol=1e-3, abs_dua_tol=1e-3)
    s.set_bound_constraints(quad.x_min, quad.x_max, quad.u_min, quad.u_max)
    s.set_rho_batch(rhos)    # instance b controls with rho = rhos[b]; the plant is the same model for all
    s.set_x0_batch(x0)       # ... from the same initial state
    s.set_rollout_metrics(settle_tol=0.05)  # weights: the diagonals of Q and R
    return s


solver = candidates()
ms = solver.rollout(a.ticks, log=())["gpu_ms"]  # no logs: nothing but the scores leaves the device
m = solver.rollout_metrics()
solver.reset()
for b in range(a.count):
    print(f"rho {rhos[b]:9.4f}: cost {m['cost'][b]:12.4f}  input breach {m['u_violation'][b]:.2e}  {m['iterations'][b]:5d} iterations "
          f"({m['unconverged'][b]:3d} ticks not converged)  settled after tick {m['settle'][b]}")
best = int(np.argmin(m["cost"]))
print(f"best rho {rhos[best]:.4f}: closed-loop cost {m['cost'][best]:.4f} over {a.ticks} ticks (the problem's own rho {quad.rho:g}: "
      f"{m['cost'][int(np.argmin(np.abs(rhos - quad.rho)))]:.4f}); {a.count} candidates, {ms:.2f} ms on the device, {8 * 8 * a.count} bytes read back")

# the same run with logs: the score of the best candidate, recomputed from its states and controls
solver = candidates()
log = solver.rollout(a.ticks)
again = solver.rollout_metrics()
solver.reset()
e, d = log["x"][:, :a.ticks, best], log["u"][:, :, best]  # the references are zero
cost = float((qx[:, None] * e * e).sum() + (ru[:, None] * d * d).sum())
print(f"check: cost of rho {rhos[best]:.4f} from the logs {cost:.10f}, on the device {m['cost'][best]:.10f}")
assert np.array_equal(again["cost"], m["cost"]) and np.array_equal(again["steps"], np.full(a.count, a.ticks))
assert abs(cost - m["cost"][best]) <= 1e-10 * cost, (cost, m["cost"][best])
assert m["iterations"][best] == log["iter"][:, best].sum() and m["unconverged"][best] == (log["status"][:, best] != 1).sum()
print("self-check passed")
