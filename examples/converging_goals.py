"""converging_batch.py for a fleet: 30,000 quadrotors, each with its OWN goal (set_x_ref_batch / set_u_ref_batch, one column per
instance) and its OWN box on the inputs (set_bound_constraints_batch), solved to a tolerance. Such a handle runs layout D's
per-instance goal form; with a batch larger than the GPU holds at once, the library runs it as ONE resident set of wavefronts and
hands a 16-lane row the next instance -- and that instance's goal and box -- as soon as its own has converged ("slot refill",
reported by jit_info()). Results are bit-identical to the plain goal kernel's (TINYMPC_REFILL=0)."""
import os

import numpy as np
from _common import TinyMPC, problems

prob = problems.quadrotor(50)
batch = 30000
rng = np.random.default_rng(0)
x0s = problems.quadrotor_batch_x0(batch) * rng.uniform(0.05, 3.0, batch)[None, :]
goals = np.zeros((12, batch))
goals[:3] = 0.1 * rng.standard_normal((3, batch))        # a position per instance
u_goals = 0.02 * rng.standard_normal((4, batch))
width = rng.uniform(0.6, 1.0, batch)                     # every instance's own input limits
x_lo, x_hi = (np.repeat(v[:, None], batch, axis=1) for v in (prob.x_min, prob.x_max))
u_lo, u_hi = prob.u_min[:, None] * width[None, :], prob.u_max[:, None] * width[None, :]


def run(refill: bool):
    os.environ["TINYMPC_REFILL"] = "1" if refill else "0"
    solver = TinyMPC()
    solver.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho, abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=200)
    solver.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    solver.set_x_ref_batch(goals)
    solver.set_u_ref_batch(u_goals)
    solver.set_bound_constraints_batch(x_lo, x_hi, u_lo, u_hi)
    solver.set_x0_batch(x0s)
    kernel = solver.jit_info()
    for _ in range(3):             # three cold solves, queued back to back
        solver.reset_workspace()
        solver.solve_queued()
    ms = solver.collect_kernel_ms()  # waits once
    out = solver.get_first_controls_batch(), solver.get_stats_batch()["iter"]
    solver.reset()
    return kernel, float(np.median(ms)), out


k0, t0, (u_plain, it_plain) = run(False)
k1, t1, (u_refill, it_refill) = run(True)
print(f"{batch} instances, a goal and a box each, iterations min/mean/max = {it_plain.min()}/{it_plain.mean():.0f}/{it_plain.max()}")
print(f"plain goal kernel  [{k0}]: {t0:.2f} ms per solve of the batch")
print(f"slot refill        [{k1}]: {t1:.2f} ms")
print("identical first controls and iteration counts:", bool(np.array_equal(u_plain, u_refill) and np.array_equal(it_plain, it_refill)))
