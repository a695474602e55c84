"""converging_goals.py for a fleet on tracks: 20,000 quadrotors, each following its OWN reference track (set_x_ref_track_batch /
set_u_ref_track_batch after prepare(): a window of N knots per instance, kept on the device), solved to a tolerance. Such a handle
runs layout D's per-instance trajectory form; with a batch larger than the GPU holds at once, the library can run it as ONE resident
set of wavefronts and hand a 16-lane row the next instance -- and that instance's reference rows -- as soon as its own has converged
("slot refill", reported by jit_info()). The example runs the same tick with TINYMPC_REFILL=0 and =1; the results are bit-identical."""
import os

import numpy as np
from _common import TinyMPC, problems

prob = problems.quadrotor(50)
batch, T = 20000, 60
rng = np.random.default_rng(0)
x0s = np.asfortranarray(problems.quadrotor_batch_x0(batch) * rng.uniform(0.02, 1.0, batch)[None, :])
t = np.arange(T)
x_track = np.asfortranarray(0.03 * np.sin(0.1 * t[None, :, None] + rng.uniform(0, 6, (12, 1, batch))))   # a track per instance
u_track = np.asfortranarray(0.003 * np.cos(0.2 * t[None, :, None] + rng.uniform(0, 6, (4, 1, batch))))


def run(refill: bool):
    os.environ["TINYMPC_REFILL"] = "1" if refill else "0"
    solver = TinyMPC()
    solver.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho, abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=200)
    solver.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    solver.prepare()               # per-instance trajectories and tracks run on layout D after prepare()
    solver.set_x_ref_track_batch(x_track)
    solver.set_u_ref_track_batch(u_track)
    solver.set_x0_batch(x0s)
    for _ in range(3):             # three cold solves of the first window, queued back to back
        solver.reset_workspace()
        solver.solve_queued()
    ms = solver.collect_kernel_ms()  # waits once
    kernel = solver.jit_info()     # (the handle settles on the trajectory form at its first solve)
    out = solver.get_first_controls_batch(), solver.get_stats_batch()["iter"]
    solver.reset()
    return kernel, float(np.median(ms)), out


k0, t0, (u_plain, it_plain) = run(False)
k1, t1, (u_refill, it_refill) = run(True)
print(f"{batch} instances, a track each, iterations min/mean/max = {it_plain.min()}/{it_plain.mean():.0f}/{it_plain.max()}")
print(f"plain trajectory form [{k0}]: {t0:.2f} ms per solve of the batch")
print(f"slot refill           [{k1}]: {t1:.2f} ms")
print("identical first controls and iteration counts:", bool(np.array_equal(u_plain, u_refill) and np.array_equal(it_plain, it_refill)))
