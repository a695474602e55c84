"""Per-instance bounds at bench size: kernel milliseconds (HIP events, tinympc_solve_timed) of the same forced-iteration solve with
  shared       one constant box for every instance (what bench.py times: layout D where the shape is compiled in)
  box          one box per instance (set_bound_constraints_batch, (nx, count) / (nu, count)): layout D's goal form (k_admm_solve_d_gbnd
               where the shape is compiled in) -- the same kernel body as `shared`, with lr / pNref / lo / hi loaded per lane
  shared-A-knot  shared per-knot bounds on layout A (TINYMPC_LAYOUT=A; the per-knot variant's own layout)
  knot         bounds per knot per instance (set_bound_constraints_batch, (nx, N, count)): layout A's k_admm_solve_ibnd
The variants run interleaved, `--rounds` times; the median of `--reps` launches per round is reported, one JSON line per variant.
    python tools/instance_bounds_sweep.py [--batch 8192] [--N 50] [--iters 200] [--rounds 4] [--reps 5] [--only box,shared]
Counters: run one variant under  rocprofv3 --pmc FETCH_SIZE -- python tools/instance_bounds_sweep.py --only knot --rounds 1
(a counter run of its own; no tracing in the same run)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ["shared", "box", "shared-A-knot", "knot"]


def make(pkg, variant, batch, N, iters):
    P = pkg.problems
    prob = P.quadrotor(N)
    nx, nu = prob.nx, prob.nu
    rng = np.random.default_rng(0)
    layout_a = variant == "shared-A-knot"
    if layout_a:
        os.environ["TINYMPC_LAYOUT"] = "A"
    try:
        s = pkg.TinyMPC()
        s.setup(prob.A, prob.B, prob.Q, prob.R, N, batch=batch, rho=prob.rho, abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=iters)
    finally:
        if layout_a:
            del os.environ["TINYMPC_LAYOUT"]
    wave = 1.0 - 0.3 * np.abs(np.sin(0.3 * np.arange(N)))  # per-knot shrink factor
    if variant == "shared":
        s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    elif variant == "shared-A-knot":
        s.set_bound_constraints(np.outer(prob.x_min, wave), np.outer(prob.x_max, wave), np.outer(prob.u_min, wave[:N - 1]),
                                np.outer(prob.u_max, wave[:N - 1]))
    else:
        fx, fu = rng.uniform(0.5, 1.0, (nx, batch)), rng.uniform(0.3, 1.0, (nu, batch))
        xl, xh, ul, uh = prob.x_min[:, None] * fx, prob.x_max[:, None] * fx, prob.u_min[:, None] * fu, prob.u_max[:, None] * fu
        if variant == "box":
            s.set_bound_constraints_batch(xl, xh, ul, uh)
        else:
            wx, wu = wave[None, :, None], wave[None, :N - 1, None]
            s.set_bound_constraints_batch(xl[:, None, :] * wx, xh[:, None, :] * wx, ul[:, None, :] * wu, uh[:, None, :] * wu)
    s.set_x_ref(np.tile(0.3 * rng.standard_normal((nx, 1)), (1, N)))
    s.set_x0_batch(P.quadrotor_batch_x0(batch))
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    names = [v for v in VARIANTS if not a.only or v in a.only.split(",")]
    solvers = {v: make(pkg, v, a.batch, a.N, a.iters) for v in names}
    for s in solvers.values():  # warm-up: first launch, table builds
        s.solve_timed()
    times = {v: [] for v in names}
    for _ in range(a.rounds):
        for v in names:
            times[v].append(float(np.median([solvers[v].solve_timed() for _ in range(a.reps)])))
    for v in names:
        s = solvers[v]
        print(json.dumps(dict(variant=v, batch=a.batch, N=a.N, iters=a.iters, layout=s.launch_info()["layout"], kernel=s.jit_info(),
                              kernel_ms=times[v], ms_per_iter=min(times[v]) / a.iters)), flush=True)
    for s in solvers.values():
        s.reset()


if __name__ == "__main__":
    main()
