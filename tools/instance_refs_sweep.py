"""Per-instance references at bench size: kernel milliseconds (HIP events, tinympc_solve_timed) of the same forced-iteration solve with
  shared      one constant reference for every instance (what bench.py times: layout D where the shape is compiled in)
  shared-A    the same on layout A (TINYMPC_LAYOUT=A; the per-instance kernels' own layout)
  shared-A-knot  a shared per-knot reference on layout A (TINYMPC_LAYOUT=A)
  goal        one goal per instance (set_x_ref_batch, (nx, count)): layout D's goal form (k_admm_solve_d_gbnd where the shape is compiled in)
  trajectory  a trajectory per instance (set_x_ref_batch, (nx, N, count)): layout A's k_admm_solve_iref
The variants run interleaved, `--rounds` times; the median of `--reps` launches per round is reported, one JSON line per variant.
    python tools/instance_refs_sweep.py [--batch 8192] [--N 50] [--iters 200] [--rounds 2] [--reps 5] [--only goal]
Counters: run one variant under  rocprofv3 --pmc FETCH_SIZE -- python tools/instance_refs_sweep.py --only trajectory --rounds 1
(a counter run of its own; no tracing in the same run)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ["shared", "shared-A", "shared-A-knot", "goal", "trajectory"]


def make(pkg, variant, batch, N, iters):
    P = pkg.problems
    prob = P.quadrotor(N)
    rng = np.random.default_rng(0)
    layout_a = variant.startswith("shared-A")
    if layout_a:
        os.environ["TINYMPC_LAYOUT"] = "A"
    try:
        s = pkg.TinyMPC()
        s.setup(prob.A, prob.B, prob.Q, prob.R, N, batch=batch, rho=prob.rho, abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=iters)
    finally:
        if layout_a:
            del os.environ["TINYMPC_LAYOUT"]
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if variant == "shared":
        s.set_x_ref(np.tile(0.3 * rng.standard_normal((prob.nx, 1)), (1, N)))
    elif variant == "shared-A-knot":
        s.set_x_ref(0.3 * rng.standard_normal((prob.nx, N)))
    elif variant == "goal":
        s.set_x_ref_batch(0.3 * rng.standard_normal((prob.nx, batch)))
    elif variant == "trajectory":
        s.set_x_ref_batch(0.3 * rng.standard_normal((prob.nx, N, batch)))
    s.set_x0_batch(P.quadrotor_batch_x0(batch))
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=2)
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
