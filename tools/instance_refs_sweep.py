"""Per-instance references at bench size: kernel milliseconds (HIP events, tinympc_solve_timed) of the same forced-iteration solve with
  shared      one constant reference for every instance (what bench.py times: layout D where the shape is compiled in)
  shared-A    the same on layout A (TINYMPC_LAYOUT=A; the per-instance kernels' own layout)
  shared-A-knot  a shared per-knot reference on layout A (TINYMPC_LAYOUT=A)
  goal        one goal per instance (set_x_ref_batch, (nx, count)): layout D's goal form (k_admm_solve_d_gbnd where the shape is compiled in)
  trajectory  a trajectory per instance (set_x_ref_batch, (nx, N, count)): layout A's k_admm_solve_iref
The variants run interleaved, `--rounds` times; the median of `--reps` launches per round is reported, one JSON line per variant.
    python tools/instance_refs_sweep.py [--batch 8192] [--N 50] [--iters 200] [--rounds 2] [--reps 5] [--only goal]
Counters: run one variant under  rocprofv3 --pmc FETCH_SIZE -- python tools/instance_refs_sweep.py --only trajectory --rounds 1
(a counter run of its own; no tracing in the same run).

Layout D (--d --parent-lib PATH): 8,192 quadrotors x 200 forced iterations with a trajectory per instance on a handle that called
prepare(), at N=50 (the compiled-in trajectory kernel, one wavefront per SIMD) and at N=20 (run-time specialised, two per SIMD; the
handle set up under TINYMPC_LAYOUT=D), with
  parent-A-<N>  the handle on the library of the parent commit at PATH (built from a checkout of the parent): layout A's
                k_admm_solve_iref, where trajectories ran before layout D had a form for them -- the yardstick
  traj-D-<N>    the same handle on this tree's library: layout D's per-instance trajectory form
  goal-D-<N>    one goal per instance on layout D's goal form -- the floor; context, not a condition
Every measurement is a fresh process; the legs alternate, `--rounds` times each (default 4 with --d). The bar: traj-D lies below
parent-A in EVERY round, for each horizon on its own (a plan class that does not stays on layout A).
    python tools/instance_refs_sweep.py --d --parent-lib /path/to/parent/libtinympc_hip.so"""
import argparse
import json
import os
import subprocess
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


D_HORIZONS = (50, 20)
D_LEGS = ["%s-%d" % (k, n) for n in D_HORIZONS for k in ("parent-A", "traj-D", "goal-D")]


def child_d(pkg, a):
    """One process of the --d sweep: one leg's kernel time on whatever library this process loaded. One line."""
    kind, N = a.child.rsplit("-", 1)
    N = int(N)
    P = pkg.problems
    prob = P.quadrotor(N)
    rng = np.random.default_rng(0)
    if N != 50:  # (N=50 x 8,192 is layout D's without a switch: the compiled-in shape)
        os.environ["TINYMPC_LAYOUT"] = "D"
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, N, batch=a.batch, rho=prob.rho, abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=a.iters)
    os.environ.pop("TINYMPC_LAYOUT", None)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    s.prepare()
    if kind == "goal-D":
        s.set_x_ref_batch(0.3 * rng.standard_normal((prob.nx, a.batch)))
    else:
        s.set_x_ref_batch(0.3 * rng.standard_normal((prob.nx, N, a.batch)))
    s.set_x0_batch(P.quadrotor_batch_x0(a.batch))
    s.solve_timed()  # warm-up: first launch, table builds, the specialisation
    out = dict(leg=a.child, kernel_ms=float(np.median([s.solve_timed() for _ in range(a.reps)])),
               kernel="%s %s" % (s.launch_info()["layout"], s.jit_info()), lds_bytes=s.launch_info()["lds_bytes"],
               workgroups=s.launch_info()["workgroups"])
    s.reset()
    print("REFS-CHILD " + json.dumps(out), flush=True)


def sweep_d(a):
    """Starts the children of the --d sweep (it never opens the GPU itself) and prints the table."""
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--d needs --parent-lib: libtinympc_hip.so built from the parent commit")
    recs = {leg: [] for leg in D_LEGS}
    for rnd in range(a.rounds):
        for leg in D_LEGS if rnd % 2 == 0 else D_LEGS[::-1]:
            env = dict(os.environ)
            env.pop("TINYMPC_LAYOUT", None)
            env.pop("TINYMPC_HIP_LIBRARY", None)
            if leg.startswith("parent"):
                env["TINYMPC_HIP_LIBRARY"] = os.path.abspath(a.parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--d", "--child", leg, "--batch", str(a.batch), "--iters", str(a.iters),
                                "--reps", str(a.reps)], env=env, capture_output=True, text=True, timeout=300)
            line = [l for l in r.stdout.splitlines() if l.startswith("REFS-CHILD ")]
            if r.returncode != 0 or not line:
                raise SystemExit("round %d (%s) failed with %d:\n%s\n%s" % (rnd, leg, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            recs[leg].append(json.loads(line[0][len("REFS-CHILD "):]))
            print("# round %d %-12s %.4f ms" % (rnd, leg, recs[leg][-1]["kernel_ms"]), flush=True)
    print("per-instance trajectories on layout D: %d quadrotors x %d forced iterations, a state trajectory per instance (goal-D: a goal per "
          "instance), every handle after prepare(); kernel ms (median of %d launches per round, %d rounds, a fresh process each, legs alternating)"
          % (a.batch, a.iters, a.reps, a.rounds))
    ms = {leg: [r["kernel_ms"] for r in recs[leg]] for leg in D_LEGS}
    for leg in D_LEGS:
        print("%-12s | %s | median %.4f | spread %.4f - %.4f | %d workgroups, %d bytes of LDS each | %s"
              % (leg, " ".join("%.4f" % v for v in ms[leg]), float(np.median(ms[leg])), min(ms[leg]), max(ms[leg]), recs[leg][0]["workgroups"],
                 recs[leg][0]["lds_bytes"], recs[leg][0]["kernel"]))
    for n in D_HORIZONS:
        new, old, floor = "traj-D-%d" % n, "parent-A-%d" % n, "goal-D-%d" % n
        on_d = recs[new][0]["kernel"].startswith("D ")
        below = all(x < o for x, o in zip(ms[new], ms[old]))
        print("N=%d: %s on layout D: %s; below %s in every round: %s (largest %.4f against smallest %.4f, %s's spread %.4f; ratio of medians %.3f); "
              "distance to the floor: %.4f against %s %.4f (ratio %.3f)"
              % (n, new, "yes" if on_d else "NO", old, "yes" if below else "NO", max(ms[new]), min(ms[old]), old, max(ms[old]) - min(ms[old]),
                 float(np.median(ms[new])) / float(np.median(ms[old])), float(np.median(ms[new])), floor, float(np.median(ms[floor])),
                 float(np.median(ms[new])) / float(np.median(ms[floor]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=0, help="default 2; 4 with --d")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--d", action="store_true")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    a.rounds = a.rounds or (4 if a.d else 2)
    if a.d and not a.child:
        return sweep_d(a)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if a.d:
        return child_d(pkg, a)
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
