"""Per-instance bounds at bench size: kernel milliseconds (HIP events, tinympc_solve_timed) of the same forced-iteration solve with
  shared       one constant box for every instance (what bench.py times: layout D where the shape is compiled in)
  box          one box per instance (set_bound_constraints_batch, (nx, count) / (nu, count)): layout D's goal form (k_admm_solve_d_gbnd
               where the shape is compiled in) -- the same kernel body as `shared`, with lr / pNref / lo / hi loaded per lane
  shared-A-knot  shared per-knot bounds on layout A (TINYMPC_LAYOUT=A; the per-knot variant's own layout)
  knot         bounds per knot per instance (set_bound_constraints_batch, (nx, N, count)): layout A's k_admm_solve_ibnd
The variants run interleaved, `--rounds` times; the median of `--reps` launches per round is reported, one JSON line per variant.
    python tools/instance_bounds_sweep.py [--batch 8192] [--N 50] [--iters 200] [--rounds 4] [--reps 5] [--only box,shared]
Counters: run one variant under  rocprofv3 --pmc FETCH_SIZE -- python tools/instance_bounds_sweep.py --only knot --rounds 1
(a counter run of its own; no tracing in the same run).

Layout D (--d --parent-lib PATH): 8,192 quadrotors x 200 forced iterations with bounds per knot AND per instance on a handle that
called prepare() (set up under TINYMPC_LAYOUT=D), at N=20 (one wavefront per SIMD) and at N=10 (two per SIMD), with
  parent-A-<N>       the handle on the library of the parent commit at PATH (built from a checkout of the parent): layout A's
                     k_admm_solve_ibnd, where such bounds ran before layout D had a form for them -- the yardstick
  knot-D-<N>         the same handle on this tree's library: layout D's per-knot bounds form (IKBND)
  parent-A-traj-<N>  ... with a state trajectory per instance as well, on the parent's library (layout A)
  knot-D-traj-<N>    ... on this tree's library: the form with ITRAJ (N=20: the compiled-in kernel)
  box-D-<N>          one box per instance on layout D's goal form -- a floor; context, not a condition
  traj-D-<N>         a trajectory per instance, bounds constant, on layout D's trajectory form -- the other floor
  parent-A-tick / knot-D-tick   N=20, both halves as tracks of T=200 knots with auto-advance, bounds per knot and instance: wall
                     microseconds of a warm-started mpc_step tick of 10 forced iterations (median of 200 ticks)
Every measurement is a fresh process; the legs alternate, `--rounds` times each (default 4). The bar: each of knot-D-<N>,
knot-D-traj-<N> and knot-D-tick lies below its parent-A leg in EVERY round, each plan class on its own (one that does not stays on
layout A).
    python tools/instance_bounds_sweep.py --d --parent-lib /path/to/parent/libtinympc_hip.so"""
import argparse
import json
import os
import subprocess
import sys
import time

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


D_HORIZONS = (20, 10)
D_KINDS = ("parent-A", "knot-D", "parent-A-traj", "knot-D-traj", "box-D", "traj-D")
D_LEGS = ["%s-%d" % (k, n) for n in D_HORIZONS for k in D_KINDS] + ["parent-A-tick", "knot-D-tick"]
D_PAIRS = [("knot-D-%d" % n, "parent-A-%d" % n) for n in D_HORIZONS] + [("knot-D-traj-%d" % n, "parent-A-traj-%d" % n) for n in D_HORIZONS] + \
          [("knot-D-tick", "parent-A-tick")]


def child_d(pkg, a):
    """One process of the --d sweep: one leg's kernel time (the tick legs: wall time per tick) on whatever library this process loaded."""
    tick = a.child.endswith("-tick")
    kind, N = (a.child[:-5], 20) if tick else (a.child.rsplit("-", 1)[0], int(a.child.rsplit("-", 1)[1]))
    P = pkg.problems
    prob = P.quadrotor(N)
    nx, nu, batch = prob.nx, prob.nu, a.batch
    rng = np.random.default_rng(0)
    os.environ["TINYMPC_LAYOUT"] = "D"
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, N, batch=batch, rho=prob.rho, abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=10 if tick else a.iters)
    os.environ.pop("TINYMPC_LAYOUT", None)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    s.prepare()
    fx, fu = rng.uniform(0.5, 1.0, (nx, batch)), rng.uniform(0.3, 1.0, (nu, batch))
    xl, xh, ul, uh = prob.x_min[:, None] * fx, prob.x_max[:, None] * fx, prob.u_min[:, None] * fu, prob.u_max[:, None] * fu
    wave = 1.0 - 0.3 * np.abs(np.sin(0.3 * np.arange(N)[:, None] + rng.uniform(0, 6, batch)[None, :]))  # per-knot shrink factor, a phase per instance
    wx, wu = wave[None], wave[None, :N - 1]
    if kind == "box-D":
        s.set_bound_constraints_batch(xl, xh, ul, uh)
    elif kind != "traj-D":
        s.set_bound_constraints_batch(xl[:, None, :] * wx, xh[:, None, :] * wx, ul[:, None, :] * wu, uh[:, None, :] * wu)
    if tick:
        T = 200
        tt = np.arange(T)
        s.set_x_ref_track_batch(np.asfortranarray(0.3 * np.sin(0.1 * tt[None, :, None] + rng.uniform(0, 6, (nx, 1, batch)))))
        s.set_u_ref_track_batch(np.asfortranarray(0.03 * np.cos(0.2 * tt[None, :, None] + rng.uniform(0, 6, (nu, 1, batch)))))
        s.set_ref_auto_advance(1)
    elif kind.endswith("traj") or kind == "traj-D":
        s.set_x_ref_batch(0.3 * rng.standard_normal((nx, N, batch)))
    x = P.quadrotor_batch_x0(batch)
    if tick:
        wall = []
        for k in range(a.ticks + 5):  # (five warm-up ticks: first launch, table builds, the specialisation)
            t0 = time.perf_counter()
            u = s.mpc_step(x)
            wall.append(1e6 * (time.perf_counter() - t0))
            x = np.asfortranarray(prob.A @ x + prob.B @ u)
        value = float(np.median(wall[5:]))
    else:
        s.set_x0_batch(x)
        s.solve_timed()  # warm-up: first launch, table builds, the specialisation
        value = float(np.median([s.solve_timed() for _ in range(a.reps)]))
    out = dict(leg=a.child, value=value, kernel="%s %s" % (s.launch_info()["layout"], s.jit_info()), lds_bytes=s.launch_info()["lds_bytes"],
               workgroups=s.launch_info()["workgroups"])
    s.reset()
    print("BOUNDS-CHILD " + json.dumps(out), flush=True)


def sweep_d(a):
    """Starts the children of the --d sweep (it never opens the GPU itself) and prints the table."""
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--d needs --parent-lib: libtinympc_hip.so built from the parent commit")
    legs = [l for l in D_LEGS if not a.only or any(l.startswith(w) or l.endswith(w) for w in a.only.split(","))]
    recs = {leg: [] for leg in legs}
    for rnd in range(a.rounds):
        for leg in legs if rnd % 2 == 0 else legs[::-1]:
            env = dict(os.environ)
            env.pop("TINYMPC_LAYOUT", None)
            env.pop("TINYMPC_HIP_LIBRARY", None)
            if leg.startswith("parent"):
                env["TINYMPC_HIP_LIBRARY"] = os.path.abspath(a.parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--d", "--child", leg, "--batch", str(a.batch), "--iters", str(a.iters),
                                "--reps", str(a.reps), "--ticks", str(a.ticks)], env=env, capture_output=True, text=True, timeout=300)
            line = [l for l in r.stdout.splitlines() if l.startswith("BOUNDS-CHILD ")]
            if r.returncode != 0 or not line:
                raise SystemExit("round %d (%s) failed with %d:\n%s\n%s" % (rnd, leg, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            recs[leg].append(json.loads(line[0][len("BOUNDS-CHILD "):]))
            print("# round %d %-18s %.4f" % (rnd, leg, recs[leg][-1]["value"]), flush=True)
    print("bounds per knot and instance on layout D: %d quadrotors x %d forced iterations, every handle after prepare(); kernel ms (median of %d "
          "launches per round); the tick legs: wall us of an mpc_step tick of 10 iterations, tracks of T=200 with auto-advance (median of %d ticks); "
          "%d rounds, a fresh process each, legs alternating" % (a.batch, a.iters, a.reps, a.ticks, a.rounds))
    v = {leg: [r["value"] for r in recs[leg]] for leg in legs}
    for leg in legs:
        print("%-18s | %s | median %.4f | spread %.4f - %.4f | %d workgroups, %d bytes of LDS each | %s"
              % (leg, " ".join("%.4f" % x for x in v[leg]), float(np.median(v[leg])), min(v[leg]), max(v[leg]), recs[leg][0]["workgroups"],
                 recs[leg][0]["lds_bytes"], recs[leg][0]["kernel"]))
    ok = True
    for new, old in D_PAIRS:
        if new not in recs or old not in recs:
            continue
        on_d = recs[new][0]["kernel"].startswith("D ")
        below = all(x < o for x, o in zip(v[new], v[old]))
        ok = ok and on_d and below
        print("%s on layout D: %s; below %s in every round: %s (largest %.4f against smallest %.4f; ratio of medians %.3f)"
              % (new, "yes" if on_d else "NO", old, "yes" if below else "NO", max(v[new]), min(v[old]), float(np.median(v[new])) / float(np.median(v[old]))))
    if not ok:
        raise SystemExit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--d", action="store_true")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
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
