"""Per-instance linear rows on per-instance trajectories at bench size: layout D's combined form against layout A and its two floors.

Kernel sweep (default): kernel milliseconds (HIP events, tinympc_solve_timed) of the same forced-iteration solve of `--batch` quadrotors
(N = `--N`, `--iters` iterations) on a handle that called prepare(), with
  parent-A    one state row + one input row per instance AND a trajectory per instance, on the library of the parent commit at
              --parent-lib: layout A's k_admm_solve_ifam, where the combination ran before layout D had a form for it -- the yardstick
  lintraj-D   the same handle on this tree's library: layout D's per-instance families on the wavefront's own linref rows
  lin-D       the rows per instance, the references the shared goal: layout D's ILIN goal form -- a floor; context, not a condition
  traj-D      the trajectories per instance, no rows: layout D's box-path trajectory form -- the other floor
--knots: the rows differ per knot and instance (tinympc_set_linear_constraints_knots_batch; parent-A is then k_admm_solve_ifamk, the
floor lin-D the per-knot variant). The combined per-knot form holds one row per knot up to N=17: run it with --N 16 or so; at N=20 the
leg shows the refusal and layout A.
Every measurement is a fresh process; the legs alternate, `--rounds` times each. The bar: lintraj-D lies below parent-A in EVERY round
(the exit status says it); its distance to the two floors is reported.
    python tools/instance_lin_traj_sweep.py --parent-lib /path/to/parent/libtinympc_hip.so [--knots --N 16]

A tracks tick (--tick): tools/ref_track_sweep.py's closed loop -- every instance on its own track of --T knots, auto-advance 1, --ticks
warm-started mpc_step ticks of --tick-iters iterations, wall time per tick -- with one state row + one input row per instance re-sent in
front of every tick (inside the timed region: the obstacle-relinearisation pattern), after prepare():
  tA  on the library of the parent commit: layout A -- the yardstick          tD  on this tree's library: the combined form
The first controls of every tick of tD must lie within 1e-9 of tA's (asserted); the bar is tD below tA in every round.
    python tools/instance_lin_traj_sweep.py --tick --parent-lib /path/to/parent/libtinympc_hip.so [--N 20] [--T 200]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.instance_lin_sweep import knot_rows, rows  # noqa: E402
from tools.ref_track_sweep import WARMUP, tracks  # noqa: E402

LEGS = ["parent-A", "lintraj-D", "lin-D", "traj-D"]


def trajectories(prob, batch):
    """nx x N x batch and nu x (N-1) x batch: every instance its own window of tools/ref_track_sweep.py's figure-eights."""
    X, U = tracks(prob, batch, prob.N)
    return X, np.asfortranarray(U[:, : prob.N - 1, :])


def per_instance(prob, batch):
    return tuple(np.repeat(m[..., None], batch, axis=-1) for m in rows(prob, batch))


def child(pkg, a):
    """One process of the kernel sweep: one leg's kernel time on whatever library this process loaded. One line."""
    prob = pkg.problems.quadrotor(a.N)
    os.environ.pop("TINYMPC_LAYOUT", None)
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=a.batch, rho=prob.rho, abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=a.iters)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if a.child != "traj-D":
        if a.knots:
            s.set_linear_constraints_knots_batch(*knot_rows(prob, a.batch, True))
        else:
            s.set_linear_constraints_batch(*per_instance(prob, a.batch))
    if a.child != "lin-D":
        X, U = trajectories(prob, a.batch)
        s.set_x_ref_batch(X)
        s.set_u_ref_batch(U)
    s.prepare()
    s.set_x0_batch(pkg.problems.quadrotor_batch_x0(a.batch))
    s.solve_timed()  # warm-up: first launch, table builds
    out = dict(leg=a.child, kernel_ms=float(np.median([s.solve_timed() for _ in range(a.reps)])),
               kernel="%s %s" % (s.launch_info()["layout"], s.jit_info()), lds_bytes=s.launch_info()["lds_bytes"],
               workgroups=s.launch_info()["workgroups"])
    s.reset()
    print("LINTRAJ-CHILD " + json.dumps(out), flush=True)


def start(a, leg, extra, tag):
    env = dict(os.environ)
    env.pop("TINYMPC_LAYOUT", None)
    env.pop("TINYMPC_HIP_LIBRARY", None)
    if leg in ("parent-A", "tA"):
        env["TINYMPC_HIP_LIBRARY"] = os.path.abspath(a.parent_lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--batch", str(a.batch), "--N", str(a.N), "--iters", str(a.iters),
           "--reps", str(a.reps)] + extra
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=500)
    line = [l for l in r.stdout.splitlines() if l.startswith(tag)]
    if r.returncode != 0 or not line:
        raise SystemExit("%s failed with %d:\n%s\n%s" % (leg, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return json.loads(line[0][len(tag):])


def sweep(a):
    """Starts the children of the kernel sweep (it never opens the GPU itself) and prints the table."""
    recs = {leg: [] for leg in LEGS}
    for rnd in range(a.rounds):
        for leg in LEGS if rnd % 2 == 0 else LEGS[::-1]:
            recs[leg].append(start(a, leg, ["--knots"] if a.knots else [], "LINTRAJ-CHILD "))
            print("# round %d %-10s %.4f ms" % (rnd, leg, recs[leg][-1]["kernel_ms"]), flush=True)
    print("per-instance linear rows on per-instance trajectories: %d quadrotors N=%d x %d forced iterations, 1 state row + 1 input row%s, a "
          "trajectory per instance, every handle after prepare(); kernel ms (median of %d launches per round, %d rounds, a fresh process each, "
          "legs alternating)" % (a.batch, a.N, a.iters, " per knot" if a.knots else "", a.reps, a.rounds))
    ms = {leg: [r["kernel_ms"] for r in recs[leg]] for leg in LEGS}
    for leg in LEGS:
        print("%-10s | %s | median %.4f | spread %.4f - %.4f | %d workgroups, %d bytes of LDS each | %s"
              % (leg, " ".join("%.4f" % v for v in ms[leg]), float(np.median(ms[leg])), min(ms[leg]), max(ms[leg]), recs[leg][0]["workgroups"],
                 recs[leg][0]["lds_bytes"], recs[leg][0]["kernel"]))
    on_d = recs["lintraj-D"][0]["kernel"].startswith("D ")
    below = all(n < o for n, o in zip(ms["lintraj-D"], ms["parent-A"]))
    med = {leg: float(np.median(ms[leg])) for leg in LEGS}
    print("lintraj-D on layout D: %s; below parent-A in every round: %s (largest %.4f against smallest %.4f, parent-A's spread %.4f; ratio of "
          "medians %.3f)" % ("yes" if on_d else "NO", "yes" if below else "NO", max(ms["lintraj-D"]), min(ms["parent-A"]),
                             max(ms["parent-A"]) - min(ms["parent-A"]), med["lintraj-D"] / med["parent-A"]))
    print("distance to the floors: lintraj-D median %.4f against lin-D %.4f (ratio %.3f) and traj-D %.4f (ratio %.3f); above both: %s"
          % (med["lintraj-D"], med["lin-D"], med["lintraj-D"] / med["lin-D"], med["traj-D"], med["lintraj-D"] / med["traj-D"],
             "yes" if med["lintraj-D"] > max(med["lin-D"], med["traj-D"]) else "NO"))
    if not below:
        raise SystemExit(1)


def child_tick(pkg, a):
    """One process of the --tick sweep: the closed loop on whatever library it loaded; one JSON line, the first controls in a.dump."""
    P = pkg.problems
    prob = P.quadrotor(a.N)
    N, batch = prob.N, a.batch
    X, U = tracks(prob, batch, a.T)
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, N, batch=batch, rho=prob.rho, max_iter=a.tick_iters, abs_pri_tol=0.0, abs_dua_tol=0.0)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    s.set_x_ref_track_batch(X)
    s.set_u_ref_track_batch(U)
    s.set_ref_auto_advance(1)
    ax, bx, au, bu = per_instance(prob, batch)
    s.set_linear_constraints_batch(ax, bx, au, bu)
    s.prepare()
    x = np.asfortranarray(X[:, 0, :] + 0.05 * P.quadrotor_batch_x0(batch))
    wall, us = [], []
    for k in range(WARMUP + a.ticks):
        bk = bx + 0.01 * k  # (new offsets every tick, formed outside the timed region: only the verb is timed)
        t0 = time.perf_counter()
        s.set_linear_constraints_batch(ax, bk, au, bu)
        u = s.mpc_step(x)
        wall.append(1e6 * (time.perf_counter() - t0))
        us.append(u)
        x = np.asfortranarray(prob.A @ x + prob.B @ u)
    info = "%s %s" % (s.launch_info()["layout"], s.jit_info())
    s.reset()
    np.save(os.path.join(a.dump, "u_%s.npy" % a.child), np.stack(us))
    print("LINTRAJ-TICK " + json.dumps(dict(leg=a.child, tick_us=float(np.median(wall[WARMUP:])), kernel=info)), flush=True)


def sweep_tick(a):
    recs, worst = {"tA": [], "tD": []}, 0.0
    with tempfile.TemporaryDirectory() as tmp:
        for rnd in range(a.rounds):
            for leg in ("tD", "tA") if rnd % 2 == 0 else ("tA", "tD"):
                extra = ["--tick", "--dump", tmp, "--T", str(a.T), "--ticks", str(a.ticks), "--tick-iters", str(a.tick_iters)]
                recs[leg].append(start(a, leg, extra, "LINTRAJ-TICK "))
                print("# round %d %-3s %.1f us" % (rnd, leg, recs[leg][-1]["tick_us"]), flush=True)
            ua, ud = np.load(os.path.join(tmp, "u_tA.npy")), np.load(os.path.join(tmp, "u_tD.npy"))
            worst = max(worst, float(np.max(np.abs(ud - ua)) / np.max(np.abs(ua))))
    print("a tracks tick with rows re-sent: %d quadrotors N=%d, T=%d, 1 state row + 1 input row per instance sent in front of every tick, "
          "auto-advance 1, every handle after prepare(), %d warm-started mpc_step ticks (%d iterations each), wall us per tick (median of the "
          "ticks of a round; %d rounds, a fresh process each, the two libraries alternating)" % (a.batch, a.N, a.T, a.ticks, a.tick_iters, a.rounds))
    for leg, name in (("tA", "tA the parent's library"), ("tD", "tD this tree")):
        v = [r["tick_us"] for r in recs[leg]]
        print("%-24s | %-36s | median %9.1f | spread %8.1f - %8.1f | %s"
              % (name, " ".join("%.1f" % x for x in v), float(np.median(v)), min(v), max(v), recs[leg][0]["kernel"]))
    below = all(d["tick_us"] < p["tick_us"] for d, p in zip(recs["tD"], recs["tA"]))
    print("tD on layout D: %s; first controls within %.1e of tA's (relative to the largest control); tD below tA in every round: %s (ratio of "
          "medians %.3f)" % ("yes" if recs["tD"][0]["kernel"].startswith("D ") else "NO", worst, "yes" if below else "NO",
                             float(np.median([r["tick_us"] for r in recs["tD"]])) / float(np.median([r["tick_us"] for r in recs["tA"]]))))
    assert worst < 1e-9, "the first controls on layout D differ from layout A's"
    if not below:
        raise SystemExit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--knots", action="store_true")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--tick", action="store_true")
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--tick-iters", type=int, default=10)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--dump", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not a.child:
        if not a.parent_lib or not os.path.exists(a.parent_lib):
            raise SystemExit("needs --parent-lib: libtinympc_hip.so built from the parent commit")
        return sweep_tick(a) if a.tick else sweep(a)
    import __graft_entry__ as ge
    (child_tick if a.tick else child)(ge.load_package(), a)


if __name__ == "__main__":
    main()
