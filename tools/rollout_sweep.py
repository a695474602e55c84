"""Closed-loop rollout at bench size: what a tick costs with the plant on the host and with the plant on the device.

`--batch` quadrotors at N = 50, tolerances 1e-3, max_iter 100, seeded x0 (tools/bench_legs.py's tick workload), a warm-started closed
loop of `--ticks` ticks with the model's own plant. The legs, wall time per tick:
  a   the library of the PARENT commit at --parent-lib: mpc_step per tick (x0 up, first controls down, one synchronisation), the plant
      x <- A x + B u in numpy between ticks -- the host loop a closed-loop study is written as today
  b   this tree's library, the ticks issued one by one with the state staying on the device: solve (launch + synchronisation) and
      plant_step per tick, no copy in either direction
  c   this tree's library, ONE rollout call for all ticks, all four logs requested: the copy-out into pageable host memory at the end
      (220 MB at 8,192 instances and 200 ticks, most of it the states) is inside the measured time; beside it the device time of the
      queue (gpu_ms, one event pair)
  c0  the same call with no logs (log=()): the queue and its one synchronisation alone
Every measurement is a fresh process -- the two libraries alternate, `--rounds` times each -- so the legs share one call's noise. Before
the counted ticks every leg runs WARMUP ticks the same way (first launch, table builds, staging buffers; leg c also one rollout of the
full length, so that its log buffers exist), then starts again from the seeded x0 with a cold ADMM state. The legs' plants differ in
rounding (numpy's dot product against the kernel's chain), so their trajectories agree to rounding, not bit for bit: the mean
iterations per tick are printed beside the times. The bar: leg c below leg a in every round at 4,096 and 8,192 instances (the exit
status says so); at 256, where the zero-copy tick is already lean, the line says which way it went.
    python tools/rollout_sweep.py --parent-lib /path/to/parent/libtinympc_hip.so [--batches 256,4096,8192] [--ticks 200] [--rounds 4]

--metrics: what a SCORED rollout costs (the rollout metrics, tinympc_set_rollout_metrics). The parent is then the commit that has the
rollout but not the metrics; same workload, same protocol. The legs:
  b   the parent's library: solve + plant_step per tick
  c   the parent's library: one rollout call with all four logs, then the eight scores per instance reduced from the logs in numpy (the
      only way to score a rollout there); both parts are timed, the line shows their sum and the numpy part
  c0  the parent's library: one rollout call without logs -- the queue alone, nothing scored
  d   this tree's library: set_rollout_metrics, one rollout call without logs, rollout_metrics() (64 bytes per instance)
The claim: d below c and below b in every round at all three sizes (the exit status says so), and how far d sits above c0.

--noise: what a Monte-Carlo realisation costs (the rollout noise, tinympc_set_rollout_noise). The parent is then the commit that has the
metrics but not the noise; same workload, same protocol, every leg a scored rollout without logs followed by rollout_metrics(). The legs:
  p   the parent's library: the process noise drawn in numpy (standard_normal, nx x ticks x batch, 157 MB at 8,192 x 200) and handed to
      the rollout as its disturbance; both parts are timed, the line shows their sum and the drawing
  c0  the parent's library: no disturbance at all -- the queue alone
  n   this tree's library: process noise drawn on the device
  nm  this tree's library: process and measurement noise drawn on the device
The claim: n below p in every round at 4,096 and 8,192 (the exit status says so); how far n and nm sit above c0, and the 256 row."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP = 3


def run_leg(pkg, leg, batch, ticks):
    """-> (wall us per tick over the counted ticks, mean iterations per tick, kernel line)"""
    P = pkg.problems
    prob = P.quadrotor(50)
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho, max_iter=100, abs_pri_tol=1e-3, abs_dua_tol=1e-3)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    x0 = np.asfortranarray(P.quadrotor_batch_x0(batch))

    def loop(n):
        """n ticks from the state the handle holds (leg a: from x) -> (seconds, iterations per tick)"""
        nonlocal x
        its = []
        t0 = time.perf_counter()
        if leg in ("c", "c0"):
            log = s.rollout(n, log=("x", "u", "iter", "status") if leg == "c" else ())
            gpu_us.append(1e3 * log["gpu_ms"] / n)
            return time.perf_counter() - t0, log["iter"].mean(axis=1) if leg == "c" else []
        for _ in range(n):
            if leg == "a":
                u = s.mpc_step(x)
                x = np.asfortranarray(prob.A @ x + prob.B @ u)
            else:
                s.solve()
                s.plant_step()
        dt = time.perf_counter() - t0
        return dt, its

    def restart():
        nonlocal x
        s.reset_workspace()
        x = x0.copy(order="F")
        s.set_x0_batch(x0)

    x = x0.copy(order="F")
    gpu_us = []
    s.set_x0_batch(x0)
    if leg in ("c", "c0"):
        loop(ticks)
        restart()
    loop(WARMUP)
    restart()
    dt, its = loop(ticks)
    iters = float(np.mean(its)) if len(its) else float("nan")
    info = "%s %s" % (s.launch_info()["layout"], s.jit_info())
    s.reset()
    return 1e6 * dt / ticks, iters, info, (gpu_us[-1] if gpu_us else None)


def numpy_scores(prob, log):
    """The eight scores per instance from a rollout's logs (references zero, the quadrotor's box): vectorised, as a study would write it."""
    qx, ru = np.diag(prob.Q), np.diag(prob.R)
    x, u = log["x"][:, :-1, :], log["u"]
    cost = np.einsum("i,itb->b", qx, x * x) + np.einsum("i,itb->b", ru, u * u)
    xv = np.maximum(0.0, np.maximum(prob.x_min[:, None, None] - x, x - prob.x_max[:, None, None])).max(axis=(0, 1))
    uv = np.maximum(0.0, np.maximum(prob.u_min[:, None, None] - u, u - prob.u_max[:, None, None])).max(axis=(0, 1))
    away = np.abs(x).max(axis=0) > 0.05
    settle = np.where(away.any(axis=0), away.shape[0] - np.argmax(away[::-1], axis=0), 0)
    return dict(cost=cost, x_violation=xv, u_violation=uv, iterations=log["iter"].sum(axis=0), max_iterations=log["iter"].max(axis=0),
                unconverged=(log["status"] != 1).sum(axis=0), settle=settle)


def run_metrics_leg(pkg, leg, batch, ticks):
    """-> (wall us per tick, the numpy part of it (leg c), the mean cost, kernel line)"""
    P = pkg.problems
    prob = P.quadrotor(50)
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho, max_iter=100, abs_pri_tol=1e-3, abs_dua_tol=1e-3)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    x0 = np.asfortranarray(P.quadrotor_batch_x0(batch))
    if leg == "d":
        s.set_rollout_metrics(settle_tol=0.05)

    def loop(n):
        """-> (seconds, seconds of numpy scoring, mean cost or nan)"""
        t0 = time.perf_counter()
        if leg == "b":
            for _ in range(n):
                s.solve()
                s.plant_step()
            return time.perf_counter() - t0, 0.0, float("nan")
        if leg == "c0":
            s.rollout(n, log=())
            return time.perf_counter() - t0, 0.0, float("nan")
        if leg == "c":
            log = s.rollout(n)
            t1 = time.perf_counter()
            m = numpy_scores(prob, log)
            t2 = time.perf_counter()
            return t2 - t0, t2 - t1, float(m["cost"].mean())
        s.rollout(n, log=())
        m = s.rollout_metrics()
        return time.perf_counter() - t0, 0.0, float(m["cost"].mean())

    def restart():
        s.reset_workspace()
        s.set_x0_batch(x0)
        if leg == "d":
            s.reset_rollout_metrics()

    s.set_x0_batch(x0)
    if leg != "b":
        loop(ticks)
        restart()
    loop(WARMUP)
    restart()
    dt, dt_np, cost = loop(ticks)
    info = "%s %s" % (s.launch_info()["layout"], s.jit_info())
    s.reset()
    return 1e6 * dt / ticks, 1e6 * dt_np / ticks, cost, info


def child_metrics(pkg, a):
    has = hasattr(pkg.load_library(), "tinympc_set_rollout_metrics")
    out = dict(library="this" if has else "parent", tick_us={}, numpy_us={}, cost={}, kernel={})
    for leg in (("d",) if has else ("b", "c", "c0")):
        us, us_np, cost, info = run_metrics_leg(pkg, leg, a.batch, a.ticks)
        out["tick_us"][leg], out["numpy_us"][leg], out["cost"][leg], out["kernel"][leg] = us, us_np, cost, info
    print("ROLLOUT-CHILD " + json.dumps(out), flush=True)


def sweep_metrics(a):
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("needs --parent-lib: libtinympc_hip.so built from the parent commit")
    ok = True
    for batch in [int(b) for b in a.batches.split(",")]:
        rows = {"this": [], "parent": []}
        for rnd in range(a.rounds):
            for lib in ("this", "parent") if rnd % 2 == 0 else ("parent", "this"):
                env = dict(os.environ)
                env.pop("TINYMPC_HIP_LIBRARY", None)
                if lib == "parent":
                    env["TINYMPC_HIP_LIBRARY"] = os.path.abspath(a.parent_lib)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--metrics", "--batch", str(batch), "--ticks", str(a.ticks)]
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
                line = [l for l in r.stdout.splitlines() if l.startswith("ROLLOUT-CHILD ")]
                if r.returncode != 0 or not line:
                    raise SystemExit("batch %d round %d (%s) failed with %d:\n%s\n%s" % (batch, rnd, lib, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
                rec = json.loads(line[0][len("ROLLOUT-CHILD "):])
                assert rec["library"] == lib, rec
                rows[lib].append(rec)
                print("# batch %d round %d %-6s %s" % (batch, rnd, lib, json.dumps(rec["tick_us"])), flush=True)
        print("scored closed-loop rollout, %d quadrotors N=50, tolerances 1e-3, max_iter 100, %d warm-started ticks, wall us per tick (%d rounds, a "
              "fresh process each, the two libraries alternating)" % (batch, a.ticks, a.rounds))
        print("%-66s | %-36s | %-9s | %-19s" % ("leg", "rounds", "median", "spread"))
        med = {}
        for leg, lib, name in (("b", "parent", "b  solve + plant_step per tick (parent)"), ("c", "parent", "c  one rollout call, all logs, scores in numpy (parent)"),
                               ("c0", "parent", "c0 one rollout call, no logs, nothing scored (parent)"),
                               ("d", "this", "d  one scored rollout call, no logs, rollout_metrics()")):
            v = [r["tick_us"][leg] for r in rows[lib]]
            med[leg] = float(np.median(v))
            print("%-66s | %-36s | %9.1f | %8.1f - %8.1f" % (name, " ".join("%.1f" % x for x in v), med[leg], min(v), max(v)))
        print("leg c's numpy part per tick (median of the rounds): %.1f us; mean cost c %.9g, d %.9g" %
              (float(np.median([r["numpy_us"]["c"] for r in rows["parent"]])), rows["parent"][0]["cost"]["c"], rows["this"][0]["cost"]["d"]))
        print("kernel: %s" % rows["this"][0]["kernel"]["d"])
        below_c = all(rd["tick_us"]["d"] < rp["tick_us"]["c"] for rd, rp in zip(rows["this"], rows["parent"]))
        below_b = all(rd["tick_us"]["d"] < rp["tick_us"]["b"] for rd, rp in zip(rows["this"], rows["parent"]))
        print("batch %d: d against c %.2fx, d against b %.2fx, d above c0 by %.1f us per tick (%.1f %%); d below c in every round: %s; d below b in every "
              "round: %s\n" % (batch, med["c"] / med["d"], med["b"] / med["d"], med["d"] - med["c0"], 100.0 * (med["d"] / med["c0"] - 1.0),
                                "yes" if below_c else "NO", "yes" if below_b else "NO"))
        ok = ok and below_c and below_b
    if not ok:
        raise SystemExit(1)


def run_noise_leg(pkg, leg, batch, ticks):
    """-> (wall us per tick, the drawing's part of it (leg p), the mean cost, kernel line)"""
    P = pkg.problems
    prob = P.quadrotor(50)
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=batch, rho=prob.rho, max_iter=100, abs_pri_tol=1e-3, abs_dua_tol=1e-3)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    x0 = np.asfortranarray(P.quadrotor_batch_x0(batch))
    s.set_rollout_metrics(settle_tol=0.05)
    sw, sv = np.full(prob.nx, 1e-3), np.full(prob.nx, 1e-2)
    rng = np.random.default_rng(1)

    def loop(n):
        """-> (seconds, seconds of drawing, mean cost)"""
        t0 = t1 = time.perf_counter()
        w = None
        if leg == "p":
            w = rng.standard_normal((batch, n, prob.nx)).T  # (nx, n, batch) in the disturbance's memory order, no copy
            w *= 1e-3
            t1 = time.perf_counter()
        s.rollout(n, disturbance=w, log=())
        m = s.rollout_metrics()
        return time.perf_counter() - t0, t1 - t0, float(m["cost"].mean())

    def restart():
        s.reset_workspace()
        s.set_x0_batch(x0)
        s.reset_rollout_metrics()
        if leg in ("n", "nm"):
            s.set_rollout_noise(process=sw, measurement=sv if leg == "nm" else None, seed=1)  # (the tick starts again at 0)

    restart()
    loop(ticks)
    restart()
    loop(WARMUP)
    restart()
    dt, dt_draw, cost = loop(ticks)
    info = "%s %s" % (s.launch_info()["layout"], s.jit_info())
    s.reset()
    return 1e6 * dt / ticks, 1e6 * dt_draw / ticks, cost, info


def child_noise(pkg, a):
    has = hasattr(pkg.load_library(), "tinympc_set_rollout_noise")
    out = dict(library="this" if has else "parent", tick_us={}, draw_us={}, cost={}, kernel={})
    for leg in (("n", "nm") if has else ("p", "c0")):
        us, us_draw, cost, info = run_noise_leg(pkg, leg, a.batch, a.ticks)
        out["tick_us"][leg], out["draw_us"][leg], out["cost"][leg], out["kernel"][leg] = us, us_draw, cost, info
    print("ROLLOUT-CHILD " + json.dumps(out), flush=True)


def sweep_noise(a):
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("needs --parent-lib: libtinympc_hip.so built from the parent commit")
    ok = True
    for batch in [int(b) for b in a.batches.split(",")]:
        rows = {"this": [], "parent": []}
        for rnd in range(a.rounds):
            for lib in ("this", "parent") if rnd % 2 == 0 else ("parent", "this"):
                env = dict(os.environ)
                env.pop("TINYMPC_HIP_LIBRARY", None)
                if lib == "parent":
                    env["TINYMPC_HIP_LIBRARY"] = os.path.abspath(a.parent_lib)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--noise", "--batch", str(batch), "--ticks", str(a.ticks)]
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
                line = [l for l in r.stdout.splitlines() if l.startswith("ROLLOUT-CHILD ")]
                if r.returncode != 0 or not line:
                    raise SystemExit("batch %d round %d (%s) failed with %d:\n%s\n%s" % (batch, rnd, lib, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
                rec = json.loads(line[0][len("ROLLOUT-CHILD "):])
                assert rec["library"] == lib, rec
                rows[lib].append(rec)
                print("# batch %d round %d %-6s %s" % (batch, rnd, lib, json.dumps(rec["tick_us"])), flush=True)
        print("noisy scored closed-loop rollout, %d quadrotors N=50, tolerances 1e-3, max_iter 100, %d warm-started ticks, no logs, wall us per tick "
              "(%d rounds, a fresh process each, the two libraries alternating)" % (batch, a.ticks, a.rounds))
        print("%-66s | %-36s | %-9s | %-19s" % ("leg", "rounds", "median", "spread"))
        med = {}
        for leg, lib, name in (("p", "parent", "p  disturbance drawn in numpy and uploaded (parent)"), ("c0", "parent", "c0 no disturbance at all (parent)"),
                               ("n", "this", "n  process noise drawn on the device"), ("nm", "this", "nm process and measurement noise drawn on the device")):
            v = [r["tick_us"][leg] for r in rows[lib]]
            med[leg] = float(np.median(v))
            print("%-66s | %-36s | %9.1f | %8.1f - %8.1f" % (name, " ".join("%.1f" % x for x in v), med[leg], min(v), max(v)))
        draw = float(np.median([r["draw_us"]["p"] for r in rows["parent"]]))
        print("leg p's drawing per tick (median of the rounds): %.1f us, p without it %.1f us; mean cost p %.9g, c0 %.9g, n %.9g, nm %.9g" %
              (draw, med["p"] - draw, rows["parent"][0]["cost"]["p"], rows["parent"][0]["cost"]["c0"], rows["this"][0]["cost"]["n"], rows["this"][0]["cost"]["nm"]))
        print("kernel: %s" % rows["this"][0]["kernel"]["n"])
        below = all(rn["tick_us"]["n"] < rp["tick_us"]["p"] for rn, rp in zip(rows["this"], rows["parent"]))
        below_bare = all(rn["tick_us"]["n"] < rp["tick_us"]["p"] - rp["draw_us"]["p"] for rn, rp in zip(rows["this"], rows["parent"]))
        print("batch %d: n against p %.2fx (against p without the drawing %.2fx), n above c0 by %.1f us per tick (%.1f %%), nm above c0 by %.1f us "
              "(%.1f %%); n below p in every round: %s; below p without the drawing in every round: %s\n"
              % (batch, med["p"] / med["n"], (med["p"] - draw) / med["n"], med["n"] - med["c0"], 100.0 * (med["n"] / med["c0"] - 1.0),
                 med["nm"] - med["c0"], 100.0 * (med["nm"] / med["c0"] - 1.0), "yes" if below else "NO", "yes" if below_bare else "NO"))
        if batch >= 4096 and not below:
            ok = False
    if not ok:
        raise SystemExit(1)


def child(pkg, a):
    has = hasattr(pkg.load_library(), "tinympc_rollout_batch")
    out = dict(library="this" if has else "parent", tick_us={}, iters={}, kernel={}, gpu_us={})
    for leg in (("b", "c", "c0") if has else ("a",)):
        us, iters, info, gpu = run_leg(pkg, leg, a.batch, a.ticks)
        out["tick_us"][leg], out["iters"][leg], out["kernel"][leg], out["gpu_us"][leg] = us, iters, info, gpu
    print("ROLLOUT-CHILD " + json.dumps(out), flush=True)


def sweep(a):
    """The parent: starts the children (it never opens the GPU itself) and prints the table."""
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("needs --parent-lib: libtinympc_hip.so built from the parent commit")
    ok = True
    for batch in [int(b) for b in a.batches.split(",")]:
        rows = {"this": [], "parent": []}
        for rnd in range(a.rounds):
            for lib in ("this", "parent") if rnd % 2 == 0 else ("parent", "this"):
                env = dict(os.environ)
                env.pop("TINYMPC_HIP_LIBRARY", None)
                if lib == "parent":
                    env["TINYMPC_HIP_LIBRARY"] = os.path.abspath(a.parent_lib)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--batch", str(batch), "--ticks", str(a.ticks)]
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
                line = [l for l in r.stdout.splitlines() if l.startswith("ROLLOUT-CHILD ")]
                if r.returncode != 0 or not line:
                    raise SystemExit("batch %d round %d (%s) failed with %d:\n%s\n%s" % (batch, rnd, lib, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
                rec = json.loads(line[0][len("ROLLOUT-CHILD "):])
                assert rec["library"] == lib, rec
                rows[lib].append(rec)
                print("# batch %d round %d %-6s %s" % (batch, rnd, lib, json.dumps(rec["tick_us"])), flush=True)
        print("closed-loop rollout, %d quadrotors N=50, tolerances 1e-3, max_iter 100, %d warm-started ticks, wall us per tick (%d rounds, a fresh "
              "process each, the two libraries alternating)" % (batch, a.ticks, a.rounds))
        print("%-58s | %-36s | %-9s | %-19s | %s" % ("leg", "rounds", "median", "spread", "iterations / tick"))
        med = {}
        for leg, lib, name in (("a", "parent", "a  mpc_step + the plant in numpy (parent)"), ("b", "this", "b  solve + plant_step per tick, state on the device"),
                               ("c", "this", "c  one rollout call, all logs copied out"), ("c0", "this", "c0 one rollout call, no logs")):
            v = [r["tick_us"][leg] for r in rows[lib]]
            med[leg] = float(np.median(v))
            it = rows[lib][0]["iters"][leg]
            print("%-58s | %-36s | %9.1f | %8.1f - %8.1f | %s" % (name, " ".join("%.1f" % x for x in v), med[leg], min(v), max(v),
                                                                 "%.2f" % it if it == it else "not read"))
        print("kernel: %s" % rows["this"][0]["kernel"]["c"])
        print("device time of the queue per tick (gpu_ms / ticks, median of the rounds): c %.1f us, c0 %.1f us"
              % (float(np.median([r["gpu_us"]["c"] for r in rows["this"]])), float(np.median([r["gpu_us"]["c0"] for r in rows["this"]]))))
        below = all(rc["tick_us"]["c"] < ra["tick_us"]["a"] for rc, ra in zip(rows["this"], rows["parent"]))
        print("batch %d: c against a %.2fx, c0 against a %.2fx, c0 against b %.2fx; c below a in every round: %s\n"
              % (batch, med["a"] / med["c"], med["a"] / med["c0"], med["b"] / med["c0"], "yes" if below else "NO"))
        if batch >= 4096 and not below:
            ok = False
    if not ok:
        raise SystemExit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,4096,8192")
    ap.add_argument("--batch", type=int, default=8192, help=argparse.SUPPRESS)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--metrics", action="store_true", help="the scored rollout against the parent's legs (see above)")
    ap.add_argument("--noise", action="store_true", help="noise drawn on the device against a disturbance drawn in numpy (see above)")
    a = ap.parse_args()
    if not a.child:
        return sweep_noise(a) if a.noise else sweep_metrics(a) if a.metrics else sweep(a)
    import __graft_entry__ as ge
    (child_noise if a.noise else child_metrics if a.metrics else child)(ge.load_package(), a)


if __name__ == "__main__":
    main()
