"""Per-instance cone slopes at bench size.

Kernel milliseconds (HIP events, tinympc_solve_timed) of forced-iteration solves of `--batch` instances, `--iters` iterations. Every
measurement is a fresh process; the legs alternate, `--rounds` times each, so they share the call's noise. Reported: each round's
median of `--reps` launches, the legs' medians and spreads.

(a) nothing existing got slower -- the row mode's own workload (quadrotors N=20, one state row plus one input row per instance,
    tinympc_set_linear_constraints_batch) on this tree's library against the library of the parent commit at --parent-lib:
      parent-A, new-A   layout A (k_admm_solve_ifam)
      parent-D, new-D   layout D after prepare() (the per-instance form)
    The condition: the new medians lie inside the parent's spread of the same session.
(b) the new mode -- rocket landings N=10 (references held constant over the horizon, so that layout D takes them), slopes per instance
    (tinympc_set_cone_slopes_batch):
      cones-A           layout A
      cones-D           layout D after prepare()
      shared            the same handle with shared cones on the kernel it picks by default
    and the wall time of tinympc_set_cone_slopes_batch and of its _device form for the whole batch.
    python tools/instance_cone_sweep.py --parent-lib /path/to/parent/libtinympc_hip.so [--batch 8192] [--iters 100] [--rounds 4] [--reps 5]"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from instance_lin_sweep import device_copy, rows  # noqa: E402

LEGS = ["parent-A", "new-A", "parent-D", "new-D", "cones-A", "cones-D", "shared"]


def slopes(prob, batch, seed=11):
    rng = np.random.default_rng(seed)
    return [np.asfortranarray(np.asarray(prob.cones[k])[:, None] * np.exp(rng.uniform(np.log(0.4), np.log(2.5), (len(prob.cones[k]), batch))))
            for k in ("cx", "cu")]


def make(pkg, leg, a):
    os.environ.pop("TINYMPC_LAYOUT", None)
    P = pkg.problems
    s = pkg.TinyMPC()
    if leg.startswith(("parent", "new")):  # (a): the row mode's workload
        prob = P.quadrotor(20)
        s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=a.batch, rho=prob.rho, abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=a.iters)
        s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
        s.set_linear_constraints_batch(*(np.repeat(m[..., None], a.batch, axis=-1) for m in rows(prob, a.batch)))
        if leg.endswith("-D"):
            s.prepare()
        s.set_x0_batch(P.quadrotor_batch_x0(a.batch))
        return s, prob
    prob = P.rocket(10)
    prob = dataclasses.replace(prob, x_ref=np.repeat(prob.x_ref[:, :1], prob.N, axis=1))
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=a.batch, rho=prob.rho, fdyn=prob.fdyn, abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=a.iters)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    s.set_x_ref(prob.x_ref)
    s.set_u_ref(prob.u_ref)
    s.set_cone_constraints(**prob.cones)
    s.set_linear_constraints(**prob.linear)
    if leg != "shared":
        s.set_cone_slopes_batch(*slopes(prob, a.batch))
    if leg == "cones-D":
        s.prepare()
    rng = np.random.default_rng(11)
    s.set_x0_batch(np.asfortranarray(prob.x0[:, None] * (1.0 + 0.1 * rng.standard_normal((prob.nx, a.batch)))))
    return s, prob


def child(pkg, a):
    """One process: one leg's kernel time on whatever library this process loaded; the cones-A leg also times the verbs. One line."""
    s, prob = make(pkg, a.child, a)
    s.solve_timed()  # warm-up: first launch, table builds
    out = dict(leg=a.child, kernel_ms=float(np.median([s.solve_timed() for _ in range(a.reps)])),
               kernel="%s %s" % (s.launch_info()["layout"], s.jit_info()))
    if a.child == "cones-A":
        L, dp = pkg.load_library(), pkg._lib.c_double_p
        host = slopes(prob, a.batch)
        dev = device_copy(pkg, host)
        wall, wall_dev = [], []
        for _ in range(1 + a.reps):
            t0 = time.perf_counter()
            rc = L.tinympc_set_cone_slopes_batch(s._h, host[0].ctypes.data_as(dp), 1, host[1].ctypes.data_as(dp), 1, 0, a.batch)
            wall.append(1e3 * (time.perf_counter() - t0))
            assert rc == 0, pkg._lib.last_error()
        for _ in range(a.reps if dev else 0):
            t0 = time.perf_counter()
            rc = L.tinympc_set_cone_slopes_batch_device(s._h, dev[0], 1, dev[1], 1, 0, a.batch)
            wall_dev.append(1e3 * (time.perf_counter() - t0))
            assert rc == 0, pkg._lib.last_error()
        out.update(verb_host_ms=wall, verb_device_ms=wall_dev)
    s.reset()
    print("CONE-CHILD " + json.dumps(out), flush=True)


def sweep(a):
    """Starts the children (it never opens the GPU itself) and prints the table."""
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("needs --parent-lib: libtinympc_hip.so built from the parent commit")
    recs = {leg: [] for leg in LEGS}
    for rnd in range(a.rounds):
        for leg in LEGS if rnd % 2 == 0 else LEGS[::-1]:
            env = dict(os.environ)
            env.pop("TINYMPC_LAYOUT", None)
            env.pop("TINYMPC_HIP_LIBRARY", None)
            if leg.startswith("parent"):
                env["TINYMPC_HIP_LIBRARY"] = os.path.abspath(a.parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--batch", str(a.batch), "--iters", str(a.iters),
                                "--reps", str(a.reps)], env=env, capture_output=True, text=True, timeout=300)
            line = [l for l in r.stdout.splitlines() if l.startswith("CONE-CHILD ")]
            if r.returncode != 0 or not line:
                raise SystemExit("round %d (%s) failed with %d:\n%s\n%s" % (rnd, leg, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            recs[leg].append(json.loads(line[0][len("CONE-CHILD "):]))
            print("# round %d %-9s %.4f ms" % (rnd, leg, recs[leg][-1]["kernel_ms"]), flush=True)
    print("per-instance cone slopes: %d instances x %d forced iterations; kernel ms (median of %d launches per round, %d rounds, a fresh process "
          "each, legs alternating). parent / new: quadrotors N=20 with one state and one input row per instance; cones / shared: rocket "
          "landings N=10, slopes per instance / shared" % (a.batch, a.iters, a.reps, a.rounds))
    ms = {leg: [r["kernel_ms"] for r in recs[leg]] for leg in LEGS}
    for leg in LEGS:
        print("%-9s | %s | median %.4f | spread %.4f - %.4f | %s" % (leg, " ".join("%.4f" % v for v in ms[leg]), float(np.median(ms[leg])),
                                                                    min(ms[leg]), max(ms[leg]), recs[leg][0]["kernel"]))
    for new, old in (("new-A", "parent-A"), ("new-D", "parent-D")):
        med, lo, hi = float(np.median(ms[new])), min(ms[old]), max(ms[old])
        print("(a) %s median inside %s's spread: %s (%.4f against %.4f - %.4f; ratio of medians %.4f)"
              % (new, old, "yes" if lo <= med <= hi else ("below it" if med < lo else "NO"), med, lo, hi, med / float(np.median(ms[old]))))
    for key, name in (("verb_host_ms", "set_cone_slopes_batch"), ("verb_device_ms", "set_cone_slopes_batch_device")):
        first = [r[key][0] for r in recs["cones-A"] if r[key]]
        rest = [v for r in recs["cones-A"] for v in (r[key][1:] if key == "verb_host_ms" else r[key])]
        if not rest:
            print("%-30s not measured (no device memory could be filled)" % name)
            continue
        print("%-30s %d instances, wall ms: %s median %.3f (min %.3f, max %.3f)"
              % (name, a.batch, ("first repeat %s | repeats" % " ".join("%.3f" % v for v in first)) if key == "verb_host_ms" else "calls",
                 float(np.median(rest)), min(rest), max(rest)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--parent-lib", default="")
    a = ap.parse_args()
    if not a.child:
        return sweep(a)
    import __graft_entry__ as ge
    child(ge.load_package(), a)


if __name__ == "__main__":
    main()
