"""Slot refill for layout D's per-instance goal form against the PARENT commit's library on the same handle: 65,536 and 16,384
quadrotors N=50, one goal (set_x_ref_batch / set_u_ref_batch) and one box (set_bound_constraints_batch) per instance, tolerances
1e-3, max_iter 200, cold solves timed with tinympc_solve_timed. Legs, every one a fresh process, alternating, `--rounds` times each:
    parent-goal   the parent's library (--parent-lib): the handle runs the plain goal kernel, k_admm_solve_d_gbnd -- the yardstick
    goal-refill   this tree, TINYMPC_REFILL=1: k_admm_solve_d_refill_gbnd
    shared-refill this tree, the same x0s with the shared reference and box: k_admm_solve_d_refill -- the floor, for context only
The first-controls hash of parent-goal and goal-refill must be equal (the tool exits 1 otherwise). The default is on only if
goal-refill lies below parent-goal in EVERY round at 65,536 instances.
    python tools/refill_goal_ab.py --parent-lib /path/to/parent/libtinympc_hip.so"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("parent-goal", "goal-refill", "shared-refill")


def child(a):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    P = pkg.problems
    prob, nb = P.quadrotor(50), a.batch
    rng = np.random.default_rng(0)
    x0s = np.asfortranarray(P.quadrotor_batch_x0(nb) * rng.uniform(0.05, 3.0, nb)[None, :])
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=nb, rho=prob.rho, max_iter=200, abs_pri_tol=1e-3, abs_dua_tol=1e-3)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if a.child != "shared-refill":
        gx = np.zeros((12, nb))
        gx[:3] = 0.1 * rng.standard_normal((3, nb))
        gu = 0.02 * rng.standard_normal((4, nb))
        w = rng.uniform(0.6, 1.0, nb)
        s.set_x_ref_batch(gx)
        s.set_u_ref_batch(gu)
        s.set_bound_constraints_batch(np.repeat(prob.x_min[:, None], nb, axis=1), np.repeat(prob.x_max[:, None], nb, axis=1),
                                      prob.u_min[:, None] * w[None, :], prob.u_max[:, None] * w[None, :])
    s.set_x0_batch(x0s)
    for _ in range(a.warmup):
        s.reset_workspace()
        s.solve_timed()
    ms = []
    for _ in range(a.reps):
        s.reset_workspace()
        ms.append(s.solve_timed())
    u, it = s.get_first_controls_batch(), s.get_stats_batch()["iter"]
    print(json.dumps({"median": float(np.median(ms)), "min": float(np.min(ms)), "kernel": s.jit_info(), "iters": [int(it.min()), float(it.mean()), int(it.max())],
                      "sha": hashlib.sha256(np.ascontiguousarray(u).tobytes()).hexdigest()[:12]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib is required: libtinympc_hip.so built from the parent commit (never this tree's TINYMPC_REFILL=0)")
    ok = True
    for nb in (65536, 16384):
        recs = {leg: [] for leg in LEGS}
        for rnd in range(a.rounds):
            for leg in LEGS if rnd % 2 == 0 else LEGS[::-1]:
                env = dict(os.environ)
                env.pop("TINYMPC_HIP_LIBRARY", None)
                env.pop("TINYMPC_REFILL", None)
                if leg == "parent-goal":
                    env["TINYMPC_HIP_LIBRARY"] = os.path.abspath(a.parent_lib)
                else:
                    env["TINYMPC_REFILL"] = "1"
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--batch", str(nb), "--warmup", str(a.warmup), "--reps", str(a.reps)],
                                   env=env, capture_output=True, text=True, timeout=300)
                if r.returncode:
                    print(f"{leg} FAILED (exit {r.returncode}): {r.stderr[-300:]}", flush=True)
                    return 1  # (nothing more is started after a failed leg)
                d = json.loads(r.stdout.strip().splitlines()[-1])
                recs[leg].append(d)
                print(f"{nb:6d} instances  round {rnd}  {leg:13s} median {d['median']:8.4f} ms  min {d['min']:8.4f}  iterations {d['iters'][0]}/{d['iters'][1]:.1f}/{d['iters'][2]}"
                      f"  first controls {d['sha']}  [{d['kernel']}]", flush=True)
        for leg in LEGS:
            print(f"# {nb} instances, {leg}: median of rounds {float(np.median([d['median'] for d in recs[leg]])):.4f} ms")
        below = [g["median"] < p["median"] for g, p in zip(recs["goal-refill"], recs["parent-goal"])]
        same = len({d["sha"] for d in recs["parent-goal"] + recs["goal-refill"]}) == 1
        print(f"# {nb} instances: goal-refill below parent-goal in {sum(below)} of {len(below)} rounds; first controls {'identical' if same else 'DIFFER'}", flush=True)
        ok = ok and same
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
