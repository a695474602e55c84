"""Slot refill for layout D's per-instance trajectory form (and its per-knot bounds form) against the PARENT commit's library on the same
handle: quadrotors with one reference trajectory per instance (set_x_ref_batch / set_u_ref_batch after prepare()), tolerances 1e-3,
max_iter 200, cold solves timed with tinympc_solve_timed. Cases: N=50 with trajectories at 65,536 instances (16 resident sets) and at
8,192 (two); N=20 with bounds per knot and instance beside the trajectories at the same two sizes. Legs, every one a fresh process,
alternating, `--rounds` times each:
    parent-plain  the parent's library (--parent-lib): the handle runs the plain trajectory form -- the yardstick
    traj-refill   this tree, TINYMPC_REFILL=1: the form's slot-refill variant
The first-controls hash of the two legs must be equal (the tool exits 1 otherwise). The default is on only if traj-refill lies below
parent-plain in EVERY round at 65,536 instances of the N=50 trajectory case.
    python tools/refill_traj_ab.py --parent-lib /path/to/parent/libtinympc_hip.so"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("parent-plain", "traj-refill")
CASES = ((50, False, 65536), (50, False, 8192), (20, True, 65536), (20, True, 8192))  # (N, bounds per knot?, instances)


def child(a):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    P = pkg.problems
    prob, nb, N = P.quadrotor(a.horizon), a.batch, a.horizon
    rng = np.random.default_rng(0)
    x0s = np.asfortranarray(P.quadrotor_batch_x0(nb) * rng.uniform(0.02, 1.0, nb)[None, :])
    gx, gu = 0.04 * rng.standard_normal((12, nb)), 0.005 * rng.standard_normal((4, nb))
    t = np.linspace(0.0, 1.0, N)
    X = np.asfortranarray(gx[:, None, :] * (1.0 + 0.5 * np.sin(3.0 * t + np.arange(12)[:, None]))[:, :, None])
    U = np.asfortranarray(gu[:, None, :] * np.cos(2.0 * t[: N - 1])[None, :, None])
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=nb, rho=prob.rho, max_iter=200, abs_pri_tol=1e-3, abs_dua_tol=1e-3)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    s.prepare()
    s.set_x_ref_batch(X)
    s.set_u_ref_batch(U)
    if a.kbnd:  # every instance's own input limits, breathing over the horizon
        w = rng.uniform(0.6, 1.0, nb)
        f = 1.0 + 0.2 * np.sin(0.4 * np.arange(N)[:, None] + rng.uniform(0, 6, nb)[None, :])  # N x batch
        xl, xh = (np.asfortranarray(np.repeat(np.repeat(v[:, None, None], N, axis=1), nb, axis=2)) for v in (prob.x_min, prob.x_max))
        ul, uh = (np.asfortranarray(v[:, None, None] * (w[None, :] * f[: N - 1])[None]) for v in (prob.u_min, prob.u_max))
        s.set_bound_constraints_batch(xl, xh, ul, uh)
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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--horizon", type=int, default=50)
    ap.add_argument("--kbnd", type=int, default=0)
    ap.add_argument("--cases", default="", help="indices into CASES, comma separated (default: all)")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib is required: libtinympc_hip.so built from the parent commit (never this tree's TINYMPC_REFILL=0)")
    ok = True
    for N, kbnd, nb in [CASES[int(i)] for i in a.cases.split(",")] if a.cases else CASES:
        tag = f"N={N}{' traj+kbnd' if kbnd else ' traj'} {nb:6d} instances"
        recs = {leg: [] for leg in LEGS}
        for rnd in range(a.rounds):
            for leg in LEGS if rnd % 2 == 0 else LEGS[::-1]:
                env = dict(os.environ)
                env.pop("TINYMPC_HIP_LIBRARY", None)
                env.pop("TINYMPC_REFILL", None)
                if leg == "parent-plain":
                    env["TINYMPC_HIP_LIBRARY"] = os.path.abspath(a.parent_lib)
                else:
                    env["TINYMPC_REFILL"] = "1"
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--batch", str(nb), "--horizon", str(N), "--kbnd", str(int(kbnd)),
                                    "--warmup", str(a.warmup), "--reps", str(a.reps)], env=env, capture_output=True, text=True, timeout=300)
                if r.returncode:
                    print(f"{leg} FAILED (exit {r.returncode}): {r.stderr[-300:]}", flush=True)
                    return 1  # (nothing more is started after a failed leg)
                d = json.loads(r.stdout.strip().splitlines()[-1])
                recs[leg].append(d)
                print(f"{tag}  round {rnd}  {leg:12s} median {d['median']:8.4f} ms  min {d['min']:8.4f}  iterations {d['iters'][0]}/{d['iters'][1]:.1f}/{d['iters'][2]}"
                      f"  first controls {d['sha']}  [{d['kernel']}]", flush=True)
        for leg in LEGS:
            print(f"# {tag}, {leg}: median of rounds {float(np.median([d['median'] for d in recs[leg]])):.4f} ms")
        below = [g["median"] < p["median"] for g, p in zip(recs["traj-refill"], recs["parent-plain"])]
        same = len({d["sha"] for d in recs["parent-plain"] + recs["traj-refill"]}) == 1
        print(f"# {tag}: traj-refill below parent-plain in {sum(below)} of {len(below)} rounds; first controls {'identical' if same else 'DIFFER'}", flush=True)
        ok = ok and same
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
