"""What the wait in front of the completion stamp costs (host_stores_retired, tinympc_device.h): closed-loop ticks of single-instance
handles, this build against the parent commit's library (tools/bin/parent/libtinympc_hip.so, built from the previous commit and named
through TINYMPC_HIP_LIBRARY), alternating FRESH child processes, four rounds. Shapes: quadrotor N=50 and cartpole N=20 (layout F, compiled
in) and cartpole N=10 (layout C); the resident session tick and the launched mpc_step tick; per round the median and mean of three runs
of 600 timed ticks, then the median and the spread of the rounds; for layout F's session also the kernel's own split of the tick
(tinympc_debug_tick_timing: waited / iterations / write-out -- the wait sits in the write-out). Modelled on tools/mailbox_ab.py.
    python tools/stamp_order_ab.py [--rounds 4] [--out profiles/stamp_order_ab.txt]     (GPU box)"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = os.path.join(ROOT, "tools", "bin", "parent", "libtinympc_hip.so")
CHILD_LIMIT = 240  # seconds; a child takes well under a minute (resident kernels are involved: nothing may wait for ever)

if len(sys.argv) > 1 and sys.argv[1] == "--child":
    import numpy as np
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package(); P = pkg.problems
    L = pkg.load_library()
    for name, prob in (("quadrotor N=50", P.quadrotor(50)), ("cartpole N=20", P.cartpole(20)), ("cartpole N=10", P.cartpole(10))):
        for session in (True, False):
            s = pkg.TinyMPC()
            s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=1, rho=prob.rho, max_iter=100, abs_pri_tol=1e-3, abs_dua_tol=1e-3)
            s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
            if session: s.session_begin()
            meds, means, its, brk, dbg = [], [], 0, [], np.zeros(4)
            for rep in range(3):
                x = prob.x0.copy(); d = []; its = 0
                for k in range(620):
                    t0 = time.perf_counter()
                    u = s.session_step(x) if session else s.mpc_step(x)[:, 0]
                    dt = time.perf_counter() - t0
                    if k >= 20:
                        d.append(1e6 * dt); its += s.get_stats()["iter"]
                        if session and hasattr(L, "tinympc_debug_tick_timing"):
                            L.tinympc_debug_tick_timing(s._h, dbg.ctypes.data_as(pkg._lib.c_double_p)); brk.append(dbg[:3].copy())
                    x = prob.A @ x + prob.B @ u
                meds.append(float(np.median(d))); means.append(float(np.mean(d)))
            split = [float(v) for v in np.median(np.array(brk), axis=0)] if brk and np.any(np.array(brk)) else None
            print("RESULT " + json.dumps(dict(shape=name, mode="session" if session else "launch", layout=s.launch_info()["layout"], median=sorted(meds)[1],
                                              mean=sorted(means)[1], iters=its / 600, split=split)), flush=True)
            if session: s.session_end()
            s.reset()
    sys.exit(0)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stamp_order_ab.txt"))
a = ap.parse_args()
if not os.path.exists(PARENT):
    sys.exit("no parent library at %s: build the previous commit and copy its libtinympc_hip.so there" % os.path.relpath(PARENT, ROOT))
lines, rows = [], {}  # rows[(shape, mode)][build] = list of per-round results


def say(text):
    print(text, flush=True)
    lines.append(text)
    with open(a.out, "w") as f:  # (rewritten as the run goes: a run that is cut short leaves what it had)
        f.write("\n".join(lines) + "\n")


say("completion stamp behind retired host stores: this build (wait) against the parent commit's library (parent), alternating fresh processes")
say("us per closed-loop tick, host clock around session_step / mpc_step; per round: median and mean of three runs of 600 ticks (the middle one of each)")
for rnd in range(a.rounds):
    for build in ("parent", "wait") if rnd % 2 == 0 else ("wait", "parent"):
        env = dict(os.environ)
        env.pop("TINYMPC_HIP_LIBRARY", None)
        if build == "parent": env["TINYMPC_HIP_LIBRARY"] = PARENT
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=CHILD_LIMIT)
        if r.returncode != 0:
            say("round %d, %s: the child ended with status %d -- stopping here\n%s" % (rnd, build, r.returncode, (r.stdout + r.stderr)[-1500:]))
            sys.exit(1)
        for ln in r.stdout.splitlines():
            if ln.startswith("RESULT "):
                d = json.loads(ln[7:])
                rows.setdefault((d["shape"], d["mode"]), {}).setdefault(build, []).append(d)
                say("round %d  %-6s  %-15s %-7s layout %s  median %7.2f  mean %7.2f  iterations per tick %.2f%s" % (
                    rnd, build, d["shape"], d["mode"], d["layout"], d["median"], d["mean"], d["iters"],
                    "   in the kernel: waited %.2f, iterations %.2f, write-out %.2f us" % tuple(d["split"]) if d["split"] else ""))
say("")
say("over the rounds: median of the rounds' medians [lowest .. highest]")
med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else 0.5 * (sorted(v)[len(v) // 2 - 1] + sorted(v)[len(v) // 2])
for (shape, mode), by in rows.items():
    for build in ("parent", "wait"):
        m = [d["median"] for d in by[build]]
        w = [d["split"][2] for d in by[build] if d["split"]]
        say("%-15s %-7s %-6s  %7.2f us  [%6.2f .. %6.2f]   mean %7.2f%s" % (shape, mode, build, med(m), min(m), max(m), med([d["mean"] for d in by[build]]),
            "   write-out in the kernel %.2f us [%.2f .. %.2f]" % (med(w), min(w), max(w)) if w else ""))
    p, w = [d["median"] for d in by["parent"]], [d["median"] for d in by["wait"]]
    say("%-15s %-7s wait - parent: %+.2f us; %s the parent's spread" % (shape, mode, med(w) - med(p), "inside" if min(p) <= med(w) <= max(p) else "OUTSIDE"))
