"""Per-instance linear rows at bench size.

Kernel milliseconds (HIP events, tinympc_solve_timed) of the same forced-iteration solve of `--batch` quadrotors (N = `--N`, `--iters`
iterations, one state row plus one input row) with
  shared-A   the rows shared (tinympc_set_linear_constraints), the handle forced to layout A (TINYMPC_LAYOUT=A): k_admm_solve_fam --
             the yardstick: the same inner loop, the rows from the shared description
  per-inst   the SAME rows sent per instance (tinympc_set_linear_constraints_batch): k_admm_solve_ifam
Every measurement is a fresh process; the two legs alternate, `--rounds` times each, so they share the call's noise. Reported: each
round's median of `--reps` launches, the legs' medians and spreads, and whether per-inst's median lies inside shared-A's spread.
Beside the legs: the same shared-row handle on the layout it picks by default (context), and the wall time of
set_linear_constraints_batch and of its _device form for the whole batch (first call, which allocates the store, and repeats).
    python tools/instance_lin_sweep.py [--batch 8192] [--N 20] [--iters 100] [--rounds 4] [--reps 5]

Layout D (--d --parent-lib PATH): the same workload on a handle that called prepare(), with
  parent-A    the rows per instance on the library of the parent commit at PATH (built from a checkout of the parent): layout A's
              k_admm_solve_ifam, where the mode ran before layout D had a form for it -- the yardstick
  inst-D      the rows per instance on this tree's library: layout D's per-instance linear-row form
  shared-D    the same rows shared (tinympc_set_linear_constraints) on the layout the handle picks, layout D's families kernel -- the
              floor; context, not a condition
  parent-A-4, inst-D-4   a second point with four state rows and four input rows (where the form's plan accepts it): what the
              per-wavefront LDS term does to the plan
Every measurement is a fresh process; the legs alternate, `--rounds` times each. The bar: inst-D lies below parent-A in EVERY round;
the margin is reported against the spread of parent-A's rounds.
    python tools/instance_lin_sweep.py --d --parent-lib /path/to/parent/libtinympc_hip.so

Rows per knot (--knots [--parent-lib PATH] [--alt-lib PATH]): the same workload on layout A, with
  const-A     the rows per instance, constant over the horizon (tinympc_set_linear_constraints_batch): k_admm_solve_ifam -- the yardstick
  knots-same  the same rows repeated over the knots through tinympc_set_linear_constraints_knots_batch: k_admm_solve_ifamk
  knots-vary  rows that differ per knot and instance through the same verb
  parent-A    const-A on the library of the parent commit at --parent-lib: did the yardstick stay inside the parent's spread?
  alt-same, alt-vary   the two knot legs on another build of this tree at --alt-lib (a variant of the kernel to compare against)
and the wall time of tinympc_set_linear_constraints_knots_batch and of its _device form for the whole batch. No ratio is a condition;
medians and spreads are reported, and the knot legs' distance to const-A.
    python tools/instance_lin_sweep.py --knots --parent-lib /path/to/parent/libtinympc_hip.so

Rows per knot on layout D (--knots --d --parent-lib PATH): the --knots workload, rows that differ per knot and instance, on a handle
that called prepare(), with
  parent-A    the handle on the library of the parent commit at PATH: layout A's k_admm_solve_ifamk, where the mode ran before layout D
              had a form for it -- the yardstick
  knots-D     the same handle on this tree's library: the per-knot variant of layout D's per-instance linear-row form
  const-D     rows constant over the horizon on layout D's per-instance linear-row form -- the floor; context, not a condition
Every measurement is a fresh process; the legs alternate, `--rounds` times each. The bar: knots-D lies below parent-A in EVERY round.
    python tools/instance_lin_sweep.py --knots --d --parent-lib /path/to/parent/libtinympc_hip.so"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ["shared-A", "per-inst"]
D_LEGS = ["parent-A", "inst-D", "shared-D", "parent-A-4", "inst-D-4"]
K_LEGS = ["const-A", "knots-same", "knots-vary"]
KD_LEGS = ["parent-A", "knots-D", "const-D"]


def rows(prob, batch, seed=7, n=1):
    """n state rows and n input rows (one each by default), the same for every instance: (Ax (n, nx), bx (n,), Au (n, nu), bu (n,))."""
    rng = np.random.default_rng(seed)
    ax, au = rng.standard_normal((n, prob.nx)), rng.standard_normal((n, prob.nu))
    ax, au = ax / np.linalg.norm(ax, axis=1, keepdims=True), au / np.linalg.norm(au, axis=1, keepdims=True)
    return ax, ax @ prob.x0 + 0.3, au, np.full(n, 0.2)


def make(pkg, leg, a):
    prob = pkg.problems.quadrotor(a.N)
    if leg == "shared-A":
        os.environ["TINYMPC_LAYOUT"] = "A"
    else:
        os.environ.pop("TINYMPC_LAYOUT", None)
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=a.batch, rho=prob.rho, abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=a.iters)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    ax, bx, au, bu = rows(prob, a.batch)
    if leg == "per-inst":
        s.set_linear_constraints_batch(*(np.repeat(m[..., None], a.batch, axis=-1) for m in (ax, bx, au, bu)))
    else:
        s.set_linear_constraints(ax, bx, au, bu)
    s.set_x0_batch(pkg.problems.quadrotor_batch_x0(a.batch))
    return s


def make_d(pkg, leg, a):
    """The --d legs: the handle as setup makes it (layout D at this batch size), the rows per instance or shared, then prepare()."""
    prob = pkg.problems.quadrotor(a.N)
    os.environ.pop("TINYMPC_LAYOUT", None)
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=a.batch, rho=prob.rho, abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=a.iters)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    ax, bx, au, bu = rows(prob, a.batch, n=4 if leg.endswith("-4") else 1)
    if leg.startswith("shared"):
        s.set_linear_constraints(ax, bx, au, bu)
    else:
        s.set_linear_constraints_batch(*(np.repeat(m[..., None], a.batch, axis=-1) for m in (ax, bx, au, bu)))
    s.prepare()
    s.set_x0_batch(pkg.problems.quadrotor_batch_x0(a.batch))
    return s


def child_d(pkg, a):
    """One process of the --d sweep: one leg's kernel time on whatever library this process loaded. One line."""
    s = make_d(pkg, a.child, a)
    s.solve_timed()  # warm-up: first launch, table builds
    out = dict(leg=a.child, kernel_ms=float(np.median([s.solve_timed() for _ in range(a.reps)])),
               kernel="%s %s" % (s.launch_info()["layout"], s.jit_info()), lds_bytes=s.launch_info()["lds_bytes"],
               workgroups=s.launch_info()["workgroups"])
    s.reset()
    print("LIN-CHILD " + json.dumps(out), flush=True)


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
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--d", "--child", leg, "--batch", str(a.batch), "--N", str(a.N),
                                "--iters", str(a.iters), "--reps", str(a.reps)], env=env, capture_output=True, text=True, timeout=300)
            line = [l for l in r.stdout.splitlines() if l.startswith("LIN-CHILD ")]
            if r.returncode != 0 or not line:
                raise SystemExit("round %d (%s) failed with %d:\n%s\n%s" % (rnd, leg, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            recs[leg].append(json.loads(line[0][len("LIN-CHILD "):]))
            print("# round %d %-10s %.4f ms" % (rnd, leg, recs[leg][-1]["kernel_ms"]), flush=True)
    print("per-instance linear rows on layout D: %d quadrotors N=%d x %d forced iterations, n state rows + n input rows (n = 1; the -4 legs: "
          "n = 4), every handle after prepare(); kernel ms (median of %d launches per round, %d rounds, a fresh process each, legs alternating)"
          % (a.batch, a.N, a.iters, a.reps, a.rounds))
    ms = {leg: [r["kernel_ms"] for r in recs[leg]] for leg in D_LEGS}
    for leg in D_LEGS:
        print("%-10s | %s | median %.4f | spread %.4f - %.4f | %d workgroups, %d bytes of LDS each | %s"
              % (leg, " ".join("%.4f" % v for v in ms[leg]), float(np.median(ms[leg])), min(ms[leg]), max(ms[leg]), recs[leg][0]["workgroups"],
                 recs[leg][0]["lds_bytes"], recs[leg][0]["kernel"]))
    for new, old in (("inst-D", "parent-A"), ("inst-D-4", "parent-A-4")):
        on_d = recs[new][0]["kernel"].startswith("D ")
        below = all(n < o for n, o in zip(ms[new], ms[old]))
        print("%s on layout D: %s; below %s in every round: %s (largest %.4f against smallest %.4f, %s's spread %.4f; ratio of medians %.3f)"
              % (new, "yes" if on_d else "NO", old, "yes" if below else "NO", max(ms[new]), min(ms[old]), old, max(ms[old]) - min(ms[old]),
                 float(np.median(ms[new])) / float(np.median(ms[old]))))
    print("distance to the floor: inst-D median %.4f against shared-D median %.4f (ratio %.3f)"
          % (float(np.median(ms["inst-D"])), float(np.median(ms["shared-D"])), float(np.median(ms["inst-D"])) / float(np.median(ms["shared-D"]))))


def knot_rows(prob, batch, vary, seed=7):
    """One state row and one input row per knot and instance in the knot verb's shapes: rows()'s, repeated (vary = False), or random unit
    rows per knot and instance with the same offsets (vary = True)."""
    ax, bx, au, bu = rows(prob, batch, seed)
    N = prob.N
    if not vary:
        return (np.repeat(np.repeat(ax[:, :, None, None], N, axis=2), batch, axis=3), np.repeat(np.repeat(bx[:, None, None], N, axis=1), batch, axis=2),
                np.repeat(np.repeat(au[:, :, None, None], N - 1, axis=2), batch, axis=3), np.repeat(np.repeat(bu[:, None, None], N - 1, axis=1), batch, axis=2))
    rng = np.random.default_rng(seed + 1)
    Ax, Au = rng.standard_normal((1, prob.nx, N, batch)), rng.standard_normal((1, prob.nu, N - 1, batch))
    Ax, Au = Ax / np.linalg.norm(Ax, axis=1, keepdims=True), Au / np.linalg.norm(Au, axis=1, keepdims=True)
    return Ax, np.einsum("kcnb,c->knb", Ax, prob.x0) + 0.3, Au, np.full((1, N - 1, batch), 0.2)


def child_k(pkg, a):
    """One process of the --knots sweep: one leg's kernel time on whatever library this process loaded; the knots-vary leg also times the
    verb. One line."""
    prob = pkg.problems.quadrotor(a.N)
    os.environ.pop("TINYMPC_LAYOUT", None)
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=a.batch, rho=prob.rho, abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=a.iters)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if a.child in ("const-A", "parent-A"):
        s.set_linear_constraints_batch(*(np.repeat(m[..., None], a.batch, axis=-1) for m in rows(prob, a.batch)))
    else:
        s.set_linear_constraints_knots_batch(*knot_rows(prob, a.batch, a.child.endswith("vary")))
    s.set_x0_batch(pkg.problems.quadrotor_batch_x0(a.batch))
    s.solve_timed()  # warm-up: first launch, table builds
    out = dict(leg=a.child, kernel_ms=float(np.median([s.solve_timed() for _ in range(a.reps)])),
               kernel="%s %s" % (s.launch_info()["layout"], s.jit_info()))
    if a.child == "knots-vary":
        L, dp = pkg.load_library(), pkg._lib.c_double_p
        host = [np.asfortranarray(m) for m in knot_rows(prob, a.batch, True)]
        dev = device_copy(pkg, host)
        fresh = pkg.TinyMPC()
        fresh.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=a.batch, rho=prob.rho)
        wall, wall_dev = [], []
        for _ in range(1 + a.reps):
            t0 = time.perf_counter()
            rc = L.tinympc_set_linear_constraints_knots_batch(fresh._h, host[0].ctypes.data_as(dp), host[1].ctypes.data_as(dp), 1,
                                                              host[2].ctypes.data_as(dp), host[3].ctypes.data_as(dp), 1, 0, a.batch)
            wall.append(1e3 * (time.perf_counter() - t0))
            assert rc == 0, pkg._lib.last_error()
        for _ in range(a.reps if dev else 0):
            t0 = time.perf_counter()
            rc = L.tinympc_set_linear_constraints_knots_batch_device(fresh._h, dev[0], dev[1], 1, dev[2], dev[3], 1, 0, a.batch)
            wall_dev.append(1e3 * (time.perf_counter() - t0))
            assert rc == 0, pkg._lib.last_error()
        out.update(verb_host_ms=wall, verb_device_ms=wall_dev)
        fresh.reset()
    s.reset()
    print("LIN-CHILD " + json.dumps(out), flush=True)


def sweep_k(a):
    """Starts the children of the --knots sweep (it never opens the GPU itself) and prints the table."""
    legs = list(K_LEGS)
    libs = {}
    if a.parent_lib:
        legs.append("parent-A")
        libs["parent-A"] = a.parent_lib
    if a.alt_lib:
        legs += ["alt-same", "alt-vary"]
        libs["alt-same"] = libs["alt-vary"] = a.alt_lib
    for path in libs.values():
        if not os.path.exists(path):
            raise SystemExit("no library at " + path)
    recs = {leg: [] for leg in legs}
    for rnd in range(a.rounds):
        for leg in legs if rnd % 2 == 0 else legs[::-1]:
            env = dict(os.environ)
            env.pop("TINYMPC_LAYOUT", None)
            env.pop("TINYMPC_HIP_LIBRARY", None)
            if leg in libs:
                env["TINYMPC_HIP_LIBRARY"] = os.path.abspath(libs[leg])
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--knots", "--child", leg, "--batch", str(a.batch), "--N", str(a.N),
                                "--iters", str(a.iters), "--reps", str(a.reps)], env=env, capture_output=True, text=True, timeout=300)
            line = [l for l in r.stdout.splitlines() if l.startswith("LIN-CHILD ")]
            if r.returncode != 0 or not line:
                raise SystemExit("round %d (%s) failed with %d:\n%s\n%s" % (rnd, leg, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            recs[leg].append(json.loads(line[0][len("LIN-CHILD "):]))
            print("# round %d %-10s %.4f ms" % (rnd, leg, recs[leg][-1]["kernel_ms"]), flush=True)
    print("per-knot linear rows on layout A: %d quadrotors N=%d x %d forced iterations, 1 state row + 1 input row; kernel ms (median of %d "
          "launches per round, %d rounds, a fresh process each, legs alternating)" % (a.batch, a.N, a.iters, a.reps, a.rounds))
    ms = {leg: [r["kernel_ms"] for r in recs[leg]] for leg in legs}
    for leg in legs:
        print("%-10s | %s | median %.4f | spread %.4f - %.4f | %s" % (leg, " ".join("%.4f" % v for v in ms[leg]), float(np.median(ms[leg])),
                                                                     min(ms[leg]), max(ms[leg]), recs[leg][0]["kernel"]))
    base = float(np.median(ms["const-A"]))
    steps = a.iters * (a.N - 1)
    for leg in legs:
        if leg in ("const-A", "parent-A"):
            continue
        med = float(np.median(ms[leg]))
        waves = (a.batch + 3) // 4  # (16 lanes per instance: four instances per wavefront)
        mb = waves * 3 * 512 / 1e6  # one slot of 3 nl = 3 vectors of 512 bytes per wavefront and forward step
        print("%-10s against const-A: ratio of medians %.3f, +%.4f ms over %d forward steps; the slots read are %d wavefronts x 3 lines x 512 B = "
              "%.2f MB per step, %.2f GB per solve (%.1f TB/s if the difference were that traffic alone)"
              % (leg, med / base, med - base, steps, waves, mb, mb * steps / 1e3, mb * steps / 1e6 / ((med - base) / 1e3) if med > base else float("nan")))
    if "parent-A" in ms:
        med, lo, hi = base, min(ms["parent-A"]), max(ms["parent-A"])
        print("const-A median inside parent-A's spread: %s (%.4f against %.4f - %.4f; ratio of medians %.3f)"
              % ("yes" if lo <= med <= hi else "NO", med, lo, hi, med / float(np.median(ms["parent-A"]))))
    for key, name in (("verb_host_ms", "set_linear_constraints_knots_batch"), ("verb_device_ms", "set_linear_constraints_knots_batch_device")):
        first = [r[key][0] for r in recs["knots-vary"] if r[key]]
        rest = [v for r in recs["knots-vary"] for v in (r[key][1:] if key == "verb_host_ms" else r[key])]
        if not rest:
            print("%-42s not measured (no device memory could be filled)" % name)
            continue
        print("%-42s %d instances, wall ms: %s median %.3f (min %.3f, max %.3f)"
              % (name, a.batch, ("first call %s | repeats" % " ".join("%.3f" % v for v in first)) if key == "verb_host_ms" else "calls",
                 float(np.median(rest)), min(rest), max(rest)))


def child_kd(pkg, a):
    """One process of the --knots --d sweep: one leg's kernel time on whatever library this process loaded. One line."""
    prob = pkg.problems.quadrotor(a.N)
    os.environ.pop("TINYMPC_LAYOUT", None)
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=a.batch, rho=prob.rho, abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=a.iters)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if a.child == "const-D":
        s.set_linear_constraints_batch(*(np.repeat(m[..., None], a.batch, axis=-1) for m in rows(prob, a.batch)))
    else:
        s.set_linear_constraints_knots_batch(*knot_rows(prob, a.batch, True))
    s.prepare()
    s.set_x0_batch(pkg.problems.quadrotor_batch_x0(a.batch))
    s.solve_timed()  # warm-up: first launch, table builds
    out = dict(leg=a.child, kernel_ms=float(np.median([s.solve_timed() for _ in range(a.reps)])),
               kernel="%s %s" % (s.launch_info()["layout"], s.jit_info()), lds_bytes=s.launch_info()["lds_bytes"],
               workgroups=s.launch_info()["workgroups"])
    s.reset()
    print("LIN-CHILD " + json.dumps(out), flush=True)


def sweep_kd(a):
    """Starts the children of the --knots --d sweep (it never opens the GPU itself) and prints the table."""
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--knots --d needs --parent-lib: libtinympc_hip.so built from the parent commit")
    recs = {leg: [] for leg in KD_LEGS}
    for rnd in range(a.rounds):
        for leg in KD_LEGS if rnd % 2 == 0 else KD_LEGS[::-1]:
            env = dict(os.environ)
            env.pop("TINYMPC_LAYOUT", None)
            env.pop("TINYMPC_HIP_LIBRARY", None)
            if leg.startswith("parent"):
                env["TINYMPC_HIP_LIBRARY"] = os.path.abspath(a.parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--knots", "--d", "--child", leg, "--batch", str(a.batch), "--N", str(a.N),
                                "--iters", str(a.iters), "--reps", str(a.reps)], env=env, capture_output=True, text=True, timeout=300)
            line = [l for l in r.stdout.splitlines() if l.startswith("LIN-CHILD ")]
            if r.returncode != 0 or not line:
                raise SystemExit("round %d (%s) failed with %d:\n%s\n%s" % (rnd, leg, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            recs[leg].append(json.loads(line[0][len("LIN-CHILD "):]))
            print("# round %d %-10s %.4f ms" % (rnd, leg, recs[leg][-1]["kernel_ms"]), flush=True)
    print("per-knot linear rows on layout D: %d quadrotors N=%d x %d forced iterations, 1 state row + 1 input row that differ per knot and "
          "instance (const-D: constant over the horizon), every handle after prepare(); kernel ms (median of %d launches per round, %d rounds, a "
          "fresh process each, legs alternating)" % (a.batch, a.N, a.iters, a.reps, a.rounds))
    ms = {leg: [r["kernel_ms"] for r in recs[leg]] for leg in KD_LEGS}
    for leg in KD_LEGS:
        print("%-10s | %s | median %.4f | spread %.4f - %.4f | %d workgroups, %d bytes of LDS each | %s"
              % (leg, " ".join("%.4f" % v for v in ms[leg]), float(np.median(ms[leg])), min(ms[leg]), max(ms[leg]), recs[leg][0]["workgroups"],
                 recs[leg][0]["lds_bytes"], recs[leg][0]["kernel"]))
    on_d = recs["knots-D"][0]["kernel"].startswith("D ")
    below = all(n < o for n, o in zip(ms["knots-D"], ms["parent-A"]))
    print("knots-D on layout D: %s; below parent-A in every round: %s (largest %.4f against smallest %.4f, parent-A's spread %.4f; ratio of medians %.3f)"
          % ("yes" if on_d else "NO", "yes" if below else "NO", max(ms["knots-D"]), min(ms["parent-A"]), max(ms["parent-A"]) - min(ms["parent-A"]),
             float(np.median(ms["knots-D"])) / float(np.median(ms["parent-A"]))))
    med, floor = float(np.median(ms["knots-D"])), float(np.median(ms["const-D"]))
    waves = (a.batch + 3) // 4  # (16 lanes per instance: four instances per wavefront)
    print("distance to the floor: knots-D median %.4f against const-D median %.4f (ratio %.3f, +%.4f ms); the staging reads %d wavefronts x "
          "%d slots x 3 vectors x 512 B = %.1f MB per launch" % (med, floor, med / floor, med - floor, waves, a.N, waves * a.N * 3 * 512 / 1e6))


def device_copy(pkg, arrays):
    """Device copies of `arrays` through the HIP runtime the library itself uses, or None where that runtime cannot be found."""
    pkg.load_library()
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line and "/torch/" not in line})
    if not paths:
        return None
    hip = C.CDLL(paths[0])
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = []
    for h in arrays:
        p = C.c_void_p()
        if hip.hipMalloc(C.byref(p), h.nbytes) != 0 or hip.hipMemcpy(p, C.c_void_p(h.ctypes.data), h.nbytes, 1) != 0:
            return None
        out.append(p)
    return out


def child(pkg, a):
    """One process: one leg's kernel time; the per-inst leg also times the verbs, the shared leg also the default layout. One line."""
    s = make(pkg, a.child, a)
    s.solve_timed()  # warm-up: first launch, table builds
    out = dict(leg=a.child, kernel_ms=float(np.median([s.solve_timed() for _ in range(a.reps)])),
               kernel="%s %s" % (s.launch_info()["layout"], s.jit_info()))
    if a.child == "per-inst":
        prob = pkg.problems.quadrotor(a.N)
        L, dp = pkg.load_library(), pkg._lib.c_double_p
        host = [np.asfortranarray(np.repeat(m[..., None], a.batch, axis=-1)) for m in rows(prob, a.batch)]
        dev = device_copy(pkg, host)
        fresh = pkg.TinyMPC()
        fresh.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=a.batch, rho=prob.rho)
        wall, wall_dev = [], []
        for _ in range(1 + a.reps):
            t0 = time.perf_counter()
            rc = L.tinympc_set_linear_constraints_batch(fresh._h, host[0].ctypes.data_as(dp), host[1].ctypes.data_as(dp), 1,
                                                        host[2].ctypes.data_as(dp), host[3].ctypes.data_as(dp), 1, 0, a.batch)
            wall.append(1e3 * (time.perf_counter() - t0))
            assert rc == 0, pkg._lib.last_error()
        for _ in range(a.reps if dev else 0):
            t0 = time.perf_counter()
            rc = L.tinympc_set_linear_constraints_batch_device(fresh._h, dev[0], dev[1], 1, dev[2], dev[3], 1, 0, a.batch)
            wall_dev.append(1e3 * (time.perf_counter() - t0))
            assert rc == 0, pkg._lib.last_error()
        out.update(verb_host_ms=wall, verb_device_ms=wall_dev)
        fresh.reset()
    else:  # context: the same shared rows on the layout the handle picks by default
        s.reset()
        os.environ.pop("TINYMPC_LAYOUT", None)
        s = make(pkg, "shared-default", a)
        s.solve_timed()
        out.update(default_ms=float(np.median([s.solve_timed() for _ in range(a.reps)])),
                   default_kernel="%s %s" % (s.launch_info()["layout"], s.jit_info()))
    s.reset()
    print("LIN-CHILD " + json.dumps(out), flush=True)


def sweep(a):
    """Starts the children (it never opens the GPU itself) and prints the table."""
    recs = {leg: [] for leg in LEGS}
    for rnd in range(a.rounds):
        for leg in LEGS if rnd % 2 == 0 else LEGS[::-1]:
            env = dict(os.environ)
            env.pop("TINYMPC_LAYOUT", None)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--batch", str(a.batch), "--N", str(a.N),
                                "--iters", str(a.iters), "--reps", str(a.reps)], env=env, capture_output=True, text=True, timeout=300)
            line = [l for l in r.stdout.splitlines() if l.startswith("LIN-CHILD ")]
            if r.returncode != 0 or not line:
                raise SystemExit("round %d (%s) failed with %d:\n%s\n%s" % (rnd, leg, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            recs[leg].append(json.loads(line[0][len("LIN-CHILD "):]))
            print("# round %d %-9s %.4f ms" % (rnd, leg, recs[leg][-1]["kernel_ms"]), flush=True)
    print("per-instance linear rows: %d quadrotors N=%d x %d forced iterations, 1 state row + 1 input row; kernel ms (median of %d launches per "
          "round, %d rounds, a fresh process each, legs alternating)" % (a.batch, a.N, a.iters, a.reps, a.rounds))
    ms = {leg: [r["kernel_ms"] for r in recs[leg]] for leg in LEGS}
    for leg in LEGS:
        print("%-9s | %s | median %.4f | spread %.4f - %.4f | %s" % (leg, " ".join("%.4f" % v for v in ms[leg]), float(np.median(ms[leg])),
                                                                    min(ms[leg]), max(ms[leg]), recs[leg][0]["kernel"]))
    med, lo, hi = float(np.median(ms["per-inst"])), min(ms["shared-A"]), max(ms["shared-A"])
    print("per-inst median inside shared-A's spread: %s (%.4f against %.4f - %.4f; ratio of medians %.3f)"
          % ("yes" if lo <= med <= hi else "NO", med, lo, hi, med / float(np.median(ms["shared-A"]))))
    d = [r["default_ms"] for r in recs["shared-A"]]
    print("context, shared rows on the default layout: %s | median %.4f | %s" % (" ".join("%.4f" % v for v in d), float(np.median(d)),
                                                                                 recs["shared-A"][0]["default_kernel"]))
    for key, name in (("verb_host_ms", "set_linear_constraints_batch"), ("verb_device_ms", "set_linear_constraints_batch_device")):
        first = [r[key][0] for r in recs["per-inst"] if r[key]]
        rest = [v for r in recs["per-inst"] for v in (r[key][1:] if key == "verb_host_ms" else r[key])]
        if not rest:
            print("%-36s not measured (no device memory could be filled)" % name)
            continue
        print("%-36s %d instances, wall ms: %s median %.3f (min %.3f, max %.3f)"
              % (name, a.batch, ("first call %s | repeats" % " ".join("%.3f" % v for v in first)) if key == "verb_host_ms" else "calls",
                 float(np.median(rest)), min(rest), max(rest)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--N", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--d", action="store_true")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--knots", action="store_true")
    ap.add_argument("--alt-lib", default="")
    a = ap.parse_args()
    if not a.child:
        return sweep_kd(a) if a.knots and a.d else sweep_k(a) if a.knots else sweep_d(a) if a.d else sweep(a)
    import __graft_entry__ as ge
    (child_kd if a.knots and a.d else child_k if a.knots else child_d if a.d else child)(ge.load_package(), a)


if __name__ == "__main__":
    main()
