"""Per-instance models at bench size.

Solve (default): kernel milliseconds (HIP events, tinympc_solve_timed) of the same forced-iteration solve of `--batch` quadrotors with
  shared-A   the shared model, one constant box, on layout A (TINYMPC_LAYOUT=A): k_admm_solve
  ibnd       the shared model with bounds per knot per instance (set_bound_constraints_batch): layout A's k_admm_solve_ibnd
  models     the same references and bounds, and a model per instance (set_model_batch): layout A's k_admm_solve_imod
The variants run interleaved, `--rounds` times; the median of `--reps` launches per round is reported, one JSON line per variant.
    python tools/instance_models_sweep.py [--batch 8192] [--N 50] [--iters 200] [--rounds 4] [--reps 5] [--only ibnd,models]

Layout D (--d): the same solve with one constant box per instance (what layout D's per-instance forms carry) on
  models-D   a model per instance after prepare(): layout D's model form (every wavefront's four operator blocks in its LDS region)
  models-A   the same handle without prepare(): layout A's k_admm_solve_imod, the path the mode takes by default
  goal-D     the shared model: layout D's goal kernel (k_admm_solve_d_gbnd, two wavefronts per SIMD) -- the floor
interleaved and reported in the same way.
    python tools/instance_models_sweep.py --d [--N 50 | --N 20]

Per-instance rho (--rho --parent-lib PATH): the --d handle kinds (layout D N=50, layout D N=20, layout A N=50; a model per instance,
one constant box per instance) with rho_b spread log-uniformly over [0.5, 4] x rho (set_rho_batch), against the SAME handles without
the verb on the library of the parent commit at PATH (built from a checkout of the parent). Every measurement is a fresh process --
this tree's library and the parent's alternate, `--rounds` times each -- so the two are interleaved in one call and share its noise;
the bar: the median of this tree's rounds lies inside the spread of the parent's rounds. Also the wall time of set_rho_batch for
`--batch` values beside set_model_batch for as many models (the precompute is the same launch). Prints a table.
    python tools/instance_models_sweep.py --rho --parent-lib /path/to/parent/libtinympc_hip.so

Setup (--setup): wall milliseconds of tinympc_set_model_batch for `--batch` quadrotor and cartpole models -- the first call (which
allocates the per-instance stores and fills them from the shared model), then `--reps` further calls, from host memory and, where
device memory can be filled, from device memory -- beside the wall time of one single-instance tinympc_setup of the same problem.

Launch count (--probe COUNT): one handle of `--batch` instances, set_model_batch for COUNT of them, one solve; meant to run under
    rocprofv3 --kernel-trace --stats -- python tools/instance_models_sweep.py --probe 64
(the kernels submitted must not depend on COUNT)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = ["shared-A", "ibnd", "models"]
D_VARIANTS = ["models-D", "models-A", "goal-D"]


def models(prob, batch, seed=0):
    rng = np.random.default_rng(seed)
    nx, nu = prob.nx, prob.nu
    A = np.asfortranarray(prob.A[:, :, None] + 1e-2 * rng.uniform(-1.0, 1.0, (nx, nx, batch)))
    B = np.asfortranarray(prob.B[:, :, None] * rng.uniform(0.85, 1.15, (nx, nu, batch)))
    Q, R = np.zeros((nx, nx, batch), order="F"), np.zeros((nu, nu, batch), order="F")
    Q[np.arange(nx), np.arange(nx), :] = np.diag(prob.Q)[:, None] * rng.uniform(0.85, 1.15, (nx, batch))
    R[np.arange(nu), np.arange(nu), :] = np.diag(prob.R)[:, None] * rng.uniform(0.85, 1.15, (nu, batch))
    f = np.asfortranarray(1e-3 * rng.standard_normal((nx, batch)))
    return A, B, Q, R, f


def make(pkg, variant, batch, N, iters):
    P = pkg.problems
    prob = P.quadrotor(N)
    nx, nu = prob.nx, prob.nu
    rng = np.random.default_rng(0)
    if variant == "shared-A":
        os.environ["TINYMPC_LAYOUT"] = "A"
    try:
        s = pkg.TinyMPC()
        s.setup(prob.A, prob.B, prob.Q, prob.R, N, batch=batch, rho=prob.rho, abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=iters)
    finally:
        os.environ.pop("TINYMPC_LAYOUT", None)
    wave = 1.0 - 0.3 * np.abs(np.sin(0.3 * np.arange(N)))  # per-knot shrink factor
    if variant == "shared-A":
        s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    elif variant in D_VARIANTS:  # (tools/instance_bounds_sweep.py's `box` variant: one constant box per instance)
        fx, fu = rng.uniform(0.5, 1.0, (nx, batch)), rng.uniform(0.3, 1.0, (nu, batch))
        s.set_bound_constraints_batch(prob.x_min[:, None] * fx, prob.x_max[:, None] * fx, prob.u_min[:, None] * fu, prob.u_max[:, None] * fu)
    else:  # (tools/instance_bounds_sweep.py's `knot` variant)
        fx, fu = rng.uniform(0.5, 1.0, (nx, batch)), rng.uniform(0.3, 1.0, (nu, batch))
        xl, xh, ul, uh = prob.x_min[:, None] * fx, prob.x_max[:, None] * fx, prob.u_min[:, None] * fu, prob.u_max[:, None] * fu
        wx, wu = wave[None, :, None], wave[None, :N - 1, None]
        s.set_bound_constraints_batch(xl[:, None, :] * wx, xh[:, None, :] * wx, ul[:, None, :] * wu, uh[:, None, :] * wu)
    if variant in ("models", "models-D", "models-A"):
        A, B, Q, R, f = models(prob, batch)
        s.set_model_batch(A, B, Q, R, fdyn=f)
    if variant == "models-D":
        s.prepare()
    s.set_x_ref(np.tile(0.3 * rng.standard_normal((nx, 1)), (1, N)))
    s.set_x0_batch(P.quadrotor_batch_x0(batch))
    return s


def solve_sweep(pkg, a):
    names = [v for v in (D_VARIANTS if a.d else VARIANTS) if not a.only or v in a.only.split(",")]
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


RHO_KINDS = [("D N=50", 50, True), ("D N=20", 20, True), ("A N=50", 50, False)]  # (name, horizon, prepare()?)


def rho_child(pkg, a):
    """One process of the --rho leg: the three handle kinds on whatever library this process loaded; one JSON line."""
    P, L = pkg.problems, pkg.load_library()
    has_verb = hasattr(L, "tinympc_set_rho_batch")
    out = dict(library="this" if has_verb else "parent", kernel_ms={}, kernel={})
    for name, N, prepare in RHO_KINDS:
        s = make(pkg, "models-D" if prepare else "models-A", a.batch, N, a.iters)
        if has_verb:
            f = np.exp(np.random.default_rng(11).uniform(np.log(0.5), np.log(4.0), a.batch))
            s.set_rho_batch(P.quadrotor(N).rho * f)
        s.solve_timed()  # warm-up: first launch, table builds
        out["kernel_ms"][name] = float(np.median([s.solve_timed() for _ in range(a.reps)]))
        out["kernel"][name] = "%s %s" % (s.launch_info()["layout"], s.jit_info())
        s.reset()
    if has_verb:  # the verbs' wall time, first call (allocates and fills the stores) and repeats
        prob = P.quadrotor(50)
        A, B, Q, R, f = models(prob, a.batch)
        rhos = prob.rho * np.exp(np.random.default_rng(11).uniform(np.log(0.5), np.log(4.0), a.batch))
        for key, call in (("set_rho_batch_ms", lambda s: s.set_rho_batch(rhos)), ("set_model_batch_ms", lambda s: s.set_model_batch(A, B, Q, R, fdyn=f))):
            s = pkg.TinyMPC()
            s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=a.batch, rho=prob.rho)
            wall = []
            for _ in range(1 + a.reps):
                t0 = time.perf_counter()
                call(s)
                wall.append(1e3 * (time.perf_counter() - t0))
            out[key] = wall
            s.reset()
    print("RHO-CHILD " + json.dumps(out), flush=True)


def rho_sweep(a):
    """The parent of the --rho leg: starts the children (it never opens the GPU itself) and prints the table."""
    import subprocess
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--rho needs --parent-lib: libtinympc_hip.so built from the parent commit")
    rows = {"this": [], "parent": []}
    for rnd in range(a.rounds):
        for lib in ("this", "parent") if rnd % 2 == 0 else ("parent", "this"):
            env = dict(os.environ)
            env.pop("TINYMPC_HIP_LIBRARY", None)
            if lib == "parent":
                env["TINYMPC_HIP_LIBRARY"] = os.path.abspath(a.parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rho-child", "--batch", str(a.batch), "--iters", str(a.iters), "--reps", str(a.reps)],
                               env=env, capture_output=True, text=True, timeout=400)
            line = [l for l in r.stdout.splitlines() if l.startswith("RHO-CHILD ")]
            if r.returncode != 0 or not line:
                raise SystemExit("round %d (%s) failed with %d:\n%s\n%s" % (rnd, lib, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
            rec = json.loads(line[0][len("RHO-CHILD "):])
            assert rec["library"] == lib, rec
            rows[lib].append(rec)
            print("# round %d %-6s %s" % (rnd, lib, json.dumps(rec["kernel_ms"])), flush=True)
    print("per-instance rho, %d quadrotors x %d forced iterations, kernel ms (median of %d launches per round, %d rounds, a fresh process each)"
          % (a.batch, a.iters, a.reps, a.rounds))
    print("%-8s | %-34s | %-34s | %-9s | %-17s | %s" % ("handle", "parent (set_model_batch)", "this tree (+ set_rho_batch)", "median", "parent spread", "inside"))
    for name, _, _ in RHO_KINDS:
        par = [r["kernel_ms"][name] for r in rows["parent"]]
        new = [r["kernel_ms"][name] for r in rows["this"]]
        med = float(np.median(new))
        print("%-8s | %-34s | %-34s | %9.4f | %7.4f - %7.4f | %s" % (name, " ".join("%.4f" % v for v in par), " ".join("%.4f" % v for v in new), med,
                                                                    min(par), max(par), "yes" if min(par) <= med <= max(par) else "NO"))
    for name, _, _ in RHO_KINDS:
        print("kernel %-8s this: %s | parent: %s" % (name, rows["this"][0]["kernel"][name], rows["parent"][0]["kernel"][name]))
    for key in ("set_rho_batch_ms", "set_model_batch_ms"):
        first = [r[key][0] for r in rows["this"]]
        rest = [v for r in rows["this"] for v in r[key][1:]]
        print("%-18s %d quadrotor N=50 instances, wall ms: first call %s | repeats median %.3f (min %.3f, max %.3f)"
              % (key[:-3], a.batch, " ".join("%.3f" % v for v in first), float(np.median(rest)), min(rest), max(rest)))


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


def setup_sweep(pkg, a):
    P, L = pkg.problems, pkg.load_library()
    dp = pkg._lib.c_double_p
    for name, prob in (("quadrotor", P.quadrotor(50)), ("cartpole", P.cartpole(20, True))):
        arrays = models(prob, a.batch)
        A, B, Q, R, f = arrays
        single = []
        for _ in range(20):  # one single-instance setup of the same problem (wall, warm pools after the first)
            t0 = time.perf_counter()
            one = pkg.TinyMPC()
            one.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, rho=prob.rho)
            single.append(1e3 * (time.perf_counter() - t0))
            steps = one.get_cache()["riccati_iters"]
            one.reset()
        s = pkg.TinyMPC()
        s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=a.batch, rho=prob.rho)
        host = [x.ctypes.data_as(dp) for x in (A, B, f, Q, R)]
        wall = []
        for _ in range(1 + a.reps):
            t0 = time.perf_counter()
            rc = L.tinympc_set_model_batch(s._h, *host, 0, a.batch)
            wall.append(1e3 * (time.perf_counter() - t0))
            assert rc == 0, pkg._lib.last_error()
        dev = device_copy(pkg, (A, B, f, Q, R))
        wall_dev = []
        for _ in range(a.reps if dev else 0):
            t0 = time.perf_counter()
            rc = L.tinympc_set_model_batch_device(s._h, *dev, 0, a.batch)
            wall_dev.append(1e3 * (time.perf_counter() - t0))
            assert rc == 0, pkg._lib.last_error()
        its = s.get_cache_batch()["riccati_iters"]
        print(json.dumps(dict(problem=name, batch=a.batch, riccati_steps_shared=int(steps), riccati_steps_min=int(its.min()), riccati_steps_max=int(its.max()),
                              first_call_ms=wall[0], host_ms=wall[1:], device_ms=wall_dev, single_setup_ms_median=float(np.median(single[1:])),
                              single_setup_ms_min=float(np.min(single)), single_setup_times_batch_ms=float(np.median(single[1:])) * a.batch)), flush=True)
        s.reset()


def probe(pkg, a):
    P = pkg.problems
    prob = P.quadrotor(a.N)
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, prob.N, batch=a.batch, rho=prob.rho, abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=10)
    A, B, Q, R, f = models(prob, a.probe)
    s.set_x0_batch(P.quadrotor_batch_x0(a.batch))
    s.set_model_batch(A, B, Q, R, fdyn=f)
    s.solve()
    print(json.dumps(dict(probe=a.probe, batch=a.batch, layout=s.launch_info()["layout"], kernel=s.jit_info())), flush=True)
    s.reset()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--d", action="store_true")
    ap.add_argument("--setup", action="store_true")
    ap.add_argument("--probe", type=int, default=0)
    ap.add_argument("--rho", action="store_true")
    ap.add_argument("--rho-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--parent-lib", default="")
    a = ap.parse_args()
    if a.rho:
        return rho_sweep(a)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    if a.rho_child:
        rho_child(pkg, a)
    elif a.probe:
        probe(pkg, a)
    elif a.setup:
        setup_sweep(pkg, a)
    else:
        solve_sweep(pkg, a)


if __name__ == "__main__":
    main()
