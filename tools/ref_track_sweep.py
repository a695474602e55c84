"""Reference tracks at bench size: what a closed-loop tick costs when every instance follows its own trajectory.

`--batch` quadrotors at N = `--N`, every instance with its own track of `--T` knots, through a warm-started closed loop of `--ticks`
mpc_step ticks (x <- A x + B u on the host between ticks; the tick's wall time is what is measured). Three legs on the same ticks:
  a   a window per tick through set_x_ref_batch + set_u_ref_batch from host memory (nx N batch 8 B over PCIe per tick)
  b   the same verbs' _device forms, the windows cut out of a device copy of the tracks per tick (one strided device-to-device copy
      per half through the HIP runtime the library itself uses): the best a caller can do without tracks
  c   tracks uploaded once (set_x_ref_track_batch / set_u_ref_track_batch) with auto-advance: the tick uploads x0 and nothing else
  c0  as c with auto-advance 0: the same window every tick, no rebuild of the rows -- c minus c0 is the per-tick rebuild
Legs a and b run on the library of the PARENT commit at --parent-lib (built from a checkout of the parent), c and c0 on this tree's.
Every measurement is a fresh process -- the two libraries alternate, `--rounds` times each -- so the legs share one call's noise. The
first controls of every tick of leg c must equal leg a's bit for bit (asserted here, for every round), and leg c must be faster than
leg a in every round (asserted too). The tolerances are 0, so every tick of every leg runs exactly `--iters` iterations: the legs
differ in how the references arrive and in nothing else. Prints a table.
    python tools/ref_track_sweep.py --parent-lib /path/to/parent/libtinympc_hip.so [--batch 8192] [--N 50] [--T 200] [--ticks 40]

Layout D (--d --parent-lib PATH): leg c alone, on a handle that called prepare(), with
  cA  on the library of the parent commit at PATH (a parent that has the track verbs): layout A, where tracks ran before layout D had a
      form for them -- the yardstick
  cD  on this tree's library: layout D's per-instance trajectory form
Every measurement is a fresh process; the two libraries alternate, `--rounds` times each. The first controls of every tick of cD must
lie within 1e-9 of cA's (asserted; another kernel, another order of operations), and the bar is cD below cA in EVERY round (reported,
and the exit status says it).
    python tools/ref_track_sweep.py --d --parent-lib /path/to/parent/libtinympc_hip.so"""
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

WARMUP = 3  # ticks before the counted ones (first launch, table builds, staging buffers)


class DeviceTracks:
    """Leg b's caller: the tracks in device memory, (batch, T, rows) row-major -- the verbs' layout --, and the window of a tick cut out of
    them on the device: instance b's window is the contiguous run of cols * rows doubles at knot k of its track."""

    def __init__(self, pkg, track):
        import ctypes as C
        pkg.load_library()
        with open("/proc/self/maps") as f:
            paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line and "/torch/" not in line})
        self.C, self.hip = C, C.CDLL(paths[0])
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
        self.rows, self.T, self.batch = track.shape
        h = np.ascontiguousarray(track.T)
        self.src, self.win = C.c_void_p(), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.src), h.nbytes) == 0 and self.hip.hipMalloc(C.byref(self.win), h.nbytes) == 0
        assert self.hip.hipMemcpy(self.src, C.c_void_p(h.ctypes.data), h.nbytes, 1) == 0  # hipMemcpyHostToDevice

    def window(self, k, cols):
        """-> device pointer of the (batch, cols, rows) window at knot k (k + cols <= T); complete when the call returns."""
        assert k + cols <= self.T
        w = 8 * self.rows * cols
        src = self.C.c_void_p(self.src.value + 8 * self.rows * k)
        assert self.hip.hipMemcpy2D(self.win, w, src, 8 * self.rows * self.T, w, self.batch, 3) == 0  # hipMemcpyDeviceToDevice
        assert self.hip.hipDeviceSynchronize() == 0
        return self.win


def tracks(prob, batch, T):
    """nx x T x batch and nu x T x batch: a figure-eight per instance, its own phase and size; small input references."""
    rng = np.random.default_rng(5)
    phase, size = rng.uniform(0.0, 2.0 * np.pi, batch), rng.uniform(0.2, 0.5, batch)
    t = 2.0 * np.pi / 150.0 * np.arange(T)[:, None] + phase[None, :]
    X = np.zeros((prob.nx, T, batch), order="F")
    X[0], X[1] = size * np.sin(t), size * np.sin(t) * np.cos(t)
    U = np.asfortranarray(0.01 * np.cos(t)[None, :, :] * np.ones((prob.nu, 1, 1)))
    return X, U


def window(track, k, cols):
    return np.asfortranarray(track[:, np.minimum(k + np.arange(cols), track.shape[1] - 1), :])


def run_leg(pkg, leg, a, prepare=False):
    """One closed loop of WARMUP + a.ticks ticks -> (per-tick wall us of the counted ticks, first controls of every tick, iterations)."""
    P = pkg.problems
    prob = P.quadrotor(a.N)
    N, batch = prob.N, a.batch
    X, U = tracks(prob, batch, a.T)
    s = pkg.TinyMPC()
    s.setup(prob.A, prob.B, prob.Q, prob.R, N, batch=batch, rho=prob.rho, max_iter=a.iters, abs_pri_tol=0.0, abs_dua_tol=0.0)
    s.set_bound_constraints(prob.x_min, prob.x_max, prob.u_min, prob.u_max)
    if prepare:
        s.prepare()
    if leg == "b":
        dX, dU = DeviceTracks(pkg, X), DeviceTracks(pkg, U)
        L = pkg.load_library()
    if leg in ("c", "c0"):
        s.set_x_ref_track_batch(X)
        s.set_u_ref_track_batch(U)
        s.set_ref_auto_advance(1 if leg == "c" else 0)
    x = np.asfortranarray(X[:, 0, :] + 0.05 * P.quadrotor_batch_x0(batch))
    wall, us, iters = [], [], []
    for k in range(WARMUP + a.ticks):
        if leg == "a":
            wx, wu = window(X, k, N), window(U, k, N - 1)  # (cut on the host outside the timed region: only the verbs are timed)
        t0 = time.perf_counter()
        if leg == "a":
            s.set_x_ref_batch(wx)
            s.set_u_ref_batch(wu)
        elif leg == "b":
            pkg._lib.check(L.tinympc_set_x_ref_batch_device(s._h, dX.window(k, N), prob.nx, N, 0, batch))
            pkg._lib.check(L.tinympc_set_u_ref_batch_device(s._h, dU.window(k, N - 1), prob.nu, N - 1, 0, batch))
        u = s.mpc_step(x)
        wall.append(1e6 * (time.perf_counter() - t0))
        us.append(u)
        iters.append(float(s.get_stats_batch()["iter"].mean()))
        x = np.asfortranarray(prob.A @ x + prob.B @ u)
    info = "%s %s" % (s.launch_info()["layout"], s.jit_info())
    s.reset()
    return wall[WARMUP:], np.stack(us), float(np.mean(iters[WARMUP:])), info


def child(pkg, a):
    """One process: the legs of whatever library it loaded; one JSON line, the first controls of legs a / c in a.dump."""
    has_tracks = hasattr(pkg.load_library(), "tinympc_set_x_ref_track_batch")
    out = dict(library="this" if has_tracks else "parent", tick_us={}, iters={}, kernel={})
    legs = ["c", "c0"] if has_tracks else ["a", "b"]
    for leg in legs:
        wall, us, iters, info = run_leg(pkg, leg, a)
        out["tick_us"][leg], out["iters"][leg], out["kernel"][leg] = float(np.median(wall)), iters, info
        if leg in ("a", "b", "c") and a.dump:
            np.save(os.path.join(a.dump, "u_%s.npy" % leg), us)
    print("TRACK-CHILD " + json.dumps(out), flush=True)


def child_d(pkg, a):
    """One process of the --d sweep: leg c after prepare() on whatever library it loaded; one JSON line, the first controls in a.dump."""
    wall, us, iters, info = run_leg(pkg, "c", a, prepare=True)
    np.save(os.path.join(a.dump, "u_%s.npy" % a.leg), us)
    print("TRACK-CHILD " + json.dumps(dict(leg=a.leg, tick_us=float(np.median(wall)), iters=iters, kernel=info)), flush=True)


def sweep_d(a):
    """The parent of the --d sweep: starts the children (it never opens the GPU itself), compares their first controls, prints the table."""
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("needs --parent-lib: libtinympc_hip.so built from the parent commit")
    rows, worst = {"cA": [], "cD": []}, 0.0
    with tempfile.TemporaryDirectory() as tmp:
        for rnd in range(a.rounds):
            for leg in ("cD", "cA") if rnd % 2 == 0 else ("cA", "cD"):
                env = dict(os.environ)
                env.pop("TINYMPC_HIP_LIBRARY", None)
                if leg == "cA":
                    env["TINYMPC_HIP_LIBRARY"] = os.path.abspath(a.parent_lib)
                cmd = [sys.executable, os.path.abspath(__file__), "--d", "--child", "--leg", leg, "--dump", tmp] + \
                      [w for k in ("batch", "N", "T", "ticks", "iters") for w in ("--" + k, str(getattr(a, k)))]
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=500)
                line = [l for l in r.stdout.splitlines() if l.startswith("TRACK-CHILD ")]
                if r.returncode != 0 or not line:
                    raise SystemExit("round %d (%s) failed with %d:\n%s\n%s" % (rnd, leg, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
                rows[leg].append(json.loads(line[0][len("TRACK-CHILD "):]))
                print("# round %d %-3s %.1f us" % (rnd, leg, rows[leg][-1]["tick_us"]), flush=True)
            ua, ud = np.load(os.path.join(tmp, "u_cA.npy")), np.load(os.path.join(tmp, "u_cD.npy"))
            worst = max(worst, float(np.max(np.abs(ud - ua)) / np.max(np.abs(ua))))
    print("reference tracks on layout D, %d quadrotors N=%d, T=%d, every handle after prepare(), closed loop of %d warm-started mpc_step ticks "
          "(%d iterations each), wall us per tick (median of the ticks of a round; %d rounds, a fresh process each, the two libraries alternating)"
          % (a.batch, a.N, a.T, a.ticks, a.iters, a.rounds))
    for leg, name in (("cA", "cA tracks, the parent's library"), ("cD", "cD tracks, this tree")):
        v = [r["tick_us"] for r in rows[leg]]
        print("%-32s | %-36s | median %9.1f | spread %8.1f - %8.1f | %.2f iterations / tick | %s"
              % (name, " ".join("%.1f" % x for x in v), float(np.median(v)), min(v), max(v), rows[leg][0]["iters"], rows[leg][0]["kernel"]))
    below = all(d["tick_us"] < p_["tick_us"] for d, p_ in zip(rows["cD"], rows["cA"]))
    print("cD on layout D: %s; first controls within %.1e of cA's (relative to the largest control); cD below cA in every round: %s (ratio of medians %.3f)"
          % ("yes" if rows["cD"][0]["kernel"].startswith("D ") else "NO", worst, "yes" if below else "NO",
             float(np.median([r["tick_us"] for r in rows["cD"]])) / float(np.median([r["tick_us"] for r in rows["cA"]]))))
    assert worst < 1e-9, "the first controls on layout D differ from layout A's"
    if not below:
        raise SystemExit(1)


def sweep(a):
    """The parent: starts the children (it never opens the GPU itself), compares their first controls, prints the table."""
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("needs --parent-lib: libtinympc_hip.so built from the parent commit")
    rows = {"this": [], "parent": []}
    equal = []
    with tempfile.TemporaryDirectory() as tmp:
        for rnd in range(a.rounds):
            for lib in ("this", "parent") if rnd % 2 == 0 else ("parent", "this"):
                env = dict(os.environ)
                env.pop("TINYMPC_HIP_LIBRARY", None)
                if lib == "parent":
                    env["TINYMPC_HIP_LIBRARY"] = os.path.abspath(a.parent_lib)
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--dump", tmp] + \
                      [w for k in ("batch", "N", "T", "ticks", "iters") for w in ("--" + k, str(getattr(a, k)))]
                r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=500)
                line = [l for l in r.stdout.splitlines() if l.startswith("TRACK-CHILD ")]
                if r.returncode != 0 or not line:
                    raise SystemExit("round %d (%s) failed with %d:\n%s\n%s" % (rnd, lib, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
                rec = json.loads(line[0][len("TRACK-CHILD "):])
                assert rec["library"] == lib, rec
                rows[lib].append(rec)
                print("# round %d %-6s %s" % (rnd, lib, json.dumps(rec["tick_us"])), flush=True)
            ua, uc = np.load(os.path.join(tmp, "u_a.npy")), np.load(os.path.join(tmp, "u_c.npy"))
            same = [bool(np.array_equal(ua[k], uc[k])) for k in range(ua.shape[0])]
            assert np.array_equal(np.load(os.path.join(tmp, "u_b.npy")), ua), "leg b's windows are not leg a's"
            equal.append(all(same))
            print("# round %d: first controls of leg c equal leg a's bit for bit on %d of %d ticks" % (rnd, sum(same), len(same)), flush=True)
    print("reference tracks, %d quadrotors N=%d, T=%d, closed loop of %d warm-started mpc_step ticks (%d iterations each), wall us per tick "
          "(median of the ticks of a round; %d rounds, a fresh process each, the two libraries alternating)" % (a.batch, a.N, a.T, a.ticks, a.iters, a.rounds))
    legs = [("a", "parent", "a  windows from host memory (parent)"), ("b", "parent", "b  windows cut on the device (parent)"),
            ("c", "this", "c  tracks, auto-advance 1 (this tree)"), ("c0", "this", "c0 tracks, auto-advance 0 (this tree)")]
    med = {}
    print("%-42s | %-36s | %-9s | %-19s | %s" % ("leg", "rounds", "median", "spread", "iterations / tick"))
    for leg, lib, name in legs:
        v = [r["tick_us"][leg] for r in rows[lib] if leg in r["tick_us"]]
        med[leg] = float(np.median(v))
        print("%-42s | %-36s | %9.1f | %8.1f - %8.1f | %.2f" % (name, " ".join("%.1f" % x for x in v), med[leg], min(v), max(v), rows[lib][0]["iters"][leg]))
    for leg, lib, _ in legs:
        if leg in rows[lib][0]["kernel"]:
            print("kernel %-2s %s" % (leg, rows[lib][0]["kernel"][leg]))
    print("per-tick rebuild of the rows (c - c0, medians): %.1f us = %.1f %% of leg c's tick" % (med["c"] - med["c0"], 100.0 * (med["c"] - med["c0"]) / med["c"]))
    print("c against a: %.2fx; c against b: %.2fx" % (med["a"] / med["c"], med["b"] / med["c"]))
    faster = [rc["tick_us"]["c"] < ra["tick_us"]["a"] for rc, ra in zip(rows["this"], rows["parent"])]
    print("leg c bit-identical to leg a in every round: %s; leg c faster than leg a in every round: %s" % ("yes" if all(equal) else "NO", "yes" if all(faster) else "NO"))
    assert all(equal), "the first controls of the tracks differ from the windows sent by hand"
    assert all(faster), "tracks are not faster than windows from host memory: look at the build path of the rows"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--dump", default="", help=argparse.SUPPRESS)
    ap.add_argument("--d", action="store_true")
    ap.add_argument("--leg", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not a.child:
        return sweep_d(a) if a.d else sweep(a)
    import __graft_entry__ as ge
    (child_d if a.d else child)(ge.load_package(), a)


if __name__ == "__main__":
    main()
