"""How a layout D launch is cut into runs of lean rounds: a plain Python restatement of the loop behind the `iteration` lambda of
tinympc_solve_d.hip (TINY_LEAN_HOIST), the grid of settings that covers every such cut, and the oracle's side of the grid. No GPU here:
tests/test_lean_run_structure_cpu.py checks this module against itself and against the oracle, tests/test_lean_run_structure_gpu.py runs
the grid on every lean build. A change to the kernel's loop changes `lean_runs` too.

The kernel's loop, with `it` the number of iterations done so far:

    nres     = the next iteration, counted from 1, whose residuals something reads (need_res at the top of tinympc_solve_d.hip)
    lean_end = min(nres - 1, max_iter)
    it < lean_end:   control once, then a run of lean_end - it lean rounds (the last one in mode 4 stores every d again)
    it == max_iter:  the final round (write-back only), the launch is over
    else:            the iteration with residuals, number it + 1 = nres

A run that ends at max_iter is a TAIL: the final round follows it, not an iteration with residuals. (A wavefront whose instances have all
converged leaves earlier, at the next run's control block or at the next iteration with residuals; `lean_runs` is the cut of a wavefront
that stays to the end.)"""
from __future__ import annotations

import numpy as np

# (the problem and the initial states are the trim test's)
from test_layout_d_lean_trim_gpu import CONVERGING_TOL, _goals, _problem, _x0s

PARK_MIN_RUN = 6  # (tinympc_plan.hip)
TOL = 0.1  # the quadrotor's converging tolerance: see test_layout_d_lean_park_gpu.py and test_lean_run_structure_cpu.py
SHAPE = "quadrotor50"  # the one shape with LDS slots, hence with park kernels
TOLS = {SHAPE: TOL, "cartpole20": CONVERGING_TOL["cartpole20"], "cartpole10": CONVERGING_TOL["cartpole10"]}  # (cartpoles: the trim test's)
WARM = 0.9  # the warm solve of a cell starts at WARM * x0


def reachable(pri_tol, dua_tol):
    return pri_tol > 0.0 and dua_tol > 0.0


def need_res(it1, max_iter, ct, pri_tol, dua_tol):
    """need_res(it1) = check(it1) && (reachable || it1 + check_termination > max_iter), as the top of tinympc_solve_d.hip states it."""
    check = ct > 0 and it1 % ct == 0
    return check and (reachable(pri_tol, dua_tol) or it1 + ct > max_iter)


def lean_runs(max_iter, ct, pri_tol, dua_tol):
    """(segments, tail): the launch's segments in order -- ("run", start, length): `length` lean rounds behind `start` finished iterations
    (iterations start + 1 ... start + length, counted from 1), ("res", it): iteration `it`, counted from 1, with residuals -- and whether the
    last run is a tail."""
    segments = []
    reach = reachable(pri_tol, dua_tol)
    last_check = (max_iter // ct) * ct if ct > 0 else 0
    it = 0
    while max_iter > 0:
        nres = max_iter + 1
        if ct > 0 and reach:
            nres = (it // ct + 1) * ct
        elif last_check > it:
            nres = last_check
        lean_end = min(nres - 1, max_iter)
        if it < lean_end:
            segments.append(("run", it, lean_end - it))
            it = lean_end
        if it >= max_iter:  # the final round
            break
        segments.append(("res", it + 1))
        it += 1
    tail = bool(segments) and segments[-1][0] == "run"
    return segments, tail


def runs_of(segments):
    return [s for s in segments if s[0] == "run"]


def first_run(max_iter, ct, pri_tol, dua_tol):
    """Rounds of the launch's first run (0: the launch starts with an iteration with residuals, or has no iteration at all)."""
    segments, _ = lean_runs(max_iter, ct, pri_tol, dua_tol)
    return segments[0][2] if segments and segments[0][0] == "run" else 0


def lean_applies(max_iter, ct, pri_tol, dua_tol):
    """tinympc_plan.hip: lean_applies for a compiled-in 16-lane box-path handle without slot refill and with TINYMPC_LEAN unset."""
    return max_iter > 0 and (ct != 1 or not reachable(pri_tol, dua_tol))


# build -> (environment, the lean words of jit_info where a lean launch has every variant the build allows)
BUILDS = {
    "plain": ({"TINYMPC_LEAN": "0"}, ()),
    "lean": ({"TINYMPC_LEAN_START": "0"}, ("lean",)),
    "start": ({"TINYMPC_LEAN_TRIM": "0"}, ("lean", "lds-start")),
    "trim": ({"TINYMPC_LEAN_SHARE": "0"}, ("lean", "lds-start", "trim")),
    "share": ({"TINYMPC_LEAN_PARK": "0"}, ("lean", "lds-start", "trim", "share")),
    "park": ({}, ("lean", "lds-start", "trim", "share", "park")),
}
SWITCHES = ("TINYMPC_LEAN", "TINYMPC_LEAN_START", "TINYMPC_LEAN_TRIM", "TINYMPC_LEAN_SHARE", "TINYMPC_LEAN_PARK")
LEAN_WORDS = BUILDS["park"][1]


def lean_words(build, shape, max_iter, ct, pri_tol, dua_tol):
    """The exact set of lean words jit_info has behind a solve of this build and setting."""
    if not lean_applies(max_iter, ct, pri_tol, dua_tol):
        return ()
    park = shape == SHAPE and first_run(max_iter, ct, pri_tol, dua_tol) >= PARK_MIN_RUN
    return tuple(w for w in BUILDS[build][1] if w != "park" or park)


# ---- the grid: (max_iter, check_termination) cells, each crossed with the four tolerance pairs
CTS = (0, 1, 2, 3, 7, 8)
GRID = [(m, ct) for ct in (2, 3, 7, 8) for m in range(3 * ct + 3)] + [(m, ct) for ct in (0, 1) for m in (0, 1, 2, 5, 6, 7)]
PAIRS = ("both", "none", "pri", "dua")  # which tolerance is positive


def pair_tols(pair, tol=TOL):
    return {"both": (tol, tol), "none": (0.0, 0.0), "pri": (tol, 0.0), "dua": (0.0, tol)}[pair]


def cells(ct=None):
    return [c for c in GRID if ct is None or c[1] == ct]


BATCHES = {9: CTS, 1: (7,), 5: (7,)}  # batch -> the check intervals it runs on (9: two full wavefronts and a third with one live row)

# ---- the handover sequence: (max_iter, check_termination, tolerance, x0 scale), one handle, no reset between the steps
SEQUENCE = [(40, 0, 0.0, 1.0), (5, 0, 0.0, 0.9), (29, 7, 0.1, 1.3), (7, 1, 0.1, 0.7), (8, 7, 0.1, 1.5), (3, 0, 0.0, 1.0), (30, 7, 0.1, 2.0),
            (0, 0, 0.0, 1.0), (23, 8, 0.1, 0.5), (13, 7, 0.1, 1.8)]


def classes(max_iter, ct, pri_tol, dua_tol):
    """The classes of cuts (test_lean_run_structure_cpu.py: CLASSES) that one cell with one tolerance pair belongs to."""
    segments, tail = lean_runs(max_iter, ct, pri_tol, dua_tol)
    runs = runs_of(segments)
    n_res = len(segments) - len(runs)
    reach = reachable(pri_tol, dua_tol)
    f = first_run(max_iter, ct, pri_tol, dua_tol)
    out = {"first run " + (str(f) if f < 8 else ">= 8")}
    if runs:
        out.add(f"{len(runs)} run" + ("s" if len(runs) > 1 else ""))
    if tail and n_res:
        t = runs[-1][2]
        out.add("tail " + (str(t) if t < 7 else ">= 7") + " behind a check")
    if max_iter > 0 and ct > 0 and max_iter % ct == 0:
        out.add("no tail")
    if tail and len(segments) == 1 and ct == 0:
        out.add("single run, no check")
    if tail and len(segments) == 1 and ct > max_iter and reach:
        out.add("single run, check beyond max_iter")
    if not reach and ct > 0 and tail and n_res == 1 and len(runs) == 2 and runs[0][2] == (max_iter // ct) * ct - 1:
        out.add("forced with checks")
    out.add("pair " + ("both" if reach else "none" if pri_tol == 0.0 and dua_tol == 0.0 else "pri" if pri_tol > 0.0 else "dua"))
    return out


# ---- the problem, and the oracle's side
def problem(pkg, shape=SHAPE):
    return _problem(pkg.problems, shape)


def x0s(pkg, prob, batch, shape=SHAPE):
    return _x0s(pkg.problems, prob, shape, batch)


def goals(prob, batch):
    return _goals(prob, batch)


class OracleBatch:
    """One OraclePort per instance, so that a batch keeps every instance's workspace from one solve to the next as a handle does."""

    def __init__(self, prob, batch):
        import pyoracle as O
        self.prob, self.batch = prob, batch
        self.orcs = [O.OraclePort(prob).load_problem(prob) for _ in range(batch)]
        self.reset_workspace()

    def update_settings(self, **kw):
        for o in self.orcs:
            o.update_settings(**kw)

    def reset_workspace(self):
        for o in self.orcs:
            o.reset_workspace()

    def solve(self, x0):
        """(states [nx, N, batch], controls [nu, N-1, batch], iterations, statuses, residuals [4, batch]) as get_solution_batch and
        get_stats_batch return them."""
        p, b = self.prob, self.batch
        sx, su = np.zeros((p.nx, p.N, b), order="F"), np.zeros((p.nu, p.N - 1, b), order="F")
        it, status, res = np.zeros(b, dtype=np.int32), np.zeros(b, dtype=np.int32), np.zeros((4, b), order="F")
        for i, o in enumerate(self.orcs):
            o.set_x0(np.ascontiguousarray(x0[:, i]))
            o.solve()
            sx[:, :, i], su[:, :, i] = o.solution()
            st = o.stats()
            it[i], status[i] = st["iter"], st["status"]
            res[:, i] = st["pri_x"], st["dua_x"], st["pri_u"], st["dua_u"]
        return sx, su, it, status, res


def oracle_cell(orc, x0, max_iter, ct, pri_tol, dua_tol):
    """(cold solve, warm solve) of one cell on an OracleBatch: from a reset workspace at x0, then at WARM * x0."""
    orc.update_settings(abs_pri_tol=pri_tol, abs_dua_tol=dua_tol, max_iter=max_iter, check_termination=ct)
    orc.reset_workspace()
    cold = orc.solve(x0)
    return cold, orc.solve(WARM * x0)


def oracle_sequence(orc, x0, sequence=SEQUENCE, tol_scale=1.0):
    """The solves of a handover sequence on an OracleBatch, no reset between the steps."""
    out = []
    for max_iter, ct, tol, scale in sequence:
        orc.update_settings(abs_pri_tol=tol * tol_scale, abs_dua_tol=tol * tol_scale, max_iter=max_iter, check_termination=ct)
        out.append(orc.solve(scale * x0))
    return out
