"""The CPU side of tests/test_lean_run_structure_gpu.py: the Python restatement of layout D's lean-run loop (tests/lean_run_cases.py) against
the two other statements of it, the coverage of its settings grid, and the conditions the grid's inputs must meet on the oracle.

Coverage is asserted, not assumed: every class of cut in CLASSES is hit by a cell whose first run is at least PARK_MIN_RUN rounds, so that
the park kernels load there, and -- where a launch of that class can have a shorter first run at all -- by one below the threshold, where
the shared kernels run. Taking a check interval out of GRID makes these assertions fail (shown below for check_termination = 8).

On the oracle (quadrotor N=50, tolerance 0.1, batch 9, a cold solve and the warm one behind it at 0.9 x0): no verdict of the grid or of the
handover sequence is marginal -- a tolerance 1e-6 smaller or larger, far more than the kernels' rounding differs from the oracle's, gives the
same iteration counts and statuses --, so the GPU test may ask for exact counts; and wherever more than one check falls into a launch the
first wavefront holds a converged instance (status 1, fewer than max_iter iterations: a dead row inside later runs) beside one that runs to
max_iter, while instance 8, the third wavefront's only live row, converges at the first check, so that its wavefront leaves at the next
run's control block. With check intervals 7 and 8 and max_iter beyond the first check, the cold counts of the first wavefront are
[7, max, 7, 14] from max_iter = 14 on and [7, max, 7, max] below (8 and 16 with an interval of 8)."""
from __future__ import annotations

import numpy as np
import pytest

import lean_run_cases as L
from lean_run_cases import GRID, PAIRS, PARK_MIN_RUN, SEQUENCE, TOL

FIRST_RUNS = ["first run " + n for n in ("0", "1", "2", "5", "6", "7", ">= 8")]
# class -> can a launch of this class have a first run below PARK_MIN_RUN with the grid's check intervals?  A tail of t rounds behind a check
# needs an interval of at least t + 1, and the first run is then at least t rounds long: tails of 6 and more never come with a short first
# run, and a tail of 5 does so only with an interval of exactly 6, which the grid does not have (its intervals are 0, 1, 2, 3, 7, 8).
CLASSES = {
    "1 run": True, "2 runs": True, "3 runs": True, "4 runs": True,
    "tail 1 behind a check": True, "tail 2 behind a check": True, "tail 5 behind a check": False, "tail 6 behind a check": False,
    "tail >= 7 behind a check": False,
    "no tail": True, "single run, no check": True, "single run, check beyond max_iter": True, "forced with checks": True,
    "pair both": True, "pair none": True, "pair pri": True, "pair dua": True,
}


def _hits(grid):
    """{class: [cells above the threshold, cells below it]} over a grid crossed with the four tolerance pairs."""
    hits = {}
    for max_iter, ct in grid:
        for pair in PAIRS:
            tols = L.pair_tols(pair)
            park = L.first_run(max_iter, ct, *tols) >= PARK_MIN_RUN
            for c in L.classes(max_iter, ct, *tols):
                hits.setdefault(c, [[], []])[0 if park else 1].append((max_iter, ct, pair))
    return hits


def _missing(grid):
    hits = _hits(grid)
    missing = [c for c in FIRST_RUNS if c not in hits]
    for c, below in CLASSES.items():
        above_cells, below_cells = hits.get(c, [[], []])
        if not above_cells:
            missing.append(c + " (park kernels)")
        if below and not below_cells:
            missing.append(c + " (first run below the threshold)")
        if not below:
            assert not below_cells, (c, below_cells)  # (the table above says there is none)
    return missing


def test_the_grid_is_the_one_the_module_states():
    assert len(GRID) == 84 and len(set(GRID)) == 84
    for ct in (2, 3, 7, 8):
        assert [m for m, c in GRID if c == ct] == list(range(3 * ct + 3))
    for ct in (0, 1):
        assert [m for m, c in GRID if c == ct] == [0, 1, 2, 5, 6, 7]
    assert [L.pair_tols(p) for p in PAIRS] == [(TOL, TOL), (0.0, 0.0), (TOL, 0.0), (0.0, TOL)]
    assert set(L.BATCHES) == {1, 5, 9} and L.BATCHES[1] == L.BATCHES[5] == (7,) and set(L.BATCHES[9]) == {c for _, c in GRID}


def test_the_restatement_agrees_with_need_res_and_with_the_plans_first_run():
    """Every iteration with need_res is a "res" segment and no other is; the runs and the "res" iterations cover 1 .. max_iter once, in order;
    the first run is the one tinympc_plan.hip: first_lean_run states (restated as _first_run in test_layout_d_lean_park_gpu.py)."""
    from test_layout_d_lean_park_gpu import _first_run
    settings = [(m, ct) for ct in range(0, 12) for m in range(0, 3 * max(ct, 3) + 3)] + list(GRID)
    for max_iter, ct in settings:
        for pri, dua in [L.pair_tols(p) for p in PAIRS]:
            segments, tail = L.lean_runs(max_iter, ct, pri, dua)
            res = [s[1] for s in segments if s[0] == "res"]
            assert res == [it for it in range(1, max_iter + 1) if L.need_res(it, max_iter, ct, pri, dua)], (max_iter, ct, pri, dua, segments)
            covered = []
            for s in segments:
                covered += [s[1]] if s[0] == "res" else list(range(s[1] + 1, s[1] + s[2] + 1))
                assert s[0] == "res" or s[2] >= 1
            assert covered == list(range(1, max_iter + 1)), (max_iter, ct, pri, dua, segments)
            assert not any(a[0] == b[0] == "run" for a, b in zip(segments, segments[1:])), segments  # (a run ends at an iteration with residuals, or at max_iter)
            assert tail == (max_iter > 0 and not L.need_res(max_iter, max_iter, ct, pri, dua))
            if pri == dua:
                assert L.first_run(max_iter, ct, pri, dua) == _first_run(max_iter, ct, pri), (max_iter, ct, pri)
            else:  # one tolerance zero: nothing can converge, the cut is the forced one
                assert segments == L.lean_runs(max_iter, ct, 0.0, 0.0)[0]


def test_every_class_of_cut_is_in_the_grid_above_and_below_the_park_threshold():
    assert _missing(GRID) == []
    hits = _hits(GRID)
    for c in FIRST_RUNS[:4]:  # first runs below the threshold cannot load the park kernels, the others always do
        assert not hits[c][0] and hits[c][1], c
    for c in FIRST_RUNS[4:]:
        assert hits[c][0] and not hits[c][1], c


def test_the_coverage_assertions_notice_a_class_that_leaves_the_grid():
    without_8 = [c for c in GRID if c[1] != 8]
    assert "tail >= 7 behind a check (park kernels)" in _missing(without_8)
    without_0 = [c for c in GRID if c[1] != 0]
    assert "single run, no check (park kernels)" in _missing(without_0)
    assert _missing([c for c in GRID if c[1] not in (2, 3)])  # (four runs below the threshold, among others)


def test_the_lean_words_follow_the_plan():
    for max_iter, ct in GRID:
        for pair in PAIRS:
            tols = L.pair_tols(pair)
            assert L.lean_words("plain", L.SHAPE, max_iter, ct, *tols) == ()
            words = L.lean_words("park", L.SHAPE, max_iter, ct, *tols)
            if max_iter <= 0 or (ct == 1 and pair == "both"):
                assert words == ()
            else:
                assert words[:4] == ("lean", "lds-start", "trim", "share")
                assert ("park" in words) == (L.first_run(max_iter, ct, *tols) >= PARK_MIN_RUN)
                assert L.lean_words("share", L.SHAPE, max_iter, ct, *tols) == words[:4]
                assert L.lean_words("park", "cartpole20", max_iter, ct, *tols) == words[:4]  # (no LDS slots, no park kernels)


def test_the_handover_sequence_walks_through_the_kernels_as_stated():
    """park -> share -> park, a tail of one behind dead rows -> plain -> park, a tail of one behind the first check -> share -> park, a tail
    of two -> nothing -> park, a tail of seven -> park, a tail of six."""
    walk = []
    for max_iter, ct, tol, _ in SEQUENCE:
        words = L.lean_words("park", L.SHAPE, max_iter, ct, tol, tol)
        segments, tail = L.lean_runs(max_iter, ct, tol, tol)
        behind_check = tail and any(s[0] == "res" for s in segments)
        walk.append((words[-1] if words else "plain" if max_iter > 0 else "nothing", L.runs_of(segments)[-1][2] if behind_check else None))
    assert walk == [("park", None), ("share", None), ("park", 1), ("plain", None), ("park", 1), ("share", None), ("park", 2), ("nothing", None),
                    ("park", 7), ("park", 6)], walk
    assert all(abs(scale) <= 2.0 and m <= 40 for m, _, _, scale in SEQUENCE)


# ---- the oracle's side
SCALES = (1.0 - 1e-6, 1.0, 1.0 + 1e-6)


@pytest.fixture(scope="module")
def oracle_grid(pkg):
    """{tolerance scale: {(max_iter, ct): (cold, warm)}} for the pair (tol, tol), batch 9."""
    prob = L.problem(pkg)
    x0 = L.x0s(pkg, prob, 9)
    orc = L.OracleBatch(prob, 9)
    return {sc: {(m, ct): L.oracle_cell(orc, x0, m, ct, TOL * sc, TOL * sc) for m, ct in GRID} for sc in SCALES}


@pytest.fixture(scope="module")
def oracle_sequences(pkg):
    prob = L.problem(pkg)
    x0 = L.x0s(pkg, prob, 9)
    return {sc: L.oracle_sequence(L.OracleBatch(prob, 9), x0, tol_scale=sc) for sc in SCALES}


def test_no_verdict_of_the_grid_is_marginal_on_the_oracle(oracle_grid):
    marginal = []
    for cell in GRID:
        for k, solve in enumerate(("cold", "warm")):
            it, status = oracle_grid[1.0][cell][k][2:4]
            for sc in SCALES:
                o_it, o_status = oracle_grid[sc][cell][k][2:4]
                if not (np.array_equal(it, o_it) and np.array_equal(status, o_status)):
                    marginal.append((cell, solve, sc))
    assert marginal == []


def _mixed_first_wavefront(it, status, max_iter):
    it, status = np.asarray(it)[:4], np.asarray(status)[:4]
    return bool(np.any((status == 1) & (it < max_iter)) and np.any((status != 1) & (it == max_iter)))


def test_the_first_wavefront_mixes_dead_and_live_rows_and_the_third_leaves_at_the_first_check(oracle_grid):
    for max_iter, ct in GRID:
        if ct not in (7, 8) or max_iter <= ct:
            continue
        _, _, it, status, _ = oracle_grid[1.0][(max_iter, ct)][0]
        assert _mixed_first_wavefront(it, status, max_iter), (max_iter, ct, it, status)
        assert it[8] == ct and status[8] == 1, (max_iter, ct, it, status)
        late = 2 * ct if max_iter >= 2 * ct else max_iter
        assert list(it[:4]) == [ct, max_iter, ct, late] and list(status[:4]) == [1, 11, 1, 1 if max_iter >= 2 * ct else 11], (max_iter, ct, it, status)
        # a check at which every live instance of a wavefront but not of the launch converges: the second wavefront goes on
        assert np.any(it[4:8] > ct), (max_iter, ct, it)


def test_the_handover_sequence_meets_the_same_conditions_on_the_oracle(oracle_sequences):
    for k, (max_iter, ct, tol, _) in enumerate(SEQUENCE):
        _, _, it, status, _ = oracle_sequences[1.0][k]
        for sc in SCALES:
            np.testing.assert_array_equal(oracle_sequences[sc][k][2], it, err_msg=f"step {k} at tolerance scale {sc}")
            np.testing.assert_array_equal(oracle_sequences[sc][k][3], status, err_msg=f"step {k} at tolerance scale {sc}")
        if tol == 0.0 or ct == 1:
            assert tol > 0.0 or (np.all(it == max_iter) and np.all(status == 11)), (k, it, status)
            continue
        assert _mixed_first_wavefront(it, status, max_iter), (k, it, status)
        assert it[8] == ct and status[8] == 1, (k, it, status)
