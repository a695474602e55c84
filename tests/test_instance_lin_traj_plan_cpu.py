"""The LDS plan of layout D's per-instance families on per-instance trajectories (ILIN with ITRAJ: d_vl / d_lds_bytes in
tinympc_solve_d.hip, plan_for in tinympc_jit.hip), without a GPU.

The restatement of the two constexpr functions is the sibling file's (test_instance_traj_plan_cpu.py, pinned there to the static LDS of
every compiled-in layout D kernel -- this form's included: its parametrised test runs over __graft_entry__.HIP_BUILTINS_D); what this
file adds is plan_for's register side for the families, restated below, and the figures of the combined form:

  a wavefront of the form holds its d ((N-1) * 4 nu doubles), its linear rows (3 nl vectors of 64 doubles, times N slots with rows per
  knot) and, behind them, its N + 2 linref rows of 64 doubles;
  the families' registers (eight per knot beside the slack) leave two wavefronts per SIMD only up to N=4: every shape below runs one per
  SIMD, workgroups of four, all N-1 slack knots in registers, on a wavefront's share of (20480 - 512) / 4 = 4,992 doubles;
  quadrotor N=20, one row: 304 + 192 + 1,408 doubles -- fits; rows per knot: 304 + 3,840 + 1,408 -- no plan, the mode stays on layout A;
  one row per knot fits up to N=17 (272 N + 112 <= 4,992), two up to N=10, three up to N=7;
  cartpole N=20 (nu=1: d is 76 doubles) and the rocket landing nx=6 nu=3 N=10 with one row and the slopes (108 + 192 + 768) fit.

(tests/test_instance_lin_traj_d_gpu.py holds the host's plan_for to the same figures through tinympc_get_launch_info.)"""
from __future__ import annotations

import __graft_entry__ as ge
from test_instance_traj_plan_cpu import CANDIDATES, LDS_PER_CU, OPS_DOUBLES, _define, d_d_doubles, d_lds_bytes, d_vl, first_fit, wave_doubles

SHARE_1 = (LDS_PER_CU // 8 - OPS_DOUBLES) // 4  # doubles of a wavefront with one per SIMD: 4,992


def fam_vreg_estimate(N, wps):
    """plan_for's register estimate for the 16-lane families with constant tables: the slack knots kept in registers, -1 without a plan.
    (6 (N-1) + 120 registers for the families' duals, masks and scalars beside the box path's; measured: scratch from N=24 on, so N <= 22)"""
    ns = N - 1
    budget = 256 * (3 - wps) - (76 if wps == 2 else 110) - 32 - 2 * ns - (6 * ns + 96 + 24)
    if budget < 0 or 8 * ns + 336 >= 512:
        return -1
    return min(budget // 2, ns)


def lin_traj_plan(nx, nu, N, nl=1, knots=False, traj=True):
    """-> {(wps, wpg): bytes per workgroup, or None where the form does not fit the candidate}."""
    out = {}
    for wps, wpg in CANDIDATES:
        vreg = fam_vreg_estimate(N, wps)
        kw = dict(fam=True, ilin=nl, knots=N if knots else 0, itraj=traj)
        vl = d_vl(nu, N, wpg, 4 * wps, vreg, **kw) if vreg >= 0 else -1
        out[(wps, wpg)] = d_lds_bytes(nu, N, wpg, vl, **kw) if vl >= 0 else None
    return out


def longest_knots_horizon(nx, nu, nl):
    fits = [N for N in range(4, 40) if first_fit(lin_traj_plan(nx, nu, N, nl, knots=True))[0] is not None]
    assert fits == list(range(4, fits[-1] + 1)), fits
    return fits[-1]


def test_a_wavefront_has_4992_doubles_with_one_per_simd():
    assert SHARE_1 == 4992


def test_quadrotor20_one_row_fits_one_wavefront_per_simd():
    N, nu = 20, 4
    plan = lin_traj_plan(12, nu, N)
    print("quadrotor N=20, 1 row + trajectories:", plan)
    assert plan[(2, 4)] is None and plan[(2, 8)] is None  # (the families' registers, not the LDS)
    (wps, wpg), lds = first_fit(plan)
    assert (wps, wpg) == (1, 4)
    assert wave_doubles(nu, N, ilin=1, itraj=True) == 304 + 192 + 1408 <= SHARE_1
    # 4,096 B of operators + four wavefronts' d, rows and linref rows; no slack in LDS
    assert lds == 4096 + 4 * 8 * (304 + 192 + 1408) == 65024
    # ... the lin1 form's bytes and the rows of 22 knots per wavefront
    assert lds == d_lds_bytes(nu, N, 4, 0, fam=True, ilin=1) + 4 * (N + 2) * 512


def test_the_compiled_in_kernel_has_the_options_the_plan_gives():
    entry = [e for e in ge.HIP_BUILTINS_D if e[0] == "k_builtin_d_quadrotor20_lin1_traj"]
    assert len(entry) == 1
    defs = entry[0][2]
    (wps, wpg), _ = first_fit(lin_traj_plan(12, 4, 20))
    assert (_define(defs, "WPS"), _define(defs, "WPG"), _define(defs, "VREG")) == (wps, wpg, fam_vreg_estimate(20, wps)), defs
    assert (_define(defs, "ILIN"), _define(defs, "ITRAJ"), _define(defs, "IKNOT"), _define(defs, "FAM"), _define(defs, "IGOAL")) == (1, 1, 0, 1, 1), defs
    # (the specialiser looks a compiled-in kernel up by its defines in its own order: the trajectory's define is the last)
    assert defs[-2:] == ["-DTINY_JIT_ILIN=1", "-DTINY_JIT_ITRAJ=1"], defs


def test_quadrotor20_rows_per_knot_fit_no_plan():
    N, nu = 20, 4
    plan = lin_traj_plan(12, nu, N, knots=True)
    print("quadrotor N=20, 1 row per knot + trajectories:", plan)
    assert all(v is None for v in plan.values())
    assert wave_doubles(nu, N, ilin=1, knots=N, itraj=True) == 304 + 3840 + 1408 > SHARE_1
    # ... while either half alone has one: rows per knot in the goal form, trajectories with one row
    assert first_fit(lin_traj_plan(12, nu, N, knots=True, traj=False))[0] == (1, 4)
    assert first_fit(lin_traj_plan(12, nu, N))[0] == (1, 4)


def test_the_longest_horizon_with_rows_per_knot():
    """One row per knot: 192 N + 64 (N + 2) + 16 (N - 1) = 272 N + 112 doubles of 4,992."""
    assert [longest_knots_horizon(12, 4, nl) for nl in (1, 2, 3)] == [17, 10, 7]
    N = 17
    assert wave_doubles(4, N, ilin=1, knots=N, itraj=True) == 272 * N + 112 <= SHARE_1 < 272 * (N + 1) + 112
    (wps, wpg), lds = first_fit(lin_traj_plan(12, 4, N, knots=True))
    assert (wps, wpg) == (1, 4) and lds == 4096 + 4 * 8 * (272 * N + 112)
    # (without trajectories the per-knot form goes to N=22, where the families' registers end)
    assert first_fit(lin_traj_plan(12, 4, 22, knots=True, traj=False))[0] == (1, 4)
    assert first_fit(lin_traj_plan(12, 4, 23, knots=True, traj=False))[0] is None


def test_cartpole20_fits():
    N, nu = 20, 1
    (wps, wpg), lds = first_fit(lin_traj_plan(4, nu, N))
    assert (wps, wpg) == (1, 4)
    assert d_d_doubles(nu, N) == 76
    assert lds == 4096 + 4 * 8 * (76 + 192 + 1408)


def test_rocket10_with_one_row_and_slopes_fits():
    """(the slopes are read per lane from the store at kernel start: no LDS of their own)"""
    N, nu = 10, 3
    (wps, wpg), lds = first_fit(lin_traj_plan(6, nu, N))
    assert (wps, wpg) == (1, 4)
    assert lds == 4096 + 4 * 8 * (108 + 192 + 768)
