"""The LDS plan of layout D's per-instance trajectory form (ITRAJ: d_vl / d_lds_bytes in tinympc_solve_d.hip, plan_for in
tinympc_jit.hip), without a GPU.

The two constexpr functions live in the kernel's source, which no host compiler reads without HIP, so they are restated here and the
restatement is pinned to the build: for every compiled-in layout D specialisation (__graft_entry__.HIP_BUILTINS_D -- the model form,
the linear-row forms, the trajectory form: every per-wavefront term of the plan) its bytes must equal the kernel's static LDS,
.amdhsa_group_segment_fixed_size in the build's assembly, which the kernel's own d_lds_bytes sized. On that footing:

  a wavefront of the form holds its slack rows beyond the registers', its d ((N-1) * 4 nu doubles) and its N + 2 linref rows of 64 doubles;
  quadrotor and cartpole N=20 fit the first candidate, two wavefronts per SIMD (20 KB less the operators' share per wavefront);
  quadrotor N=50 fits only the last, one wavefront per SIMD: 8 * (512 + 4 * ((N + 2) * 64 + (N - 1) * 16)) bytes per workgroup of four;
  quadrotor N=100 fits none (its rows alone are 102 * 512 B = 52,224 B of a wavefront's 39,936): the form is refused.

(tests/test_instance_traj_d_gpu.py holds the host's plan_for to the same figures through tinympc_get_launch_info.)"""
from __future__ import annotations

import os
import re

import pytest

import __graft_entry__ as ge

LDS_PER_CU = 160 * 1024
OPS_DOUBLES = 2 * 16 * 16
MAX_LIN_ROWS = 32
FAM_DOUBLES = 3 * MAX_LIN_ROWS * 16
IMOD_WAVE_DOUBLES = 4 * (OPS_DOUBLES + 16)
CANDIDATES = ((2, 4), (2, 8), (1, 4))  # (wavefronts per SIMD, per workgroup), plan_for's order of preference


def d_d_doubles(nu, N):
    return ((N - 1) * 4 * nu + 1) & ~1


def wave_doubles(nu, N, imod=False, ilin=0, knots=0, itraj=False):
    """What a wavefront keeps in its own LDS region besides the slack: d, and the form's rows."""
    return d_d_doubles(nu, N) + (IMOD_WAVE_DOUBLES if imod else 0) + 3 * ilin * 64 * (knots if knots else 1) + ((N + 2) * 64 if itraj else 0)


def wg_doubles(N, ct=True, fam=False, imod=False, ilin=0):
    """The workgroup's shared part: operators, tables (bounds / references that vary over the horizon), the shared linear rows."""
    return (0 if imod else OPS_DOUBLES) + (0 if ct else 3 * (N + 2) * 16 + 16) + (FAM_DOUBLES if fam and not ilin else 0)


def d_vl(nu, N, wpg, cu_waves, vreg, ct=True, fam=False, imod=False, ilin=0, knots=0, itraj=False):
    """Slack slots in LDS; -1 where the shape does not fit (cu_waves wavefronts per CU share its 160 KB)."""
    room = (LDS_PER_CU // 8 * wpg // cu_waves - wg_doubles(N, ct, fam, imod, ilin)) // wpg - wave_doubles(nu, N, imod, ilin, knots, itraj)
    if room < 0:
        return -1
    want = max(N - 1 - vreg, 0)
    return want if want <= room // 64 else -1


def d_lds_bytes(nu, N, wpg, vl, ct=True, fam=False, imod=False, ilin=0, knots=0, itraj=False):
    return 8 * (wg_doubles(N, ct, fam, imod, ilin) + wpg * (vl * 64 + wave_doubles(nu, N, imod, ilin, knots, itraj)))


def vreg_estimate(N, wps):
    """plan_for's register estimate for the 16-lane box path with constant tables: the slack knots it keeps in registers."""
    budget = 256 * (3 - wps) - (76 if wps == 2 else 110) - 32 - 2 * (N - 1)
    return min(budget // 2, N - 1) if budget >= 0 else -1


def traj_plan(nx, nu, N):
    """-> {(wps, wpg): bytes per workgroup, or None where the form does not fit the candidate}."""
    out = {}
    for wps, wpg in CANDIDATES:
        vreg = vreg_estimate(N, wps)
        vl = d_vl(nu, N, wpg, 4 * wps, vreg, itraj=True) if vreg >= 0 else -1
        out[(wps, wpg)] = d_lds_bytes(nu, N, wpg, vl, itraj=True) if vl >= 0 else None
    return out


def first_fit(plan):
    return next(((c, plan[c]) for c in CANDIDATES if plan[c] is not None), (None, None))


def _define(defs, name, default=0):
    v = [d.split("=")[1] for d in defs if d.startswith("-DTINY_JIT_%s=" % name)]
    return int(v[0]) if v else default


@pytest.mark.parametrize("entry", ge.HIP_BUILTINS_D, ids=[e[0] for e in ge.HIP_BUILTINS_D])
def test_the_restatement_gives_the_static_lds_of_every_compiled_in_layout_d_kernel(entry):
    name, _, defs = entry
    path = ge.builtin_asm_path(name)
    if not os.path.exists(path):
        pytest.skip("no build assembly (run __graft_entry__.build())")
    m = re.search(r"\.amdhsa_kernel %s\b.*?\.amdhsa_group_segment_fixed_size (\d+)" % re.escape(name), open(path).read(), re.S)
    assert m, name
    nu, N, wps, wpg, vreg = (_define(defs, k) for k in ("NU", "N", "WPS", "WPG", "VREG"))
    kw = dict(ct=_define(defs, "CT", 1) != 0, fam=_define(defs, "FAM") != 0, imod=_define(defs, "IMOD") != 0, ilin=_define(defs, "ILIN"),
              knots=N if _define(defs, "IKNOT") else 0, itraj=_define(defs, "ITRAJ") != 0)
    vl = d_vl(nu, N, wpg, 4 * wps, vreg, **kw)
    assert vl >= 0, (name, kw)
    assert d_lds_bytes(nu, N, wpg, vl, **kw) == int(m.group(1)), (name, kw, vl, m.group(1))


def test_the_compiled_in_trajectory_kernel_has_the_options_the_plan_gives_quadrotor50():
    entry = [e for e in ge.HIP_BUILTINS_D if e[0] == "k_builtin_d_quadrotor50_traj"]
    assert len(entry) == 1
    (wps, wpg), _ = first_fit(traj_plan(12, 4, 50))
    defs = entry[0][2]
    assert (_define(defs, "WPS"), _define(defs, "WPG"), _define(defs, "VREG")) == (wps, wpg, vreg_estimate(50, wps)), defs


@pytest.mark.parametrize("nx,nu", [(12, 4), (4, 1)], ids=["quadrotor20", "cartpole20"])
def test_n20_fits_two_wavefronts_per_simd(nx, nu):
    N = 20
    plan = traj_plan(nx, nu, N)
    print("N=20 nu=%d:" % nu, plan)
    (wps, wpg), lds = first_fit(plan)
    assert (wps, wpg) == (2, 4)
    # the rows and d of four wavefronts beside the operators, all 19 slack knots in registers
    assert lds == 8 * (OPS_DOUBLES + 4 * ((N + 2) * 64 + d_d_doubles(nu, N)))
    assert lds <= LDS_PER_CU // 2  # (two such workgroups per CU)


def test_quadrotor50_fits_only_one_wavefront_per_simd():
    N, nu = 50, 4
    plan = traj_plan(12, nu, N)
    print("quadrotor N=50:", plan)
    assert plan[(2, 4)] is None and plan[(2, 8)] is None
    # 4,096 B of operators + four wavefronts' rows ((N + 2) * 512 B) and d ((N - 1) * 4 nu * 8 B); no padding, no slack in LDS
    assert plan[(1, 4)] == 4096 + 4 * ((N + 2) * 512 + (N - 1) * 4 * nu * 8)
    assert plan[(1, 4)] <= LDS_PER_CU
    # ... less than the per-knot linear rows' form takes at N=20 (one row per knot: 20 slots of three vectors)
    assert plan[(1, 4)] < d_lds_bytes(nu, 20, 4, 0, fam=True, ilin=1, knots=20)


def test_quadrotor100_fits_no_plan():
    plan = traj_plan(12, 4, 100)
    print("quadrotor N=100:", plan)
    assert all(v is None for v in plan.values())
    assert (100 + 2) * 512 > (LDS_PER_CU - 8 * OPS_DOUBLES) // 4  # the rows alone exceed a wavefront's share with one wavefront per SIMD


def test_the_limit_comes_from_the_arithmetic():
    """The longest quadrotor horizon the form holds is where rows + d reach a wavefront's share: somewhere past N = 60."""
    fits = [N for N in range(4, 129) if first_fit(traj_plan(12, 4, N))[0] is not None]
    assert fits == list(range(4, fits[-1] + 1)) and 60 <= fits[-1] < 100, fits[-1]
    N = fits[-1]
    share = (LDS_PER_CU // 8 - OPS_DOUBLES) // 4
    assert wave_doubles(4, N, itraj=True) <= share < wave_doubles(4, N + 1, itraj=True)
