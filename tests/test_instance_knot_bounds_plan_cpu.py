"""The LDS plan of layout D's per-knot bounds form (IKBND, with and without ITRAJ: d_vl / d_lds_bytes in tinympc_solve_d.hip, plan_for
in tinympc_jit.hip), without a GPU.

The restatement of test_instance_traj_plan_cpu.py with one more per-wavefront term: the wavefront's own clamp rows, lo and hi, 2 (N + 2)
vectors of 64 doubles (layout A's store, staged verbatim). It is pinned to the build: the bytes it gives for the compiled-in kernel
(__graft_entry__.HIP_BUILTINS_D_KBND: quadrotor N=20 with trajectories) equal the kernel's static LDS,
.amdhsa_group_segment_fixed_size in the build's assembly, which the kernel's own d_lds_bytes sized. On that footing, for the quadrotor
(nu = 4; a wavefront's share is 2,432 doubles with two wavefronts per SIMD in workgroups of four, 2,496 in workgroups of eight, 4,992
with one per SIMD):

  references constant over the horizon   128 (N + 2) + 16 (N - 1) doubles: two per SIMD up to N=15, one up to N=33, no plan from N=34;
  with per-instance trajectories         192 (N + 2) + 16 (N - 1) doubles: two per SIMD up to N=9 (workgroups of four) and at N=10
                                         (of eight), one up to N=22, no plan from N=23;
  N=20                                   103,936 B per workgroup, 148,992 B with trajectories; N=50 has no plan in either variant;
  cartpole (nu = 1)                      fits up to N=35, N=23 with trajectories.

(tests/test_instance_knot_bounds_d_gpu.py holds the host's plan_for to the same figures through tinympc_get_launch_info.)"""
from __future__ import annotations

import os
import re

import pytest

import __graft_entry__ as ge
from test_instance_traj_plan_cpu import CANDIDATES, LDS_PER_CU, OPS_DOUBLES, _define, first_fit, vreg_estimate, wave_doubles
from test_instance_traj_plan_cpu import d_lds_bytes as _lds_without
from test_instance_traj_plan_cpu import d_vl as _vl_without

BUILTIN = "k_builtin_d_quadrotor20_traj_kbnd"


def kbnd_doubles(N):
    """The wavefront's clamp rows: lo [N + 2][64] | hi [N + 2][64]."""
    return 2 * (N + 2) * 64


def d_vl(nu, N, wpg, cu_waves, vreg, itraj=False):
    """Slack slots in LDS with the clamp rows' term; -1 where the shape does not fit. (The term comes off a wavefront's room like the other
    per-wavefront terms; box path with constant tables, the only place the form exists.)"""
    room = (LDS_PER_CU // 8 * wpg // cu_waves - OPS_DOUBLES) // wpg - wave_doubles(nu, N, itraj=itraj) - kbnd_doubles(N)
    if room < 0:
        return -1
    want = max(N - 1 - vreg, 0)
    return want if want <= room // 64 else -1


def d_lds_bytes(nu, N, wpg, vl, itraj=False):
    return _lds_without(nu, N, wpg, vl, itraj=itraj) + 8 * wpg * kbnd_doubles(N)


def kbnd_plan(nx, nu, N, itraj=False):
    """-> {(wps, wpg): bytes per workgroup, or None where the form does not fit the candidate}."""
    out = {}
    for wps, wpg in CANDIDATES:
        vreg = vreg_estimate(N, wps)
        vl = d_vl(nu, N, wpg, 4 * wps, vreg, itraj) if vreg >= 0 else -1
        out[(wps, wpg)] = d_lds_bytes(nu, N, wpg, vl, itraj) if vl >= 0 else None
    return out


def _entry():
    entry = [e for e in ge.HIP_BUILTINS_D_KBND if e[0] == BUILTIN]
    assert len(entry) == 1 and entry[0] in ge.ALL_BUILTINS and entry[0] not in ge.HIP_BUILTINS_D
    return entry[0]


def test_without_the_term_the_restatement_is_the_siblings():
    """... and with it, a shape fits exactly where the sibling's arithmetic leaves the term's doubles to spare."""
    for nu, N, wpg, cu, vreg in ((4, 20, 4, 8, 19), (4, 20, 4, 4, 19), (4, 50, 4, 4, 49), (1, 20, 8, 8, 19), (4, 10, 8, 8, 9)):
        for itraj in (False, True):
            spare = (LDS_PER_CU // 8 * wpg // cu - OPS_DOUBLES) // wpg - wave_doubles(nu, N, itraj=itraj) - 64 * max(N - 1 - vreg, 0)
            if N - 1 <= vreg:  # (no slack in LDS: the sibling's verdict is the sign of what is left)
                assert (_vl_without(nu, N, wpg, cu, vreg, itraj=itraj) >= 0) == (spare >= 0), (nu, N, wpg, cu, itraj)
            assert (d_vl(nu, N, wpg, cu, vreg, itraj) >= 0) == (spare - kbnd_doubles(N) >= 0), (nu, N, wpg, cu, itraj)
            assert d_lds_bytes(nu, N, wpg, 0, itraj) - _lds_without(nu, N, wpg, 0, itraj=itraj) == 8 * wpg * kbnd_doubles(N)


def test_the_restatement_gives_the_static_lds_of_the_compiled_in_kernel():
    name, _, defs = _entry()
    path = ge.builtin_asm_path(name)
    if not os.path.exists(path):
        pytest.skip("no build assembly (run __graft_entry__.build())")
    m = re.search(r"\.amdhsa_kernel %s\b.*?\.amdhsa_group_segment_fixed_size (\d+)" % re.escape(name), open(path).read(), re.S)
    assert m, name
    nu, N, wps, wpg, vreg = (_define(defs, k) for k in ("NU", "N", "WPS", "WPG", "VREG"))
    assert _define(defs, "IKBND") == 1 and _define(defs, "ITRAJ") == 1 and _define(defs, "IGOAL") == 1 and _define(defs, "CT") == 1
    vl = d_vl(nu, N, wpg, 4 * wps, vreg, itraj=True)
    assert vl == 0
    assert d_lds_bytes(nu, N, wpg, vl, itraj=True) == int(m.group(1)) == 148992, (vl, m.group(1))


def test_the_compiled_in_kernel_has_the_options_the_plan_gives():
    _, source, defs = _entry()
    assert source == "tinympc_solve_d.hip"
    (wps, wpg), lds = first_fit(kbnd_plan(12, 4, 20, itraj=True))
    assert (wps, wpg, lds) == (1, 4, 148992)
    assert defs == ["-DTINY_JIT_NX=12", "-DTINY_JIT_NU=4", "-DTINY_JIT_N=20", "-DTINY_JIT_VREG=%d" % vreg_estimate(20, wps), "-DTINY_JIT_WPS=%d" % wps,
                    "-DTINY_JIT_WPG=%d" % wpg, "-DTINY_JIT_CT=1", "-DTINY_JIT_FAM=0", "-DTINY_JIT_ADAPT=0", "-DTINY_JIT_IGOAL=1", "-DTINY_JIT_ITRAJ=1",
                    "-DTINY_JIT_IKBND=1"], defs


# (variant, the last N on two wavefronts per SIMD in workgroups of four, ... of eight, the last N with a plan)
LIMITS = {False: (15, 15, 33), True: (9, 10, 22)}


@pytest.mark.parametrize("itraj", [False, True], ids=["constant-references", "trajectories"])
def test_the_quadrotors_limits_come_from_the_arithmetic(itraj):
    last24, last28, last = LIMITS[itraj]
    taken = {N: first_fit(kbnd_plan(12, 4, N, itraj))[0] for N in range(4, 60)}
    print("quadrotor, itraj=%s:" % itraj, taken)
    for N in range(4, 60):
        want = (2, 4) if N <= last24 else (2, 8) if N <= last28 else (1, 4) if N <= last else None
        assert taken[N] == want, (N, taken[N], want)
    # every N <= 20 by name: which candidate it takes
    assert [taken[N] for N in range(4, 21)] == [(2, 4) if N <= last24 else (2, 8) if N <= last28 else (1, 4) for N in range(4, 21)]
    # ... and the limits are where the rows and d reach a wavefront's share
    rows = (3 if itraj else 2) * 64
    need = lambda N: rows * (N + 2) + 16 * (N - 1)
    share2, share28, share1 = (LDS_PER_CU // 8 // 2 - OPS_DOUBLES) // 4, (LDS_PER_CU // 8 - OPS_DOUBLES) // 8, (LDS_PER_CU // 8 - OPS_DOUBLES) // 4
    assert (share2, share28, share1) == (2432, 2496, 4992)
    assert need(last24) <= share2 < need(last24 + 1)
    assert need(last28) <= share28 < need(last28 + 1)
    assert need(last) <= share1 < need(last + 1)


def test_n20_per_workgroup():
    assert first_fit(kbnd_plan(12, 4, 20)) == ((1, 4), 103936)
    assert first_fit(kbnd_plan(12, 4, 20, itraj=True)) == ((1, 4), 148992)
    assert 148992 <= LDS_PER_CU


def test_quadrotor50_has_no_plan():
    for itraj in (False, True):
        plan = kbnd_plan(12, 4, 50, itraj)
        print("quadrotor N=50, itraj=%s:" % itraj, plan)
        assert all(v is None for v in plan.values())
    assert kbnd_doubles(50) > (LDS_PER_CU // 8 - OPS_DOUBLES) // 4  # the clamp rows alone exceed a wavefront's share


def test_the_cartpoles_limits():
    for itraj, last in ((False, 35), (True, 23)):
        fits = [N for N in range(4, 80) if first_fit(kbnd_plan(4, 1, N, itraj))[0] is not None]
        assert fits == list(range(4, last + 1)), (itraj, fits[-1])
    assert first_fit(kbnd_plan(4, 1, 20))[0] == (1, 4) and first_fit(kbnd_plan(4, 1, 20, itraj=True))[0] == (1, 4)
