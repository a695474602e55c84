"""The code of slot refill for layout D's per-instance trajectory and per-knot bounds forms (`REFILL && ITRAJ`, `REFILL && IKBND`,
tinympc_solve_d.hip): the compiled-in kernel k_builtin_d_quadrotor50_traj_refill and the run-time specialisations of the quadrotor N=20
fit the register file of their plan (512 VGPRs at one wavefront per SIMD, 256 at two), keep scratch out of their sweeps (rare paths --
write-back and refill of a row, once per instance -- may spill: the rule tests/test_isa_hazards.py states for the shared refill
kernels), and carry the restage of a taking row's column: LDS stores outside the sweep blocks, fed by global loads. The forms that have
no variant -- per-instance linear rows, per-instance models -- still refuse to compile with the refill define."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest
from conftest import ROOT
from test_isa_hazards import CSRC, _hiprtc_compile

from tools.isa_lint import lint as _lint

BUILTIN = "k_builtin_d_quadrotor50_traj_refill"
# (the options tinympc_jit.hip's d_label() hands the compiler for the quadrotor N=20: trajectories on two wavefronts per SIMD, trajectories
# with bounds per knot on one -- the plans of the plain kernels, k_builtin_d_quadrotor20_traj_kbnd's among them)
N20 = "-DTINY_JIT_NX=12 -DTINY_JIT_NU=4 -DTINY_JIT_N=20 -DTINY_JIT_VREG=19 -DTINY_JIT_WPS=%d -DTINY_JIT_WPG=4 -DTINY_JIT_CT=1 -DTINY_JIT_FAM=%d -DTINY_JIT_ADAPT=0 -DTINY_JIT_REFILL=1"
VARIANTS = {"traj": (2, ["-DTINY_JIT_IGOAL=1", "-DTINY_JIT_ITRAJ=1"]), "traj_kbnd": (1, ["-DTINY_JIT_IGOAL=1", "-DTINY_JIT_ITRAJ=1", "-DTINY_JIT_IKBND=1"])}


def _blocks(body: str) -> list[str]:
    return re.split(r"^\.LBB\d+_\d+:", body, flags=re.M)


def _check_kernel(text: str, name: str, vgprs: int):
    body = re.search(r"^%s:(.*?)^\.Lfunc_end" % re.escape(name), text, re.S | re.M).group(1)
    blocks = _blocks(body)
    sweeps = [b for b in blocks if b.count("v_fmac_f64_dpp") >= 15]
    rest = [b for b in blocks if b.count("v_fmac_f64_dpp") < 15]
    assert len(sweeps) >= 2, name
    for b in sweeps:
        assert "scratch_" not in b, f"{name}: a sweep block uses scratch"
    assert len(re.findall(r"\.vgpr_count:", text)) == 1 and int(re.search(r"\.vgpr_count:\s+(\d+)", text).group(1)) <= vgprs  # (one kernel per file)
    # the restage: LDS stores outside the sweep blocks ...
    assert any("ds_write_b64" in b for b in rest), f"{name}: no ds_write_b64 outside the sweeps"
    # ... and the copy loop itself: a block without arithmetic of the sweeps that loads from global memory and stores 64-bit values into LDS
    # (two rows 512 bytes apart may go out as one ds_write2st64_b64)
    assert any("global_load_dwordx2" in b and re.search(r"ds_write(2st64)?_b64", b) and "v_fmac_f64" not in b for b in rest), f"{name}: no copy loop global -> LDS"


def test_compiled_in_trajectory_refill_kernel_fits_its_plan_and_keeps_its_sweeps_out_of_scratch():
    import __graft_entry__ as ge
    assert BUILTIN in [e[0] for e in ge.HIP_BUILTINS_D_REFILL] and BUILTIN in [e[0] for e in ge.ALL_BUILTINS]
    plain = next(e for e in ge.HIP_BUILTINS_D if e[0] == "k_builtin_d_quadrotor50_traj")
    mine = next(e for e in ge.HIP_BUILTINS_D_REFILL if e[0] == BUILTIN)
    assert sorted(mine[2]) == sorted(plain[2] + ["-DTINY_JIT_REFILL=1"]) and mine[1] == plain[1]
    built = ge.builtin_asm_path(BUILTIN)
    if not os.path.exists(built):
        pytest.skip("no build assembly (run __graft_entry__.build())")
    text = open(built).read()
    checked, bad = _lint(text)
    assert checked > 100 and not bad, bad[:3]
    _check_kernel(text, BUILTIN, 512)  # (one wavefront per SIMD)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_refill_specialisations_compile_under_hiprtc(variant):
    wps, extra = VARIANTS[variant]
    rc, log = _hiprtc_compile('#include "tinympc_solve_d.hip"\n', ["--offload-arch=gfx950", "-O3", "-std=c++17", "-DTINY_JIT=1", "-I" + CSRC] + (N20 % (wps, 0)).split() + extra)
    assert rc == 0, log[-2000:]


@pytest.mark.parametrize("extra,fam,word", [(["-DTINY_JIT_IGOAL=1", "-DTINY_JIT_ILIN=1"], 1, "per-instance linear rows: no slot-refill variant"),
                                            (["-DTINY_JIT_IMOD=1"], 0, "per-instance models: no slot-refill variant")])
def test_forms_without_a_variant_still_refuse_the_refill_define(extra, fam, word):
    rc, log = _hiprtc_compile('#include "tinympc_solve_d.hip"\n', ["--offload-arch=gfx950", "-O3", "-std=c++17", "-DTINY_JIT=1", "-I" + CSRC] + (N20 % (1, fam)).split() + extra)
    assert rc != 0 and word in log, log[-2000:]


def _device_asm(tmp_path, tag, defs):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / f"jit_{tag}.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "-w", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-DTINY_JIT=1"] +
                   defs + ["-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "tinympc_solve_d.hip")], check=True, timeout=900)
    return out.read_text()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_refill_specialisations_fit_their_plan_with_clean_sweeps(tmp_path, variant):
    """The same defines through hipcc: no DPP hazard, sweep blocks free of scratch, the register budget of the plan, the restage."""
    wps, extra = VARIANTS[variant]
    text = _device_asm(tmp_path, variant, (N20 % (wps, 0)).split() + extra)
    checked, bad = _lint(text)
    assert checked > 100 and not bad, bad[:3]
    _check_kernel(text, "tinympc_jit_solve", 256 if wps == 2 else 512)
