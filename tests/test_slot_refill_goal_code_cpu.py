"""The code of slot refill for layout D's per-instance goal form (`REFILL && IGOAL`, tinympc_solve_d.hip): the compiled-in kernels
k_admm_solve_d_refill_gbnd<...> exist for the three compiled-in shapes, fit the register file and keep scratch out of their sweeps
(rare paths -- write-back and refill of a row, once per instance -- may spill: the rule tests/test_isa_hazards.py states for the
shared refill kernels); the run-time specialisation compiles under hiprtc, keeps the same rule, and really is another kernel than
the shared refill one (whose entry point used to drop the goal flag silently)."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest
from conftest import ROOT
from test_isa_hazards import CSRC, _hiprtc_compile

from tools.isa_lint import lint as _lint

SHAPES = [(12, 4, 50), (4, 1, 20), (4, 1, 10)]
JIT_DEFS = ("-DTINY_JIT_NX=12 -DTINY_JIT_NU=4 -DTINY_JIT_N=20 -DTINY_JIT_VREG=19 -DTINY_JIT_WPS=2 -DTINY_JIT_WPG=4 -DTINY_JIT_CT=1 "
            "-DTINY_JIT_FAM=0 -DTINY_JIT_ADAPT=0 -DTINY_JIT_REFILL=1").split()


def _sweep_blocks(body: str) -> list[str]:
    return [b for b in re.split(r"^\.LBB\d+_\d+:", body, flags=re.M) if b.count("v_fmac_f64_dpp") >= 15]


def test_compiled_in_goal_refill_kernels_exist_and_keep_their_sweeps_out_of_scratch():
    import __graft_entry__ as ge
    built = ge.device_asm_path("tinympc_solve_dr.hip")
    if not os.path.exists(built):
        pytest.skip("no build assembly (run __graft_entry__.build())")
    text = open(built).read()
    meta = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.name:\s+(\S+)\n(?:(?!\.name:).)*?\.vgpr_count:\s+(\d+)", text, re.S)}
    for nx, nu, N in SHAPES:
        names = [m.group(1) for m in re.finditer(r"\.amdhsa_kernel (\S+)", text)
                 if "k_admm_solve_d_refill_gbndILi%dELi%dELi%dE" % (nx, nu, N) in m.group(1)]
        assert len(names) == 1, (nx, nu, N, names)
        name = names[0]
        body = re.search(r"^%s:(.*?)^\.Lfunc_end" % re.escape(name), text, re.S | re.M).group(1)
        sweeps = _sweep_blocks(body)
        assert len(sweeps) >= 2, name
        for b in sweeps:
            assert "scratch_" not in b, f"{name}: a sweep block uses scratch"
        assert name in meta and meta[name] <= 256, (name, meta.get(name))


def test_goal_refill_specialisation_compiles_under_hiprtc():
    rc, log = _hiprtc_compile('#include "tinympc_solve_d.hip"\n',
                              ["--offload-arch=gfx950", "-O3", "-std=c++17", "-DTINY_JIT=1", "-I" + CSRC] + JIT_DEFS + ["-DTINY_JIT_IGOAL=1"])
    assert rc == 0, log[-2000:]


def _device_asm(tmp_path, tag, extra):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / f"jit_{tag}.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "-w", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-DTINY_JIT=1"] +
                   JIT_DEFS + extra + ["-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "tinympc_solve_d.hip")], check=True, timeout=900)
    return out.read_text()


def _instructions(text: str) -> list[str]:
    body = re.search(r"^tinympc_jit_solve:(.*?)^\.Lfunc_end", text, re.S | re.M).group(1)
    lines = [l.split(";")[0].strip() for l in body.splitlines()]
    return [l for l in lines if l and not l.startswith(".")]


def test_goal_refill_specialisation_is_its_own_kernel_with_clean_sweeps(tmp_path):
    """The same defines through hipcc: no DPP hazard, sweep blocks free of scratch, at most 256 registers -- and not the code of the
    shared refill kernel (without -DTINY_JIT_IGOAL=1): it loads a taking row's constants from the goal stores."""
    goal = _device_asm(tmp_path, "goal", ["-DTINY_JIT_IGOAL=1"])
    checked, bad = _lint(goal)
    assert checked > 100 and not bad, bad[:3]
    body = re.search(r"^tinympc_jit_solve:(.*?)^\.Lfunc_end", goal, re.S | re.M).group(1)
    sweeps = _sweep_blocks(body)
    assert len(sweeps) >= 2
    for b in sweeps:
        assert "scratch_" not in b, "a sweep block of the goal form's slot-refill specialisation uses scratch"
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", goal).group(1)) <= 256
    shared = _device_asm(tmp_path, "shared", [])
    a, b = _instructions(goal), _instructions(shared)
    assert a != b, "the refill entry point ignores the goal flag"
    assert sum("global_load" in l for l in a) > sum("global_load" in l for l in b)  # (the reloads of the four lane constants)
