"""Static checks of layout D's compiled-in per-instance trajectory kernel (quadrotor nx=12 nu=4 N=50: tinympc_solve_d.hip with
-DTINY_JIT_IGOAL=1 -DTINY_JIT_ITRAJ=1, __graft_entry__.HIP_BUILTINS_D) in the build's gfx950 assembly.

The form changes where the backward sweep's linref comes from -- the wavefront's own rows in LDS, one 64-bit read per step, issued a
block ahead --, not the per-lane arithmetic, which is the shared per-knot (!CT) form's: forward step 0 keeps only its input columns
(K0), the backward step's tail is the unfolded one (FOLD needs references constant over the horizon). So its iteration loop must hold
exactly the fused DPP FMAs of the goal kernel's loop of the same shape (k_admm_solve_d_gbnd<12,4,50,...> in tinympc_solve_d.hip's
assembly: FOLD changes the tail, never the chain; compared through the counting helper of test_layout_d_fold_code_cpu.py, not counted
here), and one or two v_fma_f64 more per backward step than that folded loop: the unfolded tail's r_s -- the difference the build's one
pair of a !CT and a CT loop of one shape shows (cartpole N=20: the build has no !CT instantiation of the quadrotor N=50) -- and the
step's accumulator start, which this form writes as a fused multiply-add. It touches global memory only in the rare
write-back blocks (the block rule of test_instance_models_d_code_cpu.py), scratch nowhere, and fits the one-wavefront-per-SIMD plan
without spills."""
from __future__ import annotations

import collections

import __graft_entry__ as ge
from test_instance_models_d_code_cpu import _loop_blocks, _read
from test_layout_d_fold_code_cpu import KERNELS, _loop_counts, _metadata

BUILTIN = "k_builtin_d_quadrotor50_traj"
CARTPOLE20 = {ct: "_ZN7tinympc14k_admm_solve_dILi4ELi1ELi20ELb%dELi4ELi0ELb0EEEvNS_11SolveParamsE" % ct for ct in (0, 1)}


def _asm():
    return _read(ge.builtin_asm_path(BUILTIN))


def test_the_kernel_is_registered_with_the_options_of_its_plan():
    entry = [e for e in ge.HIP_BUILTINS_D if e[0] == BUILTIN]
    assert entry and entry[0] in ge.ALL_BUILTINS  # (what the build compiles, registers and lints)
    assert len(entry) == 1 and entry[0][1] == "tinympc_solve_d.hip"
    defs = entry[0][2]
    assert "-DTINY_JIT_ITRAJ=1" in defs and "-DTINY_JIT_WPS=1" in defs and "-DTINY_JIT_VREG=49" in defs, defs
    assert "-DTINY_JIT_IGOAL=1" in defs and "-DTINY_JIT_CT=1" in defs and "-DTINY_JIT_WPG=4" in defs, defs


def test_one_wavefront_per_simd_without_spills_or_scratch():
    md = _metadata(_asm(), BUILTIN)
    print("trajectory form:", md)
    assert md["vgpr_count"] <= 512, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, md


def test_the_iteration_loop_has_the_unfolded_chain_and_touches_memory_only_in_its_rare_blocks():
    plain = _read(ge.device_asm_path("tinympc_solve_d.hip"))
    goal = _loop_counts(plain, KERNELS["goal"])
    var20, ct20 = _loop_counts(plain, CARTPOLE20[0]), _loop_counts(plain, CARTPOLE20[1])
    blocks = _loop_blocks(_asm(), BUILTIN)
    rare = [b for b in blocks if any(i.startswith(("global_", "flat_", "buffer_")) for i in b)]
    hot = [b for b in blocks if b not in rare]
    c = collections.Counter(i.split()[0] for b in hot for i in b)
    print("trajectory form, iteration loop: %d blocks (%d rare), %d fused DPP FMAs (goal kernel %d), v_fma_f64 %d (%d), VALU %d (%d), LDS reads %d (%d)"
          % (len(blocks), len(rare), c["v_fmac_f64_dpp"], goal["v_fmac_f64_dpp"], c["v_fma_f64"], goal["v_fma_f64"],
             sum(v for k, v in c.items() if k.startswith("v_")), sum(v for k, v in goal.items() if k.startswith("v_")),
             sum(v for k, v in c.items() if k.startswith("ds_read")), sum(v for k, v in goal.items() if k.startswith("ds_read"))))
    assert rare and hot
    assert goal["v_fmac_f64_dpp"] > 0 and c["v_fmac_f64_dpp"] == goal["v_fmac_f64_dpp"], (c["v_fmac_f64_dpp"], goal["v_fmac_f64_dpp"])
    # the chain does not depend on CT or FOLD: the build's !CT loop shows it on the shape it exists for
    assert var20["v_fmac_f64_dpp"] == ct20["v_fmac_f64_dpp"] > 0
    # the unfolded tail: one v_fma_f64 more for each of the N - 1 backward steps, as the !CT loop has over the CT loop (N = 20: 19)
    assert var20["v_fma_f64"] - ct20["v_fma_f64"] == 20 - 1, (var20["v_fma_f64"], ct20["v_fma_f64"])
    # ... and here at least that, at most one more again: a step's accumulator start, lr + cb | cb, is written as a fused multiply-add on
    # a lane constant in this form (the shared form's sum and select: the same bits), which a compiler may keep or split
    assert 50 - 1 <= c["v_fma_f64"] - goal["v_fma_f64"] <= 2 * (50 - 1), (c["v_fma_f64"], goal["v_fma_f64"])
    # no block of the loop, rare or not, touches scratch
    assert not [i for b in blocks for i in b if i.startswith("scratch_")]
    # LDS reads of the common path: the operators' rows, d, and one linref row per backward step -- all N - 1 slack knots are in registers,
    # so no more than the goal kernel, which reads the 25 slack rows it keeps in LDS in both sweeps
    assert sum(v for k, v in c.items() if k.startswith("ds_read")) <= sum(v for k, v in goal.items() if k.startswith("ds_read"))


def test_the_linked_form_passes_the_builds_lints():
    """The DPP-hazard lint and the in-flight lint of the build, on the assembly of the form that was linked (bare chain blocks unless the
    build had to fall back to the guarded ones)."""
    from tools.inflight_lint import lint as inflight_lint
    from tools.isa_lint import lint_file
    path = ge.builtin_asm_path(BUILTIN)
    _read(path)
    checked, bad = lint_file(path)
    assert checked >= 2 * 49 * 16 - 12 and not bad, (checked, bad[:3])
    assert not inflight_lint(path)


def test_the_plain_translation_unit_has_no_symbol_of_the_trajectory_kernel():
    text = _read(ge.device_asm_path("tinympc_solve_d.hip"))
    assert BUILTIN not in text and "k_builtin" not in text
    assert BUILTIN in _asm()
