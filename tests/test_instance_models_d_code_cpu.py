"""Static checks of layout D's compiled-in per-instance model kernel (quadrotor nx=12 nu=4 N=50: tinympc_solve_d.hip with
-DTINY_JIT_IMOD=1, __graft_entry__.HIP_BUILTINS_D) in the build's gfx950 assembly.

The form changes where the sweeps' operands come from -- every wavefront's four operator blocks in its own LDS region, the constants
from the instance's block --, not the per-lane arithmetic: its iteration loop must hold exactly the fused DPP FMAs of the goal kernel's
loop (k_admm_solve_d_gbnd<12,4,50,...> in tinympc_solve_d.hip's assembly; compared, not counted here), touch global memory only in the
rare write-back blocks (the block rule of test_layout_d_lean_code_cpu.py: a block with a global / flat / buffer instruction is a rare
one), touch scratch nowhere, and fit the one-wavefront-per-SIMD plan without spills. It is a translation unit of its own: nothing of it
reaches tinympc_solve_d.hip's code."""
from __future__ import annotations

import collections
import os
import re

import pytest

import __graft_entry__ as ge
from test_layout_d_fold_code_cpu import KERNELS, _loop_counts, _metadata

BUILTIN = "k_builtin_d_quadrotor50_models"


def _read(path):
    if not os.path.exists(path):
        pytest.skip("no build assembly (run __graft_entry__.build())")
    return open(path).read()


def _asm():
    return _read(ge.builtin_asm_path(BUILTIN))


def _loop_blocks(text: str, kernel: str):
    """The basic blocks (lists of instruction lines) of the iteration loop: the widest span between a label and a branch back to it."""
    m = re.search(r"^%s:(.*?)^\.Lfunc_end" % re.escape(kernel), text, re.S | re.M)
    assert m, kernel
    lines = [x.split(";")[0].rstrip() for x in m.group(1).split("\n")]
    labels, loop = {}, None
    for i, x in enumerate(lines):
        lm = re.match(r"^(\.LBB\d+_\d+):", x)
        if lm:
            labels[lm.group(1)] = i
        bm = re.search(r"\ss_c?branch\w*\s+(\.LBB\d+_\d+)", x)
        if bm and bm.group(1) in labels and (loop is None or i - labels[bm.group(1)] > loop[1] - loop[0]):
            loop = (labels[bm.group(1)], i)
    assert loop, "no loop in " + kernel
    blocks, cur = [], []
    for x in lines[loop[0]:loop[1] + 1]:
        if re.match(r"^\.LBB\d+_\d+:", x):
            blocks.append(cur)
            cur = []
        elif x.startswith("\t") and not x.strip().startswith("."):
            cur.append(x.strip())
    blocks.append(cur)
    return blocks


def test_the_kernel_is_registered_with_the_options_of_its_plan():
    entry = [e for e in ge.HIP_BUILTINS_D if e[0] == BUILTIN]
    assert entry and entry[0] in ge.ALL_BUILTINS  # (what the build compiles, registers and lints)
    assert len(entry) == 1 and entry[0][1] == "tinympc_solve_d.hip"
    assert "-DTINY_JIT_IMOD=1" in entry[0][2] and "-DTINY_JIT_WPS=1" in entry[0][2] and "-DTINY_JIT_VREG=49" in entry[0][2], entry[0][2]


def test_one_wavefront_per_simd_without_spills_or_scratch():
    md = _metadata(_asm(), BUILTIN)
    assert md["vgpr_count"] <= 512, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, md


def test_the_iteration_loop_has_the_goal_kernels_chain_and_touches_memory_only_in_its_rare_blocks():
    goal = _loop_counts(_read(ge.device_asm_path("tinympc_solve_d.hip")), KERNELS["goal"])
    blocks = _loop_blocks(_asm(), BUILTIN)
    rare = [b for b in blocks if any(i.startswith(("global_", "flat_", "buffer_")) for i in b)]
    hot = [b for b in blocks if b not in rare]
    c = collections.Counter(i.split()[0] for b in hot for i in b)
    print("model form, iteration loop: %d blocks (%d rare), %d fused DPP FMAs (goal kernel %d), VALU %d (goal kernel %d), LDS %d (%d)"
          % (len(blocks), len(rare), c["v_fmac_f64_dpp"], goal["v_fmac_f64_dpp"], sum(v for k, v in c.items() if k.startswith("v_")),
             sum(v for k, v in goal.items() if k.startswith("v_")), sum(v for k, v in c.items() if k.startswith("ds_")),
             sum(v for k, v in goal.items() if k.startswith("ds_"))))
    assert goal["v_fmac_f64_dpp"] > 0
    assert c["v_fmac_f64_dpp"] == goal["v_fmac_f64_dpp"], (c["v_fmac_f64_dpp"], goal["v_fmac_f64_dpp"])
    assert c["v_fma_f64"] == goal["v_fma_f64"], (c["v_fma_f64"], goal["v_fma_f64"])
    # (the whole chain count is already there in the blocks that touch no global memory: what a rare block repeats of a step -- the
    # compiler duplicates forward step 0 behind knot 0's stale copy -- is not on the common path)
    # no block of the loop, rare or not, touches scratch
    assert not [i for b in blocks for i in b if i.startswith("scratch_")]
    # the operators are re-read from the wavefront's LDS region once per sweep: 2 x 16 row reads on top of the goal kernel's reads of
    # the slack it keeps in LDS (the model form keeps all 49 knots in registers: fewer LDS instructions, not more)
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


def test_the_plain_translation_unit_has_no_symbol_of_the_model_kernel():
    text = _read(ge.device_asm_path("tinympc_solve_d.hip"))
    assert BUILTIN not in text and "k_builtin" not in text
    assert BUILTIN in _asm()
