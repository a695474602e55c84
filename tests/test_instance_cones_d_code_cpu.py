"""Static checks of layout D's compiled-in per-instance families kernel for the rocket landing (nx=6 nu=3 N=10, slopes per instance and
one state row: tinympc_solve_d.hip with -DTINY_JIT_FAM=1 -DTINY_JIT_IGOAL=1 -DTINY_JIT_ILIN=1 -DTINY_JIT_ICONE=1, __graft_entry__.HIP_BUILTINS_D) in the
build's gfx950 assembly.

The form reads the cone slope of the lane's own instance (tinympc_set_cone_slopes_batch) ONCE, in front of the iteration loop, beside
the rows its wavefront stages into LDS: the loop must read no global memory at all, store to it only in the rare write-back /
stale-copy blocks (the block rule of test_instance_lin_d_code_cpu.py), touch scratch nowhere, and fit the one-wavefront-per-SIMD plan
without spills."""
from __future__ import annotations

import collections
import os

import pytest

import __graft_entry__ as ge
from test_instance_models_d_code_cpu import _loop_blocks
from test_layout_d_fold_code_cpu import _metadata

BUILTIN = "k_builtin_d_rocket10_cones"
NS, NXU = 9, 9  # slots of the horizon, rows of the system: a sweep step's chain has at least one fused FMA per row


def _read(path):
    if not os.path.exists(path):
        pytest.skip("no build assembly (run __graft_entry__.build())")
    return open(path).read()


def _asm():
    return _read(ge.builtin_asm_path(BUILTIN))


def test_the_kernel_is_registered_with_the_options_of_its_plan():
    entry = [e for e in ge.HIP_BUILTINS_D if e[0] == BUILTIN]
    assert entry and entry[0] in ge.ALL_BUILTINS  # (what the build compiles, registers and lints)
    assert len(entry) == 1 and entry[0][1] == "tinympc_solve_d.hip"
    names = [e[0] for e in ge.HIP_BUILTINS_D]
    assert names.index(BUILTIN) == names.index("k_builtin_d_quadrotor20_lin1") + 1  # (beside the row mode's kernel)
    defs = entry[0][2]
    assert "-DTINY_JIT_ICONE=1" in defs and "-DTINY_JIT_ILIN=1" in defs and "-DTINY_JIT_FAM=1" in defs and "-DTINY_JIT_IGOAL=1" in defs and "-DTINY_JIT_CT=1" in defs, defs
    # the plan of the families at N = 10: one wavefront per SIMD, workgroups of four, all 9 slack knots in registers
    assert "-DTINY_JIT_WPS=1" in defs and "-DTINY_JIT_WPG=4" in defs and "-DTINY_JIT_VREG=9" in defs, defs
    assert "-DTINY_JIT_NX=6" in defs and "-DTINY_JIT_NU=3" in defs and "-DTINY_JIT_N=10" in defs, defs


def test_one_wavefront_per_simd_without_spills_or_scratch():
    md = _metadata(_asm(), BUILTIN)
    print("per-instance families form, rocket N=10:", md)
    assert md["vgpr_count"] <= 512, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, md


def test_the_iteration_loop_reads_no_global_memory_and_stores_only_in_its_rare_blocks():
    blocks = _loop_blocks(_asm(), BUILTIN)
    mem = ("global_", "flat_", "buffer_")
    rare = [b for b in blocks if any(i.startswith(mem) for i in b)]
    hot = [b for b in blocks if b not in rare]
    c = collections.Counter(i.split()[0] for b in hot for i in b)
    print("per-instance families form, iteration loop: %d blocks (%d rare), %d fused DPP FMAs, VALU %d, LDS reads %d, LDS writes %d"
          % (len(blocks), len(rare), c["v_fmac_f64_dpp"], sum(v for k, v in c.items() if k.startswith("v_")),
             sum(v for k, v in c.items() if k.startswith("ds_read")), sum(v for k, v in c.items() if k.startswith("ds_write"))))
    assert not [i for b in blocks for i in b if i.startswith("scratch_")]
    # nothing in the loop LOADS from global memory: the slope was loaded, the rows staged into LDS, in front of it
    loads = [i for b in blocks for i in b if i.startswith(mem) and ("_load" in i or "atomic" in i)]
    assert not loads, loads[:3]
    assert rare and all(any("_store" in i for i in b if i.startswith(mem)) for b in rare)
    assert c["v_fmac_f64_dpp"] >= 2 * NS * NXU - 12, c["v_fmac_f64_dpp"]
    assert sum(v for k, v in c.items() if k.startswith("ds_read")) > 0  # (the row comes from LDS)


def test_the_linked_form_passes_the_builds_lints():
    from tools.inflight_lint import lint as inflight_lint
    from tools.isa_lint import lint_file
    path = ge.builtin_asm_path(BUILTIN)
    _read(path)
    checked, bad = lint_file(path)
    assert checked >= 2 * NS * NXU - 12 and not bad, (checked, bad[:3])
    assert not inflight_lint(path)
