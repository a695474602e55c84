"""Static checks of layout D's compiled-in per-knot linear-row kernel (quadrotor nx=12 nu=4 N=20, one row per side at every knot:
tinympc_solve_d.hip with -DTINY_JIT_FAM=1 -DTINY_JIT_IGOAL=1 -DTINY_JIT_ILIN=1 -DTINY_JIT_IKNOT=1, __graft_entry__.HIP_BUILTINS_D) in the
build's gfx950 assembly.

The form is the per-instance linear-row form (tests/test_instance_lin_d_code_cpu.py) with N slots of rows in the wavefront's LDS region
instead of one: the staging in front of the iteration loop copies more, and a step's three reads per row carry the slot as an immediate
offset. Inside the loop nothing may change -- no load from global memory, stores only in the rare write-back / stale-copy blocks, both
sweeps' whole fused chain in the blocks without any, no scratch, no spills on the one-wavefront-per-SIMD plan. It is a translation unit
of its own: nothing of it reaches tinympc_solve_d.hip's code."""
from __future__ import annotations

import collections
import os
import re

import pytest

import __graft_entry__ as ge
from test_instance_models_d_code_cpu import _loop_blocks
from test_layout_d_fold_code_cpu import _metadata

BUILTIN = "k_builtin_d_quadrotor20_knotlin1"
NS, NXU = 19, 16  # slots of the horizon, chain length of a sweep step


def _read(path):
    if not os.path.exists(path):
        pytest.skip("no build assembly (run __graft_entry__.build())")
    return open(path).read()


def _asm():
    assert [e for e in ge.HIP_BUILTINS_D if e[0] == BUILTIN], "the build does not know " + BUILTIN
    return _read(ge.builtin_asm_path(BUILTIN))


def test_the_kernel_is_registered_once_with_the_options_of_its_plan():
    entry = [e for e in ge.HIP_BUILTINS_D if e[0] == BUILTIN]
    assert len(entry) == 1 and entry[0] in ge.ALL_BUILTINS  # (what the build compiles, registers and lints)
    assert [e[0] for e in ge.ALL_BUILTINS].count(BUILTIN) == 1 and entry[0][1] == "tinympc_solve_d.hip"
    defs = entry[0][2]
    assert "-DTINY_JIT_IKNOT=1" in defs and "-DTINY_JIT_ILIN=1" in defs and "-DTINY_JIT_FAM=1" in defs and "-DTINY_JIT_IGOAL=1" in defs, defs
    assert "-DTINY_JIT_CT=1" in defs and "-DTINY_JIT_ADAPT=0" in defs and "-DTINY_JIT_ICONE=1" not in defs, defs
    # the plan of the families at N = 20: one wavefront per SIMD, workgroups of four, all 19 slack knots in registers
    assert "-DTINY_JIT_WPS=1" in defs and "-DTINY_JIT_WPG=4" in defs and "-DTINY_JIT_VREG=19" in defs, defs
    assert "-DTINY_JIT_NX=12" in defs and "-DTINY_JIT_NU=4" in defs and "-DTINY_JIT_N=20" in defs, defs
    # ... and, but for the form's own define, the options of the constant-row kernel of the same shape, in the specialiser's order
    lin1 = [e for e in ge.HIP_BUILTINS_D if e[0] == "k_builtin_d_quadrotor20_lin1"][0][2]
    assert defs == lin1 + ["-DTINY_JIT_IKNOT=1"], (defs, lin1)


def test_one_wavefront_per_simd_without_spills_or_scratch():
    md = _metadata(_asm(), BUILTIN)
    print("per-knot linear-row form:", md)
    print("per-knot linear-row form: vgpr_count", md["vgpr_count"])
    assert md["vgpr_count"] <= 512, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, md
    # the workgroup's LDS: the shared operators and, per wavefront, d and N slots of three vectors -- 512 + 4 x (304 + 3,840) doubles
    text = _asm()
    i = text.index(".name:           " + BUILTIN)
    lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", text[text.rfind("\n  - ", 0, i):text.find("\n  - ", i)]).group(1))
    assert lds == 8 * (512 + 4 * (304 + 3 * 20 * 64)), lds


def test_the_iteration_loop_reads_no_global_memory_and_stores_only_in_its_rare_blocks():
    blocks = _loop_blocks(_asm(), BUILTIN)
    mem = ("global_", "flat_", "buffer_")
    rare = [b for b in blocks if any(i.startswith(mem) for i in b)]
    hot = [b for b in blocks if b not in rare]
    c = collections.Counter(i.split()[0] for b in hot for i in b)
    print("per-knot linear-row form, iteration loop: %d blocks (%d rare), %d fused DPP FMAs, VALU %d, LDS reads %d, LDS writes %d"
          % (len(blocks), len(rare), c["v_fmac_f64_dpp"], sum(v for k, v in c.items() if k.startswith("v_")),
             sum(v for k, v in c.items() if k.startswith("ds_read")), sum(v for k, v in c.items() if k.startswith("ds_write"))))
    # no block of the loop, rare or not, touches scratch
    assert not [i for b in blocks for i in b if i.startswith("scratch_")]
    # nothing in the loop LOADS from global memory: the slots were staged into LDS, the table constants loaded, in front of it
    loads = [i for b in blocks for i in b if i.startswith(mem) and ("_load" in i or "atomic" in i)]
    assert not loads, loads[:3]
    # ... and what stores there are sit in blocks off the common path: the blocks without any hold both sweeps' chains (forward NS
    # steps, backward NS steps less the folded tail, NXU fused FMAs each) and the families' mat-vecs on top
    assert rare and all(any("_store" in i for i in b if i.startswith(mem)) for b in rare)
    assert c["v_fmac_f64_dpp"] >= 2 * NS * NXU - 12, c["v_fmac_f64_dpp"]
    # the rows come from LDS: three vectors for knot 0 and for each of the NS steps' slots (an instruction reads at most two of them)
    assert sum(v for k, v in c.items() if k.startswith("ds_read")) >= 2 * (NS + 1)


def test_the_linked_form_passes_the_builds_lints():
    """The DPP-hazard lint and the in-flight lint of the build, on the assembly of the form that was linked (bare chain blocks unless the
    build had to fall back to the guarded ones)."""
    from tools.inflight_lint import lint as inflight_lint
    from tools.isa_lint import lint_file
    path = ge.builtin_asm_path(BUILTIN)
    _asm()
    checked, bad = lint_file(path)
    assert checked >= 2 * NS * NXU - 12 and not bad, (checked, bad[:3])
    assert not inflight_lint(path)


def test_the_plain_translation_unit_has_no_symbol_of_the_kernel():
    text = _read(ge.device_asm_path("tinympc_solve_d.hip"))
    assert BUILTIN not in text and "k_builtin" not in text
    assert BUILTIN in _asm()
