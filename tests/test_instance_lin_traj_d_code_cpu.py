"""Static checks of layout D's compiled-in kernel for per-instance linear rows on per-instance trajectories (quadrotor nx=12 nu=4 N=20,
one row per side: tinympc_solve_d.hip with -DTINY_JIT_FAM=1 -DTINY_JIT_IGOAL=1 -DTINY_JIT_ILIN=1 -DTINY_JIT_ITRAJ=1,
__graft_entry__.HIP_BUILTINS_D) in the build's gfx950 assembly, beside the form it extends (k_builtin_d_quadrotor20_lin1).

The combined form changes where the backward sweep's linref comes from -- a read of the wavefront's own rows in LDS, one per slot, issued
a block ahead, where the goal form holds one lane constant -- and nothing of the arithmetic: the families' term is added to the read as
it is added to the constant, the accumulator start is the families' own sum and select. So its iteration loop holds exactly the lin1
loop's floating-point instructions of every kind (and one select that lin1 hoists out of its loop), and NS 64-bit LDS reads more, one
per slot: the two of the sweep's head (slots NS-1, NS-2), the first block's (NS-3) and one per block from NS-1 down to 3 (slots NS-4 ..
0; blocks 2 and 1 both use slot 0's, so their sums are formed once, as on the goal form's constant). No LDS write more, no global load,
no scratch; one wavefront per SIMD without spills."""
from __future__ import annotations

import collections
import re

import __graft_entry__ as ge
from test_instance_lin_d_code_cpu import BUILTIN as LIN1
from test_instance_lin_d_code_cpu import NS, NXU, _read
from test_instance_models_d_code_cpu import _loop_blocks
from test_layout_d_fold_code_cpu import _metadata

BUILTIN = "k_builtin_d_quadrotor20_lin1_traj"
MEM = ("global_", "flat_", "buffer_")
FP64 = ("v_fmac_f64_dpp", "v_fma_f64", "v_add_f64", "v_mul_f64", "v_max_f64", "v_min_f64", "v_rcp_f64", "v_div_scale_f64", "v_div_fmas_f64",
        "v_div_fixup_f64", "v_cmp_")


def _asm(name=BUILTIN):
    return _read(ge.builtin_asm_path(name))


def _hot(name):
    blocks = _loop_blocks(_asm(name), name)
    rare = [b for b in blocks if any(i.startswith(MEM) for i in b)]
    hot = [b for b in blocks if b not in rare]
    return blocks, rare, collections.Counter(i.split()[0] for b in hot for i in b)


def _lds_bytes(name):
    m = re.search(r"\.amdhsa_kernel %s\b.*?\.amdhsa_group_segment_fixed_size (\d+)" % re.escape(name), _asm(name), re.S)
    assert m, name
    return int(m.group(1))


def _kind(counter, prefix):
    return sum(v for k, v in counter.items() if k.startswith(prefix))


def test_the_kernel_is_registered_with_the_options_of_its_plan():
    entry = [e for e in ge.HIP_BUILTINS_D if e[0] == BUILTIN]
    assert entry and entry[0] in ge.ALL_BUILTINS  # (what the build compiles, registers and lints)
    assert len(entry) == 1 and entry[0][1] == "tinympc_solve_d.hip"
    lin1 = [e for e in ge.HIP_BUILTINS_D if e[0] == LIN1][0][2]
    assert entry[0][2] == lin1 + ["-DTINY_JIT_ITRAJ=1"], entry[0][2]  # the lin1 form's plan and the trajectory bit


def test_one_wavefront_per_simd_without_spills_or_scratch():
    md, md1 = _metadata(_asm(), BUILTIN), _metadata(_asm(LIN1), LIN1)
    print("linear rows on trajectories:", md, "\nlin1:", md1)
    assert md["vgpr_count"] <= 512, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, md
    # the wavefront's 22 linref rows behind its three row vectors: (N + 2) * 512 B for each of the workgroup's four wavefronts
    lds, lds1 = _lds_bytes(BUILTIN), _lds_bytes(LIN1)
    print("LDS bytes per workgroup:", lds, "lin1:", lds1)
    assert lds == lds1 + 4 * (NS + 3) * 512 == 65024, (lds, lds1)


def test_the_iteration_loop_is_the_lin1_loop_with_one_more_lds_read_per_linref():
    blocks, rare, c = _hot(BUILTIN)
    blocks1, rare1, c1 = _hot(LIN1)
    print("linear rows on trajectories, iteration loop: %d blocks (%d rare; lin1 %d, %d), fused DPP FMAs %d (%d), VALU %d (%d), "
          "LDS reads %d (%d), LDS writes %d (%d)"
          % (len(blocks), len(rare), len(blocks1), len(rare1), c["v_fmac_f64_dpp"], c1["v_fmac_f64_dpp"], _kind(c, "v_"), _kind(c1, "v_"),
             _kind(c, "ds_read"), _kind(c1, "ds_read"), _kind(c, "ds_write"), _kind(c1, "ds_write")))
    for k in sorted(set(c) | set(c1)):
        if c[k] != c1[k]:
            print("  differs: %-24s %d (lin1 %d)" % (k, c[k], c1[k]))
    # no block of the loop, rare or not, touches scratch; nothing in it loads from global memory (both blocks of rows were staged in front)
    assert not [i for b in blocks for i in b if i.startswith("scratch_")]
    assert not [i for b in blocks for i in b if i.startswith(MEM) and ("_load" in i or "atomic" in i)]
    assert rare and all(any("_store" in i for i in b if i.startswith(MEM)) for b in rare)
    # the chain: both sweeps' fused DPP FMAs and the families' mat-vecs, as many as lin1's loop has
    assert c["v_fmac_f64_dpp"] == c1["v_fmac_f64_dpp"] >= 2 * NS * NXU - 12, (c["v_fmac_f64_dpp"], c1["v_fmac_f64_dpp"])
    # ... and every other kind of floating-point work, comparisons and selects included
    for k in FP64:
        assert _kind(c, k) == _kind(c1, k), (k, _kind(c, k), _kind(c1, k))
    # ... but one 64-bit select (two v_cndmask_b32): the head's lane choice between pNref and the last slot's row, which lin1 makes once
    # in front of the loop, on two lane constants
    assert _kind(c, "v_cndmask_b32") == _kind(c1, "v_cndmask_b32") + 2, (_kind(c, "v_cndmask_b32"), _kind(c1, "v_cndmask_b32"))
    # what is new: one 64-bit LDS read per linref (see the module docstring), and no write
    assert _kind(c, "ds_read") == _kind(c1, "ds_read") + NS, (_kind(c, "ds_read"), _kind(c1, "ds_read"))
    assert c["ds_read_b64"] == c1["ds_read_b64"] + NS
    assert _kind(c, "ds_write") == _kind(c1, "ds_write")
    # the loop's other LDS and memory instruction kinds are lin1's
    for k in set(c) | set(c1):
        if k.startswith(("ds_", "global_", "flat_", "buffer_", "s_barrier")) and k != "ds_read_b64":
            assert c[k] == c1[k], (k, c[k], c1[k])


def test_the_linked_form_passes_the_builds_lints():
    """The DPP-hazard lint and the in-flight lint of the build, on the assembly of the form that was linked (bare chain blocks unless the
    build had to fall back to the guarded ones)."""
    from tools.inflight_lint import lint as inflight_lint
    from tools.isa_lint import lint_file
    path = ge.builtin_asm_path(BUILTIN)
    _read(path)
    checked, bad = lint_file(path)
    assert checked >= 2 * NS * NXU - 12 and not bad, (checked, bad[:3])
    assert not inflight_lint(path)


def test_the_plain_translation_unit_has_no_symbol_of_the_kernel():
    text = _read(ge.device_asm_path("tinympc_solve_d.hip"))
    assert BUILTIN not in text and "k_builtin" not in text
    assert BUILTIN in _asm()
