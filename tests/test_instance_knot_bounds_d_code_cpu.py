"""Static checks of layout D's compiled-in per-knot bounds kernel (quadrotor nx=12 nu=4 N=20 beside per-instance trajectories:
tinympc_solve_d.hip with -DTINY_JIT_IGOAL=1 -DTINY_JIT_ITRAJ=1 -DTINY_JIT_IKBND=1, __graft_entry__.HIP_BUILTINS_D_KBND) in the build's
gfx950 assembly.

The form changes where the forward sweep's clamp comes from -- the wavefront's own lo and hi rows in LDS, read one step ahead like d,
where the goal form holds two lane constants -- and nothing of the arithmetic: one v_max_f64 / v_min_f64 pair per step on the value read.
Beyond the trajectory form (ITRAJ alone) its iteration loop therefore has two 64-bit LDS reads per forward step, the step's lo and hi
(2 (N - 1) in all: the first step's in front of the sweep, every later one during the step before it), and two for knot 0's clamp,
which the compiler may pair into one ds_read2st64_b64 (lo and hi of one row lie (N + 2) * 512 B apart). The trajectory form's own
count is d and the linref, one each per step, and one more: 2 (N - 1) + 1, which the build's trajectory kernel (quadrotor N=50) shows.
So: 4 (N - 1) + 3 = 79 reads of 64 bits for N=20. No LDS write more, no global load, no scratch; one wavefront per SIMD without
spills, 148,992 B of LDS per workgroup."""
from __future__ import annotations

import collections
import os
import re

import __graft_entry__ as ge
from test_instance_knot_bounds_plan_cpu import BUILTIN, first_fit, kbnd_plan
from test_instance_models_d_code_cpu import _loop_blocks, _read
from test_instance_traj_d_code_cpu import BUILTIN as TRAJ50
from test_layout_d_fold_code_cpu import _metadata

N, NS, NXU = 20, 19, 16
MEM = ("global_", "flat_", "buffer_")


def _asm(name=BUILTIN):
    return _read(ge.builtin_asm_path(name))


def _hot(name):
    blocks = _loop_blocks(_asm(name), name)
    rare = [b for b in blocks if any(i.startswith(MEM) for i in b)]
    hot = [b for b in blocks if b not in rare]
    return blocks, rare, collections.Counter(i.split()[0] for b in hot for i in b)


def _reads64(c):
    """64-bit LDS reads of a loop, a paired read of two 64-bit values counted as two (the operator rows' ds_read2_b64 apart)."""
    return c["ds_read_b64"] + 2 * c["ds_read2st64_b64"]


def test_the_symbol_exists_in_its_own_assembly_only():
    assert re.search(r"\.amdhsa_kernel %s\b" % BUILTIN, _asm())
    text = _read(ge.device_asm_path("tinympc_solve_d.hip"))
    assert BUILTIN not in text and "k_builtin" not in text


def test_one_wavefront_per_simd_without_spills_or_scratch_and_the_planned_lds():
    md = _metadata(_asm(), BUILTIN)
    print("per-knot bounds form:", md)
    assert md["vgpr_count"] <= 512, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, md
    m = re.search(r"\.amdhsa_kernel %s\b.*?\.amdhsa_group_segment_fixed_size (\d+)" % BUILTIN, _asm(), re.S)
    (wps, wpg), lds = first_fit(kbnd_plan(12, 4, N, itraj=True))
    assert (wps, wpg) == (1, 4) and int(m.group(1)) == lds == 148992, (m.group(1), lds)


def test_the_iteration_loop_reads_two_clamp_rows_per_forward_step_and_nothing_else_changes():
    blocks, rare, c = _hot(BUILTIN)
    _, _, t50 = _hot(TRAJ50)
    print("per-knot bounds form, iteration loop: %d blocks (%d rare), fused DPP FMAs %d, v_max_f64 %d, v_min_f64 %d, LDS reads b64 %d, paired %d, "
          "operator rows %d, LDS writes %d; trajectory form N=50: b64 %d"
          % (len(blocks), len(rare), c["v_fmac_f64_dpp"], c["v_max_f64"], c["v_min_f64"], c["ds_read_b64"], c["ds_read2st64_b64"], c["ds_read2_b64"],
             c["ds_write_b64"], t50["ds_read_b64"]))
    # no block of the loop, rare or not, touches scratch; nothing in it loads from global memory (the rows were staged in front)
    assert not [i for b in blocks for i in b if i.startswith("scratch_")]
    assert not [i for b in blocks for i in b if i.startswith(MEM) and ("_load" in i or "atomic" in i)]
    assert rare and all(any("_store" in i for i in b if i.startswith(MEM)) for b in rare)
    # the chain of both sweeps (forward step 0 keeps only its input columns: K0)
    assert c["v_fmac_f64_dpp"] >= 2 * NS * NXU - 12, c["v_fmac_f64_dpp"]
    # one clamp per forward step and knot 0's: as many v_min_f64 as the trajectory form has per knot
    assert c["v_min_f64"] == N and t50["v_min_f64"] == 50, (c["v_min_f64"], t50["v_min_f64"])
    # the trajectory form's reads: d and the linref per step, and one more
    assert _reads64(t50) == t50["ds_read_b64"] == 2 * 49 + 1, t50
    # ... and here lo and hi per forward step and knot 0's pair beyond that
    assert _reads64(c) == (2 * NS + 1) + 2 * NS + 2, (c["ds_read_b64"], c["ds_read2st64_b64"])
    # the operator rows' reads and the LDS writes (d of every backward step) are the trajectory form's
    assert c["ds_read2_b64"] == t50["ds_read2_b64"]
    assert c["ds_write_b64"] == NS and t50["ds_write_b64"] == 49
    for k in c:
        if k.startswith("ds_"):
            assert k in ("ds_read_b64", "ds_read2_b64", "ds_read2st64_b64", "ds_write_b64"), k


def test_the_build_compiled_registered_and_linted_it_like_its_siblings():
    """The DPP-hazard lint and the in-flight lint of the build, on the assembly of the form that was linked (bare chain blocks unless the
    build had to fall back to the guarded ones) -- build_hip() runs both over ALL_BUILTINS and fails on a finding."""
    from tools.inflight_lint import lint as inflight_lint
    from tools.isa_lint import lint_file
    assert [e[0] for e in ge.ALL_BUILTINS].count(BUILTIN) == 1
    path = ge.builtin_asm_path(BUILTIN)
    _read(path)
    checked, bad = lint_file(path)
    assert checked >= 2 * NS * NXU - 12 and not bad, (checked, bad[:3])
    assert not inflight_lint(path)
    registry = _read(os.path.join(ge.BUILD_DIR, "tinympc_builtin_registry.inc"))
    assert '"%s"' % BUILTIN in registry and "-DTINY_JIT_ITRAJ=1 -DTINY_JIT_IKBND=1" in registry
