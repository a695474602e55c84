"""Static checks of layout D's trimmed lean kernels (tinympc_ltrim_d.hip = tinympc_solve_d.hip with TINY_LEAN, TINY_LEAN_START and
TINY_LEAN_TRIM) in the build's gfx950 assembly; the parsing is test_layout_d_lean_start_code_cpu.py's.

The variant takes instructions that are not arithmetic out of the lean inner loop and must leave the arithmetic alone: the same 1,556
fused DPP FMAs and 50 `v_fma_f64` per wavefront-iteration as the lean-start kernels, no more VALU instructions than their 1,862, no more
LDS instructions (213), waits (101) or branches. Of the parts that were built one passed its A/B and is in (docs/NOTEBOOK.md section 15):
the d stores of a lean round go through a per-lane address, so the 49 `s_and_saveexec_b64` / `s_mov_b64 exec` pairs around them are gone
(what the build has: 0 and 2 `s_mov_b64`, 1,860 VALU -- the ballot behind the stores' mask left the loop as well). The part that set the
priority only when it changes did not pass and is not in the source: the loop keeps its `s_memrealtime` and `s_setprio`, and nothing is
asserted about them.

Branches of the parent's lean loop (tinympc_lstart_d.hip), counted on a build of the parent commit with the same compiler: 3 in the
headline kernel (s_cbranch_scc0, s_cbranch_scc1, s_cbranch_vccnz), 3 in its goal form. `s_and_saveexec_b64` there: 49."""
from __future__ import annotations

import collections
import json
import os
import re

import pytest

import __graft_entry__ as ge
from test_layout_d_lean_start_code_cpu import GLOBAL, _lean_loop, _metadata
from tools.headline_code_hash import (KERNEL, KERNEL_LEAN, KERNEL_LEAN_START, KERNEL_LEAN_TRIM, RECORD, RECORD_LEAN, RECORD_LEAN_START,
                                      RECORD_LEAN_TRIM, SOURCE_LEAN, SOURCE_LEAN_START, SOURCE_LEAN_TRIM, current_hash)

KERNELS = {  # the quadrotor N=50 kernel (what the headline runs) and its per-instance goal form
    "headline": KERNEL_LEAN_TRIM,
    "goal": "_ZN7tinympc29k_admm_solve_d_gbnd_lean_trimILi12ELi4ELi50ELi4ELi25EEEvNS_11SolveParamsE",
}
PARENT_BRANCHES = {"headline": 3, "goal": 3}  # (see the module's docstring)
PARENT_LDS, PARENT_WAITS = 213, 101
ALL_TRIM = r"_ZN7tinympc\d+k_admm_solve_d(?:_gbnd)?_lean_trimI\w+"


def _asm(source=SOURCE_LEAN_TRIM):
    path = ge.device_asm_path(source)
    if not os.path.exists(path):
        pytest.skip("no build assembly (run __graft_entry__.build())")
    return open(path).read()


@pytest.mark.parametrize("which", list(KERNELS))
def test_the_lean_loop_keeps_its_arithmetic(which):
    c, blocks = _lean_loop(_asm(), KERNELS[which])
    assert c["v_fmac_f64_dpp"] == 1556, c["v_fmac_f64_dpp"]
    assert c["v_fma_f64"] == 50, c["v_fma_f64"]
    movs = sum(v for k, v in c.items() if k.startswith("v_mov_b64"))
    valu = sum(v for k, v in c.items() if k.startswith("v_"))
    print(which, "lean loop: VALU", valu, "v_mov_b64*", movs)
    assert valu <= 1862, valu
    assert movs <= 2, movs
    assert not [i for b in blocks for i in b if i.startswith("scratch_")]
    assert not [i for b in blocks for i in b if i.startswith(GLOBAL)]


@pytest.mark.parametrize("which", list(KERNELS))
def test_the_lean_loop_has_lost_the_exec_round_trips_and_gained_nothing(which):
    c, blocks = _lean_loop(_asm(), KERNELS[which])
    lds = sum(v for k, v in c.items() if k.startswith("ds_"))
    branches = [i for b in blocks for i in b if re.match(r"s_c?branch", i)]
    print(which, "lean loop: s_and_saveexec_b64", c["s_and_saveexec_b64"], "s_mov_b64", c["s_mov_b64"], "LDS", lds, "s_waitcnt", c["s_waitcnt"],
          "branches", collections.Counter(i.split()[0] for i in branches))
    assert c["s_and_saveexec_b64"] <= 2, c["s_and_saveexec_b64"]  # (49 in the parent: one around every d store)
    assert not [i for b in blocks for i in b if re.match(r"s_mov_b64\s+exec\b", i)]
    assert lds <= PARENT_LDS, lds
    assert c["ds_write_b64"] == 49 + 25, c["ds_write_b64"]  # (every d store and every LDS slack slot, one instruction each)
    assert c["s_waitcnt"] <= PARENT_WAITS, c["s_waitcnt"]
    assert len(branches) <= PARENT_BRANCHES[which], branches


def test_every_kernel_of_the_unit_runs_two_wavefronts_per_simd_without_scratch():
    text = _asm()
    names = sorted(set(re.findall(r"^\s+\.name:\s+(%s)$" % ALL_TRIM, text, re.M)))
    assert KERNELS["headline"] in names and KERNELS["goal"] in names and len(names) == 8, names  # (three shapes: 2 + 3 + 3 kernels)
    for k in names:
        md = _metadata(text, k)
        assert md["vgpr_count"] <= 256, (k, md)
        assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, (k, md)


def test_the_unit_holds_only_its_own_symbols_and_the_other_units_keep_their_code():
    """The variant is textual: the plain, the lean and the lean-start translation units have none of its symbols and still have their
    recorded hashes."""
    for source in ("tinympc_solve_d.hip", SOURCE_LEAN, SOURCE_LEAN_START):
        assert "_lean_trim" not in _asm(source), source
    assert not re.search(r"k_admm_solve_d(?:_gbnd)?(?:_lean)?(?:_start)?I", _asm())
    for kernel, source, record in ((KERNEL, "tinympc_solve_d.hip", RECORD), (KERNEL_LEAN, SOURCE_LEAN, RECORD_LEAN),
                                   (KERNEL_LEAN_START, SOURCE_LEAN_START, RECORD_LEAN_START)):
        want, got = json.load(open(record)), current_hash(kernel, source)
        if got["compiler"] != want["compiler"]:
            pytest.skip(f"another compiler ({got['compiler']} against {want['compiler']}): the recorded hash does not apply")
        assert got["sha256"] == want["sha256"], (kernel, got)


def test_the_headline_kernel_is_the_code_that_was_measured():
    want = json.load(open(RECORD_LEAN_TRIM))
    got = current_hash(KERNEL_LEAN_TRIM, SOURCE_LEAN_TRIM)
    if got is None:
        pytest.skip("no build assembly (run __graft_entry__.build())")
    if got["compiler"] != want["compiler"]:
        pytest.skip(f"another compiler ({got['compiler']} against {want['compiler']}): the recorded hash does not apply")
    assert got["sha256"] == want["sha256"], (
        f"the headline kernel's code changed ({got['instructions']} instructions, recorded {want['instructions']}): A/B the builds with "
        f"tools/headline_ab.py on one box, then `python tools/headline_code_hash.py --record-lean-trim` (recorded state: {want['measured']})")
