"""Static checks of layout D's lean kernels with d and the slack sharing the register slots (tinympc_lshare_d.hip = tinympc_solve_d.hip
with TINY_LEAN, TINY_LEAN_START, TINY_LEAN_TRIM and TINY_LEAN_SHARE) in the build's gfx950 assembly; the parsing is
test_layout_d_lean_start_code_cpu.py's.

The variant moves no arithmetic: the shared round -- the kernel's hot loop, a run's rounds but the last -- has the parent's 1,860 VALU
instructions per wavefront-round (1,556 fused DPP FMAs, 50 `v_fma_f64`, one `v_mov_b64*`: step 0's start from c0; no difference to
state), and of the parent's 213 LDS instructions the 24 `ds_write_b64` and 24 `ds_read_b64` that carried d_s of the register slots
from the backward to the next forward sweep are gone: 165.

`s_waitcnt`: 101, the parent's. The plan asked for fewer unless the unit is built with -DTINY_SHARE_KEEP_WAITS. The form without the
waits of the twenty backward blocks that have no LDS instruction around them was built and measured (80 waits): the compiler puts an
`s_nop 0` of its own between two asm statements with nothing in between, the block trades its wait for a nop, and the round medians of
the two builds overlapped in both A/B pairs (docs/NOTEBOOK.md section 18). A part that fails the bar stays out of the source, so what is
built is what that switch would have built, the switch is gone with the part, and the assertion here is "no more than the parent".

The kernel has a second round body behind the loop (the last round of a run: shared forward sweep, the trimmed kernels' backward sweep);
what `_lean_loop` finds is the loop."""
from __future__ import annotations

import json
import os
import re

import pytest

import __graft_entry__ as ge
from test_layout_d_lean_start_code_cpu import GLOBAL, _lean_loop, _metadata
from tools.headline_code_hash import (KERNEL, KERNEL_LEAN, KERNEL_LEAN_SHARE, KERNEL_LEAN_START, KERNEL_LEAN_TRIM, RECORD, RECORD_LEAN,
                                      RECORD_LEAN_SHARE, RECORD_LEAN_START, RECORD_LEAN_TRIM, SOURCE_LEAN, SOURCE_LEAN_SHARE, SOURCE_LEAN_START,
                                      SOURCE_LEAN_TRIM, current_hash)

KERNELS = {  # the quadrotor N=50 kernel (what the headline runs) and its per-instance goal form
    "headline": KERNEL_LEAN_SHARE,
    "goal": "_ZN7tinympc30k_admm_solve_d_gbnd_lean_shareILi12ELi4ELi50ELi4ELi25EEEvNS_11SolveParamsE",
}
PARENT_VALU, PARENT_WAITS = 1860, 101  # (the lean loop of tinympc_ltrim_d.hip: test_layout_d_lean_trim_code_cpu.py)
SHARED_LDS = 165                      # (its 213 less the 24 stores and 24 reads of d_s of the register slots)
PARENT_LOOP_BYTES = 17400             # (the parent's lean loop, 17.4 KB)
ALL_SHARE = r"_ZN7tinympc\d+k_admm_solve_d(?:_gbnd)?_lean_shareI\w+"


def _asm(source=SOURCE_LEAN_SHARE):
    path = ge.device_asm_path(source)
    if not os.path.exists(path):
        pytest.skip("no build assembly (run __graft_entry__.build())")
    return open(path).read()


@pytest.mark.parametrize("which", list(KERNELS))
def test_the_shared_loop_has_the_parents_arithmetic(which):
    c, blocks = _lean_loop(_asm(), KERNELS[which])
    assert c["v_fmac_f64_dpp"] == 1556, c["v_fmac_f64_dpp"]
    assert c["v_fma_f64"] == 50, c["v_fma_f64"]
    movs = sum(v for k, v in c.items() if k.startswith("v_mov_b64"))
    valu = sum(v for k, v in c.items() if k.startswith("v_"))
    print(which, "shared loop: VALU", valu, "v_mov_b64*", movs)
    assert valu == PARENT_VALU, valu
    assert movs <= 1, movs
    assert not [i for b in blocks for i in b if i.startswith("scratch_")]
    assert not [i for b in blocks for i in b if i.startswith(GLOBAL)]


@pytest.mark.parametrize("which", list(KERNELS))
def test_the_shared_loop_has_lost_the_lds_round_trip_of_the_register_slots(which):
    c, blocks = _lean_loop(_asm(), KERNELS[which])
    lds = sum(v for k, v in c.items() if k.startswith("ds_"))
    # (bytes: every VALU instruction of the loop is 8 bytes -- VOP3 or DPP64 --, every LDS instruction 8, the scalar ones 4; the
    # assembler's padding s_nop, at most one per chain block, are not in the compiler's text and are counted at their maximum)
    size = sum(4 if i.startswith("s_") else 8 for b in blocks for i in b) + 4 * 98
    print(which, "shared loop: LDS", lds, "ds_write_b64", c["ds_write_b64"], "ds_read*", lds - c["ds_write_b64"], "s_waitcnt", c["s_waitcnt"],
          "s_nop", c["s_nop"], "bytes <=", size)
    assert lds <= SHARED_LDS, lds
    assert c["ds_write_b64"] == 25 + 25, c["ds_write_b64"]  # (d_s and the slack of the 25 LDS slots, one instruction each)
    assert c["s_waitcnt"] <= PARENT_WAITS, c["s_waitcnt"]  # (see the module's docstring)
    assert size <= PARENT_LOOP_BYTES, size


def test_every_kernel_of_the_unit_runs_two_wavefronts_per_simd_without_scratch():
    text = _asm()
    names = sorted(set(re.findall(r"^\s+\.name:\s+(%s)$" % ALL_SHARE, text, re.M)))
    assert KERNELS["headline"] in names and KERNELS["goal"] in names and len(names) == 8, names  # (three shapes: 2 + 3 + 3 kernels)
    for k in names:
        md = _metadata(text, k)
        assert md["vgpr_count"] <= 256, (k, md)
        assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, (k, md)
        m = re.search(r"^%s:(.*?)^\.Lfunc_end" % re.escape(k), text, re.S | re.M)
        assert "scratch_" not in m.group(1), k


def test_every_chain_of_the_unit_starts_on_the_8_byte_grid():
    """Every fused DPP chain is the text of one asm block, and every block opens with `.p2align 3` (the instructions of a chain are 8
    bytes each): in the compiler's assembly the first DPP FMA of a run of them follows the directive directly."""
    text = _asm()
    for k in KERNELS.values():
        m = re.search(r"^%s:(.*?)^\.Lfunc_end" % re.escape(k), text, re.S | re.M)
        lines = [x.split(";")[0].strip() for x in m.group(1).split("\n")]
        lines = [x for x in lines if x and not x.startswith(("//", "#"))]
        chains = off_grid = 0
        for prev, cur in zip(lines, lines[1:]):
            if cur.startswith("v_fmac_f64_dpp") and not prev.startswith("v_fmac_f64_dpp"):
                chains += 1
                off_grid += prev != ".p2align\t3" and prev != ".p2align 3"
        assert chains >= 3 * 98 and off_grid == 0, (k, chains, off_grid)


def test_the_unit_holds_only_its_own_symbols_and_the_other_units_keep_their_code():
    """The variant is textual: the plain, the lean, the lean-start and the trimmed translation units have none of its symbols and still
    have their recorded hashes."""
    for source in ("tinympc_solve_d.hip", SOURCE_LEAN, SOURCE_LEAN_START, SOURCE_LEAN_TRIM):
        assert "_lean_share" not in _asm(source), source
    assert not re.search(r"k_admm_solve_d(?:_gbnd)?(?:_lean)?(?:_start)?(?:_trim)?I", _asm())
    for kernel, source, record in ((KERNEL, "tinympc_solve_d.hip", RECORD), (KERNEL_LEAN, SOURCE_LEAN, RECORD_LEAN),
                                   (KERNEL_LEAN_START, SOURCE_LEAN_START, RECORD_LEAN_START), (KERNEL_LEAN_TRIM, SOURCE_LEAN_TRIM, RECORD_LEAN_TRIM)):
        want, got = json.load(open(record)), current_hash(kernel, source)
        if got["compiler"] != want["compiler"]:
            pytest.skip(f"another compiler ({got['compiler']} against {want['compiler']}): the recorded hash does not apply")
        assert got["sha256"] == want["sha256"], (kernel, got)


def test_the_headline_kernel_is_the_code_that_was_measured():
    want = json.load(open(RECORD_LEAN_SHARE))
    got = current_hash(KERNEL_LEAN_SHARE, SOURCE_LEAN_SHARE)
    if got is None:
        pytest.skip("no build assembly (run __graft_entry__.build())")
    if got["compiler"] != want["compiler"]:
        pytest.skip(f"another compiler ({got['compiler']} against {want['compiler']}): the recorded hash does not apply")
    assert got["sha256"] == want["sha256"], (
        f"the headline kernel's code changed ({got['instructions']} instructions, recorded {want['instructions']}): A/B the builds with "
        f"tools/headline_ab.py on one box, then `python tools/headline_code_hash.py --record-lean-share` (recorded state: {want['measured']})")
