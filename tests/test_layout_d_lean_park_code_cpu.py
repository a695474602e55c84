"""Static checks of layout D's lean kernels with a slot split of their own inside a run of lean rounds (tinympc_lpark_d.hip =
tinympc_solve_d.hip with TINY_LEAN, TINY_LEAN_START, TINY_LEAN_TRIM, TINY_LEAN_SHARE and TINY_LEAN_PARK) in the build's gfx950 assembly;
the parsing is test_layout_d_lean_start_code_cpu.py's.

The variant moves no arithmetic: the shared round -- the kernel's hot loop -- keeps the parent's 1,860 VALU instructions per
wavefront-round (1,556 fused DPP FMAs, 50 `v_fma_f64`, one `v_mov_b64*`), and each of the k = VL - VLR LDS slots that is a register slot
inside a run takes four LDS instructions out of it: the slack's store and d's read going forward, the slack's read and d's store going
backward. The parent's loop has 165 LDS instructions, 50 of them `ds_write_b64`; k >= 12 is the condition the change was accepted
under (48 instructions: the smallest step the A/B of docs/NOTEBOOK.md section 18 has resolved).

The registers of the converted slots are the ones the parent's loop left idle, so the kernel stays within 256 VGPRs without scratch:
what lived in them across a run is parked in LDS or rebuilt behind the run (the table is in docs/NOTEBOOK.md section 21)."""
from __future__ import annotations

import json
import os
import re

import pytest

import __graft_entry__ as ge
from test_layout_d_lean_start_code_cpu import GLOBAL, _lean_loop, _metadata
from tools.headline_code_hash import (KERNEL, KERNEL_LEAN, KERNEL_LEAN_PARK, KERNEL_LEAN_SHARE, KERNEL_LEAN_START, KERNEL_LEAN_TRIM, RECORD,
                                      RECORD_LEAN, RECORD_LEAN_PARK, RECORD_LEAN_SHARE, RECORD_LEAN_START, RECORD_LEAN_TRIM, SOURCE_LEAN,
                                      SOURCE_LEAN_PARK, SOURCE_LEAN_SHARE, SOURCE_LEAN_START, SOURCE_LEAN_TRIM, current_hash)

KERNELS = {  # the quadrotor N=50 kernel (what the headline runs) and its per-instance goal form: the unit's only kernels
    "headline": KERNEL_LEAN_PARK,
    "goal": "_ZN7tinympc29k_admm_solve_d_gbnd_lean_parkILi12ELi4ELi50ELi4ELi25EEEvNS_11SolveParamsE",
}
PARENTS = {  # the same two kernels of tinympc_lshare_d.hip
    "headline": KERNEL_LEAN_SHARE,
    "goal": "_ZN7tinympc30k_admm_solve_d_gbnd_lean_shareILi12ELi4ELi50ELi4ELi25EEEvNS_11SolveParamsE",
}
PARENT_VALU, PARENT_WAITS = 1860, 101 # (the shared loop of tinympc_lshare_d.hip: test_layout_d_lean_share_code_cpu.py)
PARENT_LDS, PARENT_WRITES = 165, 50
K_MIN = 12                             # (converted slots: the condition)
ALL_PARK = r"_ZN7tinympc\d+k_admm_solve_d(?:_gbnd)?_lean_parkI\w+"


def _asm(source=SOURCE_LEAN_PARK):
    path = ge.device_asm_path(source)
    if not os.path.exists(path):
        pytest.skip("no build assembly (run __graft_entry__.build())")
    return open(path).read()


def _loop_bytes(blocks):
    # (every VALU instruction of the loop is 8 bytes -- VOP3 or DPP64 --, every LDS instruction 8, the scalar ones 4; the assembler's
    # padding s_nop, at most one per chain block, are not in the compiler's text and are counted at their maximum)
    return sum(4 if i.startswith("s_") else 8 for b in blocks for i in b) + 4 * 98


def _converted_slots():
    """k, from the source: the unit's constant (the kernels' VL is 25)."""
    text = open(os.path.join(ge.CSRC, "tinympc_solve_d.hip")).read()
    return int(re.search(r"^#define TINY_PARK_SLOTS (\d+)", text, re.M).group(1))


@pytest.mark.parametrize("which", list(KERNELS))
def test_the_loop_has_the_parents_arithmetic(which):
    c, blocks = _lean_loop(_asm(), KERNELS[which])
    assert c["v_fmac_f64_dpp"] == 1556, c["v_fmac_f64_dpp"]
    assert c["v_fma_f64"] == 50, c["v_fma_f64"]
    movs = sum(v for k, v in c.items() if k.startswith("v_mov_b64"))
    valu = sum(v for k, v in c.items() if k.startswith("v_"))
    print(which, "loop: VALU", valu, "v_mov_b64*", movs)
    assert valu == PARENT_VALU, valu
    assert movs <= 1, movs
    assert not [i for b in blocks for i in b if i.startswith("scratch_")]
    assert not [i for b in blocks for i in b if i.startswith(GLOBAL)]


@pytest.mark.parametrize("which", list(KERNELS))
def test_every_converted_slot_takes_four_lds_instructions_out_of_the_loop(which):
    k = _converted_slots()
    assert k >= K_MIN, k
    c, blocks = _lean_loop(_asm(), KERNELS[which])
    _, parent_blocks = _lean_loop(_asm(SOURCE_LEAN_SHARE), PARENTS[which])
    lds = sum(v for n, v in c.items() if n.startswith("ds_"))
    size, parent_size = _loop_bytes(blocks), _loop_bytes(parent_blocks)
    print(which, "k", k, "loop: LDS", lds, "ds_write_b64", c["ds_write_b64"], "ds_read*", lds - c["ds_write_b64"], "s_waitcnt", c["s_waitcnt"], "s_nop", c["s_nop"],
          "bytes <=", size, "parent", parent_size)
    assert lds == PARENT_LDS - 4 * k, lds
    assert c["ds_write_b64"] == PARENT_WRITES - 2 * k, c["ds_write_b64"]
    assert c["s_waitcnt"] <= PARENT_WAITS, c["s_waitcnt"]
    assert size <= parent_size, (size, parent_size)


def test_the_units_two_kernels_run_two_wavefronts_per_simd_without_scratch():
    text = _asm()
    names = sorted(set(re.findall(r"^\s+\.name:\s+(%s)$" % ALL_PARK, text, re.M)))
    assert names == sorted(KERNELS.values()), names  # (the one shape with LDS slots: the shared-table and the goal form)
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
    """The variant is textual: the plain, the lean, the lean-start, the trimmed and the shared translation units have none of its symbols
    and still have their recorded hashes."""
    for source in ("tinympc_solve_d.hip", SOURCE_LEAN, SOURCE_LEAN_START, SOURCE_LEAN_TRIM, SOURCE_LEAN_SHARE):
        assert "_lean_park" not in _asm(source), source
    assert not re.search(r"k_admm_solve_d(?:_gbnd)?(?:_lean)?(?:_start)?(?:_trim)?(?:_share)?I", _asm())
    for kernel, source, record in ((KERNEL, "tinympc_solve_d.hip", RECORD), (KERNEL_LEAN, SOURCE_LEAN, RECORD_LEAN),
                                   (KERNEL_LEAN_START, SOURCE_LEAN_START, RECORD_LEAN_START), (KERNEL_LEAN_TRIM, SOURCE_LEAN_TRIM, RECORD_LEAN_TRIM),
                                   (KERNEL_LEAN_SHARE, SOURCE_LEAN_SHARE, RECORD_LEAN_SHARE)):
        want, got = json.load(open(record)), current_hash(kernel, source)
        if got["compiler"] != want["compiler"]:
            pytest.skip(f"another compiler ({got['compiler']} against {want['compiler']}): the recorded hash does not apply")
        assert got["sha256"] == want["sha256"], (kernel, got)


def test_the_headline_kernel_is_the_code_that_was_measured():
    want = json.load(open(RECORD_LEAN_PARK))
    got = current_hash(KERNEL_LEAN_PARK, SOURCE_LEAN_PARK)
    if got is None:
        pytest.skip("no build assembly (run __graft_entry__.build())")
    if got["compiler"] != want["compiler"]:
        pytest.skip(f"another compiler ({got['compiler']} against {want['compiler']}): the recorded hash does not apply")
    assert got["sha256"] == want["sha256"], (
        f"the headline kernel's code changed ({got['instructions']} instructions, recorded {want['instructions']}): A/B the builds with "
        f"tools/headline_ab.py on one box, then `python tools/headline_code_hash.py --record-lean-park` (recorded state: {want['measured']})")
