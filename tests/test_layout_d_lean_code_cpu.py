"""Static checks of layout D's lean kernels (tinympc_lean_d.hip = tinympc_solve_d.hip with TINY_LEAN) in the build's gfx950 assembly.

An iteration whose residuals nothing can read (no termination check falls on it, or the tolerances cannot be met and a later check
overwrites its snapshot) runs a forward sweep without the residual maxima: per forward step `mov + 16 FMAs + 4` instead of
`+ 8 (+ 1)`, no read of vold for the slots kept in LDS. The headline (tolerances 0, a check in every iteration) runs 199 of its 200
iterations that way, and it is bound by FP64 VALU issue, so what counts is the number of VALU instructions per wavefront-iteration
of the LEAN LOOP: the innermost loop that holds a forward and a backward sweep (1,556 fused DPP FMAs) and no `v_max_f64` with an
|abs| operand. The plain kernel's loop has 2,176; the bound asserted here, 1,960, was derived from that census before anything was
built (2,176 less 49 x 4 residual instructions, the 24 slack hand-over copies and knot 0's two maxima). What the build has: 1,916 VALU,
49 `v_mov_b64*` (the accumulator starts), 165 LDS instructions (190 in the plain loop), in both kernels; measured on the GPU
786.1 M VALU instructions per headline launch against 892.8 M (profiles/d_lean_pmc_valu.json). The lean loop must not touch scratch in
any block (the kernels sit at 254 / 252 of 256 registers with the iteration that keeps the residuals next to the lean loop in the same
function), and the plain kernels must keep their code: a new translation unit, new symbols, the plain kernel's hash still that of its
record.

Rare blocks (write-back: the only blocks of the loop that touch global memory) are left out of the counts, as in
test_layout_d_fold_code_cpu.py."""
from __future__ import annotations

import collections
import json
import os
import re

import pytest
from conftest import ROOT

import __graft_entry__ as ge
from tools.headline_code_hash import KERNEL, KERNEL_LEAN, RECORD, RECORD_LEAN, SOURCE_LEAN, current_hash

KERNELS = {  # the lean quadrotor N=50 kernel (what the headline runs) and its per-instance goal form
    "headline": KERNEL_LEAN,
    "goal": "_ZN7tinympc24k_admm_solve_d_gbnd_leanILi12ELi4ELi50ELi4ELi25EEEvNS_11SolveParamsE",
}
ALL_LEAN = r"_ZN7tinympc\d+k_admm_solve_d(?:_gbnd)?_leanI\w+"


def _asm():
    path = ge.device_asm_path(SOURCE_LEAN)
    if not os.path.exists(path):
        pytest.skip("no build assembly (run __graft_entry__.build())")
    return open(path).read()


def _loops(text: str, kernel: str):
    """Every loop of the kernel (a label and a branch back to it) as a list of basic blocks of instruction lines."""
    m = re.search(r"^%s:(.*?)^\.Lfunc_end" % re.escape(kernel), text, re.S | re.M)
    assert m, kernel
    lines = [x.split(";")[0].rstrip() for x in m.group(1).split("\n")]
    labels, spans = {}, []
    for i, x in enumerate(lines):
        lm = re.match(r"^(\.LBB\d+_\d+):", x)
        if lm:
            labels[lm.group(1)] = i
        bm = re.search(r"\ss_c?branch\w*\s+(\.LBB\d+_\d+)", x)
        if bm and bm.group(1) in labels:
            spans.append((labels[bm.group(1)], i))
    for a, b in spans:
        blocks, cur = [], []
        for x in lines[a:b + 1]:
            if re.match(r"^\.LBB\d+_\d+:", x):
                blocks.append(cur)
                cur = []
            elif x.startswith("\t") and not x.strip().startswith("."):
                cur.append(x.strip())
        blocks.append(cur)
        yield b - a, blocks


def _lean_loop(text: str, kernel: str):
    """-> (mnemonic counts without the rare blocks, all blocks) of the innermost loop that holds both sweeps and no |abs| maximum."""
    best = None
    for span, blocks in _loops(text, kernel):
        hot = [b for b in blocks if not any(i.startswith(("global_", "flat_", "buffer_")) for i in b)]
        c = collections.Counter(i.split()[0] for b in hot for i in b)
        abs_max = sum(1 for b in blocks for i in b if i.startswith("v_max_f64") and "|" in i)
        if c["v_fmac_f64_dpp"] >= 2 * 49 * 16 - 12 and abs_max == 0 and (best is None or span < best[0]):
            best = (span, c, blocks)
    assert best, "no lean loop in " + kernel
    return best[1], best[2]


def _metadata(text: str, kernel: str) -> dict:
    i = text.index(".name:           " + kernel)
    block = text[i:text.find("\n  - ", i)]
    return {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", block)}


@pytest.mark.parametrize("which", list(KERNELS))
def test_lean_loop_instruction_count(which):
    c, blocks = _lean_loop(_asm(), KERNELS[which])
    assert c["v_fmac_f64_dpp"] == 2 * 49 * 16 - 12, c["v_fmac_f64_dpp"]
    assert c["v_fma_f64"] == 48 + 2, c["v_fma_f64"]
    movs = sum(v for k, v in c.items() if k.startswith("v_mov_b64"))
    assert movs <= 56, movs
    valu = sum(v for k, v in c.items() if k.startswith("v_"))
    print(which, "lean loop: VALU", valu, "v_mov_b64*", movs, "LDS", sum(v for k, v in c.items() if k.startswith("ds_")))
    assert valu <= 1960, valu  # (2,176 in the plain kernel's loop)
    # no scratch access in ANY block of the lean loop, the rare ones included
    assert not [i for b in blocks for i in b if i.startswith("scratch_")]
    # ... and no chain pushed off the 8-byte grid (D_AL would have padded it with an s_nop)
    assert c["s_nop"] == 0, c["s_nop"]


def test_every_lean_kernel_runs_two_wavefronts_per_simd_without_scratch():
    text = _asm()
    names = sorted(set(re.findall(r"^\s+\.name:\s+(%s)$" % ALL_LEAN, text, re.M)))
    assert KERNELS["headline"] in names and KERNELS["goal"] in names, names
    for k in names:
        md = _metadata(text, k)
        assert md["vgpr_count"] <= 256, (k, md)
        assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, (k, md)


def test_the_plain_translation_unit_has_no_lean_kernel_and_keeps_its_code():
    """The variant is textual: nothing of it reaches tinympc_solve_d.hip's code, whose headline kernel still has the recorded hash."""
    path = ge.device_asm_path("tinympc_solve_d.hip")
    if not os.path.exists(path):
        pytest.skip("no build assembly (run __graft_entry__.build())")
    assert "_lean" not in open(path).read()
    want, got = json.load(open(RECORD)), current_hash()
    if got["compiler"] != want["compiler"]:
        pytest.skip(f"another compiler ({got['compiler']} against {want['compiler']}): the recorded hash does not apply")
    assert got["kernel"] == KERNEL and got["sha256"] == want["sha256"], got


def test_the_lean_headline_kernel_is_the_code_that_was_measured():
    if not os.path.exists(RECORD_LEAN):
        pytest.skip("no recorded hash")
    want = json.load(open(RECORD_LEAN))
    got = current_hash(KERNEL_LEAN, SOURCE_LEAN)
    if got is None:
        pytest.skip("no build assembly (run __graft_entry__.build())")
    if got["compiler"] != want["compiler"]:
        pytest.skip(f"another compiler ({got['compiler']} against {want['compiler']}): the recorded hash does not apply")
    assert got["sha256"] == want["sha256"], (
        f"the lean headline kernel's code changed ({got['instructions']} instructions, recorded {want['instructions']}): A/B the builds with "
        f"tools/headline_ab.py on one box, then `python tools/headline_code_hash.py --record-lean` (recorded state: {want['measured']})")
