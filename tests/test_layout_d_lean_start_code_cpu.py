"""Static checks of layout D's lean kernels with LDS accumulator starts and hoisted loop control (tinympc_lstart_d.hip =
tinympc_solve_d.hip with TINY_LEAN and TINY_LEAN_START) in the build's gfx950 assembly; the parsing is test_layout_d_lean_code_cpu.py's.

The lean loop of tinympc_lean_d.hip has 1,916 VALU instructions per wavefront-iteration, all of them the algorithm's own arithmetic
except 49 `v_mov_b64`, the forward steps' accumulator starts `a = cf`. Here 48 of them are gone -- cf sits in a 16-double table in LDS
and a `ds_read_b64` issued one block ahead fills the accumulator; step 0 keeps its copy of c0, which is per instance -- and the loop's
control (write-back test, "all done" exit, it_done) is evaluated once per run of lean rounds instead of once per round. The bound on
the VALU count, 1,870, is the census less the 48 copies plus two of slack, set before anything was built; what the build has is 1,862
(six fewer than that: with `active` invariant in the loop the compiler also moves the ballot behind the backward sweep's masked d
stores out of it), 1 `v_mov_b64*`, 213 LDS instructions (165), 3 branch instructions.

Branches of the parent's lean loop, counted on a build of the parent commit with the same compiler: 9 in the headline kernel
(5 s_cbranch_vccz, 1 s_cbranch_vccnz, 1 s_cbranch_scc0, 1 s_cbranch_execnz, 1 s_branch), 12 in its goal form.

(What the compiler's assembly cannot show: every chain block opens with `.p2align 3`, and a block whose surroundings come to 4 bytes
more than a multiple of 8 -- the LDS-slot steps of tinympc_lean_d.hip, every forward step from 1 on here -- gets one 4-byte padding
s_nop from the assembler. The `s_nop` counted below are the compiler's own.)"""
from __future__ import annotations

import collections
import json
import os
import re

import pytest

import __graft_entry__ as ge
from tools.headline_code_hash import (KERNEL, KERNEL_LEAN, KERNEL_LEAN_START, RECORD, RECORD_LEAN, RECORD_LEAN_START, SOURCE_LEAN,
                                      SOURCE_LEAN_START, current_hash)

KERNELS = {  # the quadrotor N=50 kernel (what the headline runs) and its per-instance goal form
    "headline": KERNEL_LEAN_START,
    "goal": "_ZN7tinympc30k_admm_solve_d_gbnd_lean_startILi12ELi4ELi50ELi4ELi25EEEvNS_11SolveParamsE",
}
PARENT_BRANCHES = {"headline": 9, "goal": 12}  # (see the module's docstring)
ALL_START = r"_ZN7tinympc\d+k_admm_solve_d(?:_gbnd)?_lean_startI\w+"
GLOBAL = ("global_", "flat_", "buffer_")


def _asm():
    path = ge.device_asm_path(SOURCE_LEAN_START)
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
        hot = [b for b in blocks if not any(i.startswith(GLOBAL) for i in b)]
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
def test_lean_loop_census(which):
    c, blocks = _lean_loop(_asm(), KERNELS[which])
    assert c["v_fmac_f64_dpp"] == 2 * 49 * 16 - 12, c["v_fmac_f64_dpp"]
    assert c["v_fma_f64"] == 48 + 2, c["v_fma_f64"]
    movs = sum(v for k, v in c.items() if k.startswith("v_mov_b64"))
    valu = sum(v for k, v in c.items() if k.startswith("v_"))
    print(which, "lean loop: VALU", valu, "v_mov_b64*", movs, "LDS", sum(v for k, v in c.items() if k.startswith("ds_")))
    assert movs <= 2, movs  # (step 0's start from c0; 49 in the lean kernels of tinympc_lean_d.hip)
    assert valu <= 1870, valu  # (1,916 there)
    # no scratch access and no global memory access in ANY block of the loop: the write-back is no longer part of it
    assert not [i for b in blocks for i in b if i.startswith("scratch_")]
    assert not [i for b in blocks for i in b if i.startswith(GLOBAL)]
    assert c["s_nop"] == 0, c["s_nop"]


@pytest.mark.parametrize("which", list(KERNELS))
def test_lean_loop_has_lost_the_control_branches(which):
    _, blocks = _lean_loop(_asm(), KERNELS[which])
    branches = [i for b in blocks for i in b if re.match(r"s_c?branch", i)]
    print(which, "lean loop:", len(branches), "branch instructions", collections.Counter(i.split()[0] for i in branches))
    assert len(branches) <= PARENT_BRANCHES[which] - 2, branches


def test_every_kernel_of_the_unit_runs_two_wavefronts_per_simd_without_scratch():
    text = _asm()
    names = sorted(set(re.findall(r"^\s+\.name:\s+(%s)$" % ALL_START, text, re.M)))
    assert KERNELS["headline"] in names and KERNELS["goal"] in names and len(names) == 8, names  # (three shapes: 2 + 3 + 3 kernels)
    for k in names:
        md = _metadata(text, k)
        assert md["vgpr_count"] <= 256, (k, md)
        assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, (k, md)


def test_the_unit_holds_only_its_own_symbols_and_the_other_units_keep_their_code():
    """The variant is textual: the plain and the lean translation units have none of its symbols and still have their recorded hashes."""
    for source in ("tinympc_solve_d.hip", SOURCE_LEAN):
        path = ge.device_asm_path(source)
        if not os.path.exists(path):
            pytest.skip("no build assembly (run __graft_entry__.build())")
        assert "_lean_start" not in open(path).read(), source
    assert not re.search(r"k_admm_solve_d(?:_gbnd)?(?:_lean)?I", _asm())
    for kernel, source, record in ((KERNEL, "tinympc_solve_d.hip", RECORD), (KERNEL_LEAN, SOURCE_LEAN, RECORD_LEAN)):
        want, got = json.load(open(record)), current_hash(kernel, source)
        if got["compiler"] != want["compiler"]:
            pytest.skip(f"another compiler ({got['compiler']} against {want['compiler']}): the recorded hash does not apply")
        assert got["sha256"] == want["sha256"], (kernel, got)


def test_the_headline_kernel_is_the_code_that_was_measured():
    want = json.load(open(RECORD_LEAN_START))
    got = current_hash(KERNEL_LEAN_START, SOURCE_LEAN_START)
    if got is None:
        pytest.skip("no build assembly (run __graft_entry__.build())")
    if got["compiler"] != want["compiler"]:
        pytest.skip(f"another compiler ({got['compiler']} against {want['compiler']}): the recorded hash does not apply")
    assert got["sha256"] == want["sha256"], (
        f"the headline kernel's code changed ({got['instructions']} instructions, recorded {want['instructions']}): A/B the builds with "
        f"tools/headline_ab.py on one box, then `python tools/headline_code_hash.py --record-lean-start` (recorded state: {want['measured']})")
