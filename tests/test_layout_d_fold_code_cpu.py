"""Static instruction count of layout D's iteration loop (tinympc_solve_d.hip) in the build's gfx950 assembly.

The headline kernel is bound by FP64 VALU issue, so what it costs is the number of VALU instructions a wavefront issues per
iteration. Two parts of that work do not change within a launch and are done once (K0 / FOLD in tinympc_solve_d.hip): forward step 0
keeps only its nu input columns (the state columns are summed into c0 before the loop), and the backward step's tail is 2 FP64
instructions instead of 3 (r_s is not formed: the operator's input columns carry -rho). Per wavefront-iteration of quadrotor N=50 that
is 2 sweeps x 49 steps x 16 columns - 12 = 1,556 fused DPP FMAs and 48 + 2 v_fma_f64. The loop's rare paths (write-back, stale copies:
the only blocks of the loop that touch global memory) are not counted."""
from __future__ import annotations

import collections
import os
import re

import pytest
from conftest import ROOT

import __graft_entry__ as ge

KERNELS = {  # the plain quadrotor N=50 kernel (the headline) and its per-instance goal form
    "headline": "_ZN7tinympc14k_admm_solve_dILi12ELi4ELi50ELb1ELi4ELi25ELb0EEEvNS_11SolveParamsE",
    "goal": "_ZN7tinympc19k_admm_solve_d_gbndILi12ELi4ELi50ELi4ELi25EEEvNS_11SolveParamsE",
}


def _asm():
    path = ge.device_asm_path("tinympc_solve_d.hip")
    if not os.path.exists(path):
        pytest.skip("no build assembly (run __graft_entry__.build())")
    return open(path).read()


def _loop_counts(text: str, kernel: str) -> collections.Counter:
    """Instruction mnemonics of the iteration loop (the widest span between a label and a branch back to it), rare paths left out."""
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
            cur.append(x.split()[0])
    blocks.append(cur)
    out = collections.Counter()
    for b in blocks:
        if not any(i.startswith(("global_", "flat_", "buffer_")) for i in b):
            out.update(b)
    return out


def _metadata(text: str, kernel: str) -> dict:
    i = text.index(".name:           " + kernel)
    block = text[i:text.find("\n  - ", i)]
    return {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", block)}


@pytest.mark.parametrize("which", list(KERNELS))
def test_iteration_loop_instruction_count(which):
    c = _loop_counts(_asm(), KERNELS[which])
    assert c["v_fmac_f64_dpp"] == 2 * 49 * 16 - 12, c["v_fmac_f64_dpp"]
    assert c["v_fma_f64"] == 48 + 2, c["v_fma_f64"]
    valu = sum(v for k, v in c.items() if k.startswith("v_"))
    assert valu <= 2200, valu  # (2,237 before the two folds)


@pytest.mark.parametrize("which", list(KERNELS))
def test_two_wavefronts_per_simd_without_scratch(which):
    md = _metadata(_asm(), KERNELS[which])
    assert md["vgpr_count"] <= 256, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, md
