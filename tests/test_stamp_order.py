"""Build-time lint of the generated gfx950 code: the store order behind the completion stamp (tools/stamp_lint.py).

Layouts C and F answer a single-instance handle through pinned host memory: write-through stores from every wavefront, then a completion
stamp that the host polls. The stamp may only follow once every thread has retired its own stores (tinympc_device.h:
host_stores_retired, the barrier, host_stamp_store). __graft_entry__.build() runs the lint on the assembly of the objects it links and
fails on a violation; this file checks the lint itself on planted text and every kernel that raises a stamp: tinympc_solve_c.hip (the
build's own `.s` when it is current, a fresh `hipcc -S` otherwise), the compiled-in layout-F kernels, and layout F as hiprtc builds it."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest
from conftest import ROOT

from tools.stamp_lint import STAMP_MARK, WAIT_MARK, lint as _stamp_lint

CSRC = os.path.join(ROOT, "tinympc-matlab_amd", "csrc")

# planted text for tools/stamp_lint.py: a write-through store of the write-out, the two helpers' marks, the stamp behind its barrier
_HOST_STORE = "global_store_dwordx2 v[4:5], v[2:3], off sc0 sc1\n"
_RETIRED = ";;#ASMSTART\n ; %s\n ;;#ASMEND\n" % WAIT_MARK
_WAIT = _RETIRED + "s_waitcnt vmcnt(0)\n"
_STAMP = ("s_and_saveexec_b64 s[2:3], vcc\n s_cbranch_execz .LBB0_90\n ;;#ASMSTART\n ; %s\n ;;#ASMEND\n v_mov_b32_e32 v9, 0\n"
          "global_store_dwordx2 v9, v[6:7], s[4:5] offset:48 sc0 sc1\n.LBB0_90:\n s_endpgm\n" % STAMP_MARK)


def test_stamp_lint_flags_a_stamp_that_can_overtake_a_host_store():
    # the shape through round 5: store, barrier, stamp -- no wait on vmcnt (a workgroup-scope release emits none), no helper
    sites, bad = _stamp_lint(_HOST_STORE + "s_barrier\n" + _STAMP)
    assert sites == {"": 1} and len(bad) == 2 and any("vmcnt(0)" in b[2] for b in bad) and any("host_stores_retired" in b[2] for b in bad)
    # a wait on the LDS / scalar counter alone, and a wait that leaves one store in flight
    for wait in ("s_waitcnt lgkmcnt(0)\n", "s_waitcnt vmcnt(1)\n", "s_waitcnt vmcnt(10) lgkmcnt(0)\n"):
        sites, bad = _stamp_lint(_HOST_STORE + _RETIRED + wait + "s_barrier\n" + _STAMP)
        assert sites == {"": 1} and len(bad) == 1 and "vmcnt(0)" in bad[0][2], wait
    # a host store between the wait and the barrier
    sites, bad = _stamp_lint(_HOST_STORE + _WAIT + "flat_store_dwordx2 v[4:5], v[2:3] sc0 sc1\n s_barrier\n" + _STAMP)
    assert sites == {"": 1} and len(bad) == 1 and bad[0][1].startswith("flat_store")
    # the wait on the fall-through path, but not on the path through a branch that skips it
    sites, bad = _stamp_lint(_HOST_STORE + "s_cbranch_scc1 .LBB0_2\n" + _WAIT + ".LBB0_2:\n s_barrier\n" + _STAMP)
    assert sites == {"": 1} and len(bad) == 1 and bad[0][1].startswith("global_store")
    # a store loop whose body begins with a vmcnt(0) for its load: the first wait in program order retires nothing of the LAST pass
    loop = ".LBB0_1:\n global_load_dwordx2 v[2:3], v[10:11], off\n s_waitcnt vmcnt(0)\n" + _HOST_STORE + "s_cbranch_scc1 .LBB0_1\n"
    sites, bad = _stamp_lint(loop + _RETIRED + "s_barrier\n" + _STAMP)
    assert sites == {"": 1} and len(bad) == 1
    # second property: the L2 is neither written back nor invalidated between the last host stores and the stamp
    for where in (0, 1, 2):
        op = "buffer_inv sc0 sc1\n" if where == 2 else "buffer_wbl2 sc0 sc1\n"
        text = _HOST_STORE + (op if where == 0 else "") + _WAIT + (op if where == 1 else "") + "s_barrier\n" + _STAMP.replace("v_mov_b32_e32 v9, 0\n", op if where == 2 else "")
        sites, bad = _stamp_lint(text)
        assert sites == {"": 1} and len(bad) == 1 and bad[0][1].startswith(op.split()[0]), where
    # a stamp's mark with no barrier in front of it, or with no store behind it
    assert len(_stamp_lint(_HOST_STORE + _WAIT + _STAMP)[1]) == 1
    assert len(_stamp_lint(_HOST_STORE + _WAIT + "s_barrier\n" + _STAMP.replace(" sc0 sc1", ""))[1]) == 1


def test_stamp_lint_accepts_the_helper_order_on_every_path():
    assert _stamp_lint(_HOST_STORE + _WAIT + "s_barrier\n" + _STAMP) == ({"": 1}, [])
    # the compiler may fold its own waits into the helper's
    assert _stamp_lint(_HOST_STORE + _RETIRED + "s_waitcnt vmcnt(0) expcnt(0) lgkmcnt(0)\n s_barrier\n" + _STAMP) == ({"": 1}, [])
    assert _stamp_lint(_HOST_STORE + _RETIRED + "v_cmp_eq_u32_e32 vcc, 0, v0\n s_waitcnt vmcnt(0) lgkmcnt(0)\n s_barrier\n" + _STAMP) == ({"": 1}, [])
    # the store loop (its body begins with a vmcnt(0) for a load) left through its exit path, the wait behind the loop ...
    loop = ".LBB0_1:\n global_load_dwordx2 v[2:3], v[10:11], off\n s_waitcnt vmcnt(0)\n" + _HOST_STORE + "s_cbranch_scc1 .LBB0_1\n"
    assert _stamp_lint(loop + _WAIT + "s_barrier\n" + _STAMP) == ({"": 1}, [])
    # ... and the wait in front of a loop-exit label that the store loop reaches, and a branch around the loop (no store on that path)
    assert _stamp_lint("s_cbranch_scc0 .LBB0_3\n" + loop + _WAIT + ".LBB0_3:\n s_barrier\n" + _STAMP) == ({"": 1}, [])
    mid = ".LBB0_1:\n s_waitcnt vmcnt(0)\n" + _HOST_STORE + "s_cbranch_scc0 .LBB0_3\n v_add_u32_e32 v10, 8, v10\n s_branch .LBB0_1\n.LBB0_3:\n"
    assert _stamp_lint(mid + _WAIT + "s_barrier\n" + _STAMP) == ({"": 1}, [])
    # early-answer lines (SolveParams::host_ans) are host stores that nothing waits for: only what precedes a stamp's barrier counts
    early = "global_store_dwordx2 v8, v[0:1], s[6:7] sc0 sc1\n s_barrier\n v_add_f64 v[2:3], v[2:3], v[2:3]\n"
    assert _stamp_lint(early + _HOST_STORE + _WAIT + "s_barrier\n" + _STAMP) == ({"": 1}, [])
    # a function without a stamp: no site, no finding -- per function (`name:` ... `.Lfunc_end`)
    assert _stamp_lint(_HOST_STORE + "s_barrier\n" + _HOST_STORE + "s_endpgm\n") == ({"": 0}, [])
    two = "k_tables:\n" + _HOST_STORE + "s_barrier\n s_endpgm\n.Lfunc_end0:\nk_solve:\n" + _HOST_STORE + _WAIT + "s_barrier\n" + _STAMP + ".Lfunc_end1:\n"
    assert _stamp_lint(two) == ({"k_tables": 0, "k_solve": 1}, [])
    # (a plain store -- no sc0 sc1 -- is not the host's business)
    assert _stamp_lint(_HOST_STORE + _WAIT + "global_store_dwordx2 v[4:5], v[2:3], off\n s_barrier\n" + _STAMP) == ({"": 1}, [])


# the specialisations of tests/test_isa_hazards.py::test_layout_f_specialisations_have_no_dpp_hazard_and_no_scratch
E_ROCKET = dict(nround=1, ncone=2, cones="{0,0,2},{0,6,8}", nlx=1, nlu=0)
F_SHAPES = [
    (6, 3, 100, 0, 7, 4, E_ROCKET),     # BASELINE config 4, one instance (the build lints the same instance)
    (6, 3, 100, 1, 7, 4, dict(nround=2, ncone=3, cones="{0,0,2},{0,6,8},{1,1,4}", nlx=12, nlu=5)),  # overlapping cones, many rows (run-time loop)
    (6, 3, 10, 0, 2, 2, E_ROCKET),      # short horizon: five chunks of two slots, a one-slot last chunk
    (12, 4, 50, 1, 7, 2, None),         # box path
    (4, 1, 120, 1, 8, 4, None),         # eight wavefronts
]
_f_asm = {}  # (one compilation per specialisation, shared by the tests below)


def _layout_f_asm(nx, nu, N, ct, wpg, S, fam, session, tmp_path):
    """tinympc_solve_f.hip with the options tinympc_jit.hip hands hiprtc for one specialisation, compiled here with hipcc: the assembly."""
    key = (nx, nu, N, ct, wpg, S, repr(fam), session)
    if key not in _f_asm:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("hipcc not available")
        f = fam or dict(nround=0, ncone=0, cones="{-1,0,0}", nlx=0, nlu=0)
        out = tmp_path / "jit_f.s"
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "-w", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        "-DTINY_JIT=1", f"-DTINY_JIT_NX={nx}", f"-DTINY_JIT_NU={nu}", f"-DTINY_JIT_N={N}", f"-DTINY_JIT_CT={ct}", f"-DTINY_JIT_FAM={1 if fam else 0}",
                        f"-DTINY_JIT_F_WPG={wpg}", f"-DTINY_JIT_F_S={S}", f"-DTINY_JIT_E_NROUND={f['nround']}", f"-DTINY_JIT_E_NCONE={f['ncone']}",
                        f"-DTINY_JIT_E_CONES={f['cones']}", f"-DTINY_JIT_E_NLX={f['nlx']}", f"-DTINY_JIT_E_NLU={f['nlu']}", *(["-DTINY_JIT_F_SESSION=1"] if session else []),
                        "-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "tinympc_solve_f.hip")], check=True, timeout=900)
        _f_asm[key] = out.read_text()
    return _f_asm[key]


# ---- the completion stamp's store order (tools/stamp_lint.py) on the generated code. Every kernel that serves a single-instance handle's
# pinned-host path raises exactly ONE stamp; the counts are asserted per function, so that a kernel the lint cannot find its site in fails.
# tinympc_solve_c.hip's functions that raise none, and why:
C_WITHOUT_STAMP = {
    "k_build_chunk_tables": "builds layout C's chunked tables in device memory before a solve: no host store at all",
    "k_build_f_input_tables": "builds layout F's input-side tables in device memory before a solve: no host store at all",
}


def _assert_one_stamp_in_order(text, kernels, where):
    sites, bad = _stamp_lint(text)
    assert not bad, f"{where}: {len(bad)} finding(s) on the completion stamp's store order, first: {bad[:3]}"
    assert kernels and set(kernels) <= set(sites), (where, sorted(set(kernels) - set(sites)))
    wrong = {k: sites[k] for k in kernels if sites[k] != 1}
    assert not wrong, f"{where}: one stamp site expected in each of these (host_stores_retired / host_stamp_store, tinympc_device.h): {wrong}"
    return sites


def test_layout_c_raises_its_stamp_behind_retired_host_stores(tmp_path):
    """Every instantiation of k_admm_solve_c (the latency kernel: launched and resident, with and without the families)."""
    import __graft_entry__ as ge
    source = "tinympc_solve_c.hip"
    built = ge.device_asm_path(source)
    if os.path.exists(built) and os.path.getmtime(built) >= max(os.path.getmtime(os.path.join(CSRC, f)) for f in (source, "tinympc_device.h")):
        text = open(built).read()
    else:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("hipcc not available and no build assembly")
        out = tmp_path / (source + ".s")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "-w", "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, "-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, source)], check=True, timeout=900)
        text = out.read_text()
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
    solve = [k for k in kernels if "k_admm_solve_c" in k]
    others = [k for k in kernels if k not in solve]
    assert len(solve) >= 40 and len(set(solve)) == len(solve), len(solve)
    assert len(others) == len(C_WITHOUT_STAMP) and all(any(n in k for k in others) for n in C_WITHOUT_STAMP), others
    sites = _assert_one_stamp_in_order(text, solve, source)
    assert set(sites) == set(kernels), "a function of %s is no kernel: %s" % (source, sorted(set(sites) ^ set(kernels)))
    assert all(sites[k] == 0 for k in others), {k: sites[k] for k in others}
    assert sum(sites.values()) == len(solve)


def test_compiled_in_layout_f_kernels_raise_their_stamp_behind_retired_host_stores():
    """Every compiled-in specialisation of tinympc_solve_f.hip, launched and resident (`_session`), in the form that was linked."""
    import __graft_entry__ as ge
    names = [e[0] for e in ge.HIP_BUILTINS if e[1] == "tinympc_solve_f.hip"]
    assert len(names) == 8 and sum(n.endswith("_session") for n in names) == 3
    for name in names:
        path = ge.builtin_asm_path(name)
        if not os.path.exists(path):
            pytest.skip("no build assembly (run __graft_entry__.build())")
        sites = _assert_one_stamp_in_order(open(path).read(), [name], name)
        assert sites == {name: 1}, sites


@pytest.mark.parametrize("nx,nu,N,ct,wpg,S,fam,session", [s + (False,) for s in F_SHAPES] + [s + (True,) for s in F_SHAPES if s[3] == 0])
def test_layout_f_specialisations_raise_their_stamp_behind_retired_host_stores(nx, nu, N, ct, wpg, S, fam, session, tmp_path):
    """Layout F as hiprtc will build it on the GPU box (nothing lints the result there): the shapes of the test above, and the resident
    form (-DTINY_JIT_F_SESSION=1) of those with per-knot tables -- the session kernel exists for CT=0 only (tinympc_solve_f.hip refuses
    SESSION with CT at compile time)."""
    text = _layout_f_asm(nx, nu, N, ct, wpg, S, fam, session, tmp_path)
    sites = _assert_one_stamp_in_order(text, ["tinympc_jit_solve"], "tinympc_solve_f.hip as a run-time specialisation")
    assert sites == {"tinympc_jit_solve": 1}, sites
