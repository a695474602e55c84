#!/usr/bin/env python3
"""Record what the reference's own compiled core answers in the adaptive-rho and code-generation tests, so that those tests run
where oracle/_ref cannot be built (it needs the reference tree) -- the GPU box and a plain checkout included.

    make -C oracle ref ref_zeroinit && python tests/golden/gen_ref_records.py

adaptive_rho_ref.npz  the zero-initialised build (oracle/Makefile target ref_zeroinit) of the cases of tests/test_adaptive_rho.py:
                      per case the sensitivity tables, and per solve x0, return code, iterations, status, rho, solution, Kinf, Pinf.
                      Keys: "<case>__<name>", per-solve names end in _<solve index>.
codegen_ref.npz       the reference emitter (oracle/_ref ref_codegen) for tests/test_codegen.py: the cache and statistics it was driven
                      with, and a SHA-256 digest of every line of the generated tiny_data.hpp / tiny_data.cpp (after the time-stamped
                      comment block). Digests only: no generated text is stored.
"""
from __future__ import annotations

import hashlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyoracle as O  # noqa: E402
import __graft_entry__ as ge  # noqa: E402
from test_adaptive_rho import CLIP_CASES, CLIP_N, CLIP_SETTINGS, SOLVE_CASES, x0_of_solve  # noqa: E402
from test_codegen import SETTINGS as CODEGEN_SETTINGS, codegen_problem, body_lines  # noqa: E402

P = ge.load_package().problems


def record_adaptive() -> dict:
    out = {}

    def run(tag, prob, settings, adaptive, nsolve):
        ref = O.OracleRef(prob, zeroinit=True).load_problem(prob, settings)
        ref.set_adaptive_rho(True, *adaptive)
        for n in ("dKinf_drho", "dPinf_drho", "dC1_drho", "dC2_drho"):
            out[f"{tag}__{n}"] = ref.get(n)
        for k in range(nsolve):
            x0 = x0_of_solve(prob, k)
            ref.set_x0(x0)
            out[f"{tag}__x0_{k}"] = x0
            out[f"{tag}__rc_{k}"] = np.array(ref.solve())
            st = ref.stats()
            out[f"{tag}__iter_{k}"], out[f"{tag}__status_{k}"], out[f"{tag}__rho_{k}"] = np.array(st["iter"]), np.array(st["status"]), np.array(st["rho"])
            out[f"{tag}__x_{k}"], out[f"{tag}__u_{k}"] = ref.solution()
            out[f"{tag}__Kinf_{k}"], out[f"{tag}__Pinf_{k}"] = ref.get("Kinf"), ref.get("Pinf")

    for N, settings in SOLVE_CASES:
        run(f"N{N}", P.quadrotor(N), settings, (1.0, 100.0, True), 3)
    for i, adaptive in enumerate(CLIP_CASES):
        run(f"clip{i}", P.quadrotor(CLIP_N), CLIP_SETTINGS, adaptive, 1)
    return out


def record_codegen() -> dict:
    out = {}
    for which in ("cartpole", "quadrotor"):
        prob = codegen_problem(P, which)
        ref = O.OracleRef(prob).load_problem(prob, CODEGEN_SETTINGS)
        ref.set_x0(prob.x0)
        ref.solve()
        st = ref.stats()
        out[f"{which}__iter"], out[f"{which}__solved"] = np.array(st["iter"]), np.array(st["solved"])
        for n in ("Kinf", "Pinf", "Quu_inv", "AmBKt"):
            out[f"{which}__{n}"] = ref.get(n)
        with tempfile.TemporaryDirectory() as d:
            assert ref.codegen(os.path.join(d, "ref")) == 0
            for f, key in (("tinympc/tiny_data.hpp", "hpp"), ("src/tiny_data.cpp", "cpp")):
                lines = body_lines(os.path.join(d, "ref", f))
                out[f"{which}__{key}_line_sha256"] = np.array([np.frombuffer(hashlib.sha256(line.encode()).digest(), np.uint8) for line in lines])
    return out


if __name__ == "__main__":
    if not (os.path.exists(O.REF_LIB) and os.path.exists(O.REF_ZEROINIT_LIB)):
        sys.exit("oracle/_ref is not built: make -C oracle ref ref_zeroinit (needs the reference tree)")
    np.savez_compressed(os.path.join(HERE, "adaptive_rho_ref.npz"), **record_adaptive())
    np.savez_compressed(os.path.join(HERE, "codegen_ref.npz"), **record_codegen())
    print("wrote", os.path.join(HERE, "adaptive_rho_ref.npz"), os.path.join(HERE, "codegen_ref.npz"))
