"""CPU checks of the per-knot linear-constraint verbs (tinympc_set_linear_constraints_knots_batch and its _device form): the stepped
oracle the GPU tests compare against (tests/knot_lin_cases.py) is orc_solve, bit for bit, where the rows are the same at every knot; the
verbs are declared, exported and typed; a NULL handle is refused before anything touches a device; the Python method refuses a solver
that was never set up and arrays of the wrong shape before the library is called; the sharding helper cuts the verb's arrays along the
instance axis; and the generated code of the mode's kernel (k_admm_solve_ifamk, tinympc_ifamk_a.hip) uses no scratch memory."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import ROOT

import __graft_entry__ as ge
import knot_lin_cases as K

VERBS = ["tinympc_set_linear_constraints_knots_batch", "tinympc_set_linear_constraints_knots_batch_device"]


@pytest.mark.parametrize("name", K.VERIFIED)
def test_stepped_oracle_with_repeated_rows_is_orc_solve_bit_for_bit(pkg, name):
    """Knot 0's rows of an instance repeated over the horizon: states, controls, iteration count and status of the stepped oracle equal
    orc_solve's under those rows, on every sampled instance of the four verified cases."""
    prob, nlx, nlu, batch, settings = K.case(pkg, name)
    x0s, *rows = K.rows_knots(prob, nlx, nlu, batch)
    for b in K.sample(batch):
        rb = K.held(K.of(rows, b), prob.N)
        wh = K.whole_solve(prob, settings, x0s[:, b], (rb[0][:, :, 0], rb[1][:, 0], rb[2][:, :, 0], rb[3][:, 0]))
        st = K.SteppedOracle(prob, settings, rb).solve(x0s[:, b], rb)
        print(name, "instance", b, "iterations", st[2], wh[2], "status", st[3], wh[3])
        np.testing.assert_array_equal(st[0], wh[0])
        np.testing.assert_array_equal(st[1], wh[1])
        assert st[2:] == wh[2:]


def test_verbs_are_declared_exported_and_typed(pkg):
    header = open(os.path.join(ROOT, "include", "tinympc_hip.h")).read()
    lib = pkg.load_library()
    L = pkg._lib
    for name in VERBS:
        assert "int " + name + "(tinympc_solver *s, const double *" in header
        assert hasattr(lib, name)
        res, args = L.SIGNATURES[name]
        ptr = C.c_void_p if name.endswith("_device") else L.c_double_p
        assert res is C.c_int
        assert args == [L.Handle, ptr, ptr, C.c_int, ptr, ptr, C.c_int, C.c_int, C.c_int]
    assert "#define TINYMPC_ABI_VERSION 1" in header  # (symbols were added, nothing changed)
    assert pkg.abi_version() == 1


@pytest.mark.parametrize("name", VERBS)
def test_null_handle_is_not_initialized(pkg, name):
    lib = pkg.load_library()
    L = pkg._lib
    A, b = np.ones(4 * 5), np.ones(5)
    if name.endswith("_device"):
        pa, pb = C.c_void_p(A.ctypes.data), C.c_void_p(b.ctypes.data)
    else:
        pa, pb = A.ctypes.data_as(L.c_double_p), b.ctypes.data_as(L.c_double_p)
    assert getattr(lib, name)(None, pa, pb, 1, None, None, 0, 0, 1) == L.ERR_NOT_INITIALIZED
    assert getattr(lib, name)(None, None, None, 0, None, None, 0, 0, 1) == L.ERR_NOT_INITIALIZED


def test_python_method_needs_setup(pkg):
    s = pkg.TinyMPC()
    calls = (lambda: s.set_linear_constraints_knots_batch(np.ones((1, 4, 5, 3)), np.ones((1, 5, 3)), None, None),
             lambda: s.set_linear_constraints_knots_batch(None, None, np.ones((2, 1, 4, 2)), np.ones((2, 4, 2)), first=5))
    for call in calls:
        with pytest.raises(pkg.TinyMPCError) as ei:
            call()
        assert ei.value.code == pkg._lib.ERR_NOT_INITIALIZED


def test_python_method_refuses_wrong_shapes_before_the_library(pkg, monkeypatch):
    """A solver object with the dimensions of a set-up one and NO handle: a shape error must be raised before the handle is used."""
    s = pkg.TinyMPC()
    monkeypatch.setattr(s, "_check_setup", lambda: None)
    s.nx, s.nu, s.N, s.batch = 4, 1, 5, 3
    one = np.ones
    bad = [
        (one((1, 4, 3)), one((1, 3)), None, None),                    # the constant verb's shapes: no knot axis
        (one((1, 4, 4, 3)), one((1, 4, 3)), None, None),              # N-1 knots on the state side
        (one((1, 5, 5, 3)), one((1, 5, 3)), None, None),              # nx + 1 columns
        (one((1, 4, 5, 3)), one((2, 5, 3)), None, None),              # b with another row count
        (one((1, 4, 5, 3)), one((1, 5, 2)), None, None),              # b with another instance count
        (None, None, one((2, 1, 5, 3)), one((2, 5, 3))),              # N knots on the input side
        (one((1, 4, 5, 3)), one((1, 5, 3)), one((2, 1, 4, 2)), one((2, 4, 2))),  # sides with different instance counts
    ]
    for arrays in bad:
        with pytest.raises(pkg.TinyMPCError) as ei:
            s.set_linear_constraints_knots_batch(*arrays)
        assert ei.value.code == pkg._lib.ERR_INVALID_INPUT, arrays


def test_sharding_cuts_the_instance_axis(pkg):
    """Every rank's slice of the verb's arrays, handed to its own handle with first = 0: the shards are contiguous, cover the batch
    once, keep the knot axis whole, and an empty side stays empty."""
    B = pkg.batch
    rng = np.random.default_rng(0)
    Ax, bx, bu = rng.standard_normal((2, 12, 20, 37)), rng.standard_normal((2, 20, 37)), rng.standard_normal((1, 19, 37))
    seen = []
    for rank in range(4):
        first, (sax, sbx, sau, sbu) = B.shard_instances((Ax, bx, None, bu), rank, 4)
        assert (first, sbx.shape[-1]) == B.shard_range(37, rank, 4) and sau is None
        assert sax.shape[:3] == (2, 12, 20) and sbx.shape[:2] == (2, 20) and sbu.shape[:2] == (1, 19)
        np.testing.assert_array_equal(sax, Ax[..., first:first + sax.shape[-1]])
        np.testing.assert_array_equal(sbu, bu[..., first:first + sbu.shape[-1]])
        seen += list(range(first, first + sax.shape[-1]))
    assert seen == list(range(37))


def _kernels(text):
    """{mangled kernel name: its metadata fields} of one device assembly file."""
    out = {}
    for block in re.split(r"\n  - \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = {k: int(v) for k, v in
                     re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", block)}
    return out


def test_the_kernel_of_the_mode_uses_no_scratch():
    """The build's assembly of tinympc_ifamk_a.hip: fifteen kernels, the geometries and forms of k_admm_solve_ifam. No form uses scratch
    memory or spills a vector register; at 16 lanes per instance (nine forms) the scalar spill count is zero as well, as
    k_admm_solve_ifam's is. The scalar spills of the wider forms go to vector-register lanes (registers, not memory) and are printed."""
    path = ge.device_asm_path("tinympc_ifamk_a.hip")
    assert os.path.exists(path), "build() leaves the assembly of every source next to its object file"
    ks = {k: v for k, v in _kernels(open(path).read()).items() if "k_admm_solve_ifamk" in k}
    assert len(ks) == 15, sorted(ks)
    for name, md in sorted(ks.items()):
        lanes = int(re.search(r"ifamkILi(\d+)E", name).group(1))
        print(name, md)
        assert lanes in (16, 32, 64)
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md["vgpr_spill_count"] == 0 and md["vgpr_count"] <= 512, (name, md)
        if lanes == 16:
            assert md["sgpr_spill_count"] == 0, (name, md)
    assert sum("ifamkILi16E" in k for k in ks) == 9
