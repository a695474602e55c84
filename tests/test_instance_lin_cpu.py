"""CPU checks of the per-instance linear-constraint verbs (tinympc_set_linear_constraints_batch and its _device form): declared, exported
and typed in the ctypes table; a NULL handle is refused before anything touches a device; the Python method refuses a solver that was
never set up; the sharding helper cuts the verb's arrays along the instance axis; and the generated code of the mode's one kernel
(k_admm_solve_ifam, tinympc_ifam_a.hip) uses no scratch memory."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest
from conftest import ROOT

import __graft_entry__ as ge

VERBS = ["tinympc_set_linear_constraints_batch", "tinympc_set_linear_constraints_batch_device"]


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


@pytest.mark.parametrize("name", VERBS)
def test_null_handle_is_not_initialized(pkg, name):
    lib = pkg.load_library()
    L = pkg._lib
    A, b = np.ones(4), np.ones(1)
    if name.endswith("_device"):
        pa, pb = C.c_void_p(A.ctypes.data), C.c_void_p(b.ctypes.data)
    else:
        pa, pb = A.ctypes.data_as(L.c_double_p), b.ctypes.data_as(L.c_double_p)
    assert getattr(lib, name)(None, pa, pb, 1, None, None, 0, 0, 1) == L.ERR_NOT_INITIALIZED
    assert getattr(lib, name)(None, None, None, 0, None, None, 0, 0, 1) == L.ERR_NOT_INITIALIZED


def test_python_method_needs_setup(pkg):
    s = pkg.TinyMPC()
    calls = (lambda: s.set_linear_constraints_batch(np.ones((1, 4, 3)), np.ones((1, 3)), None, None),
             lambda: s.set_linear_constraints_batch(None, None, np.ones((2, 1, 2)), np.ones((2, 2)), first=5))
    for call in calls:
        with pytest.raises(pkg.TinyMPCError) as ei:
            call()
        assert ei.value.code == pkg._lib.ERR_NOT_INITIALIZED


def test_sharding_cuts_the_instance_axis(pkg):
    """Every rank's slice of the verb's arrays, handed to its own handle with first = 0: the shards are contiguous, cover the batch
    once, and an empty side stays empty."""
    B = pkg.batch
    rng = np.random.default_rng(0)
    Ax, bx, bu = rng.standard_normal((2, 12, 37)), rng.standard_normal((2, 37)), rng.standard_normal((1, 37))
    seen = []
    for rank in range(4):
        first, (sax, sbx, sau, sbu) = B.shard_instances((Ax, bx, None, bu), rank, 4)
        assert (first, sbx.shape[-1]) == B.shard_range(37, rank, 4) and sau is None
        np.testing.assert_array_equal(sax, Ax[..., first:first + sax.shape[-1]])
        np.testing.assert_array_equal(sbu, bu[..., first:first + sbu.shape[-1]])
        seen += list(range(first, first + sax.shape[-1]))
    assert seen == list(range(37))
    with pytest.raises(ValueError):
        B.shard_instances((Ax, bx[:, :5]), 0, 2)


def _kernels(text):
    """{mangled kernel name: its metadata fields} of one device assembly file."""
    out = {}
    for block in re.split(r"\n  - \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = {k: int(v) for k, v in
                     re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", block)}
    return out


def test_the_kernel_of_the_mode_uses_no_scratch():
    """The build's assembly of tinympc_ifam_a.hip: fifteen kernels -- five (lanes per instance, columns) geometries, each with the state
    in LDS with or without the tables beside it, or in HBM.
    16 lanes per instance (nine forms), the condition: no scratch memory (private_segment_fixed_size 0) and zero spill counts, vector
    and scalar. The families' body alone parks 36 to 50 wave-uniform values in the lanes of a vector register (k_admm_solve_fam, same
    build); this kernel gives the arguments' pointers vector registers as their home instead and spills nothing.
    32 and 64 lanes (six forms): no scratch memory and no vector spill, so no width is refused (the 64-lane form fetches the first four
    per-instance rows of every sweep when the sweep starts instead of holding them for the whole solve: it needed 120 bytes of scratch
    otherwise). Their scalar spills to vector-register lanes (59 to 81: registers, not memory) are printed."""
    path = ge.device_asm_path("tinympc_ifam_a.hip")
    assert os.path.exists(path), "build() leaves the assembly of every source next to its object file"
    ks = {k: v for k, v in _kernels(open(path).read()).items() if "k_admm_solve_ifam" in k}
    assert len(ks) == 15, sorted(ks)
    for name, md in sorted(ks.items()):
        lanes = int(re.search(r"ifamILi(\d+)E", name).group(1))
        print(name, md)
        assert lanes in (16, 32, 64)
        assert md["private_segment_fixed_size"] == 0, (name, md)
        assert md["vgpr_spill_count"] == 0 and md["vgpr_count"] <= 512, (name, md)
        if lanes == 16:
            assert md["sgpr_spill_count"] == 0, (name, md)
    assert sum("ifamILi16E" in k for k in ks) == 9
