"""TinyMPC -- host-side mirror of the reference's MATLAB class (/root/reference/src/TinyMPC.m).

Same method names, argument meaning, defaults and error behaviour as the `.m` class, over the C ABI
of libtinympc_hip.so instead of the MEX function. MATLAB itself is not available in the build image;
the drop-in `.m` class and MEX shim live in tinympc-matlab_amd/matlab/ and mirror this file.

Reference behaviours reproduced here (file:line in /root/reference/src/TinyMPC.m):
  constructor defaults                     :24-40   tol 1e-4, max_iter 100, check_termination 1, bounds off
  setup(A,B,Q,R,N,'rho',..)                :42-104  dimension asserts, unknown options silently ignored (:368-376),
                                                     bound flags forced off at setup (:71-73), settings pushed (:94-98)
  set_x0 / set_x_ref / set_u_ref           :106-124 x0(:) column; refs broadcast by expand_matrix (:393-405)
  update_settings                          :126-139 only known fields, then pushed
  solve -> always 0                        :141-147
  get_solution -> states / controls        :149-157
  set_bound_constraints                    :256-278 expand with -/+1e17 fill (:378-391), both flags auto-enabled
  set_linear / cone / equality constraints :243-317
  reset                                    :319-325
  check_setup -> TinyMPC:NotSetup          :328-334
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import TinyMPCError, c_double_p, c_int_p

BOUND_INF = 1e17


def _f(a) -> np.ndarray:
    return np.asfortranarray(np.asarray(a, dtype=np.float64))


def _p(a: np.ndarray):
    return a.ctypes.data_as(c_double_p)


class TinyMPC:
    def __init__(self):
        self.nx = self.nu = self.N = 0
        self.A = self.B = self.Q = self.R = None
        self.rho = 1.0
        self.is_setup = False
        self.batch = 1
        self.settings = dict(abs_pri_tol=1e-4, abs_dua_tol=1e-4, max_iter=100, check_termination=1,
                             en_state_bound=False, en_input_bound=False, en_state_soc=False, en_input_soc=False,
                             en_state_linear=False, en_input_linear=False, adaptive_rho=False,
                             adaptive_rho_min=0.1, adaptive_rho_max=10.0, adaptive_rho_enable_clipping=True)
        self.x_min = self.x_max = self.u_min = self.u_max = None
        self._h = _lib.Handle()
        self._tick = None  # persistent buffers of mpc_step / session_step
        self._L = None

    # ------------------------------------------------------------------ setup
    def setup(self, A, B, Q, R, N, batch: int = 1, device: int = -1, **varargin):
        A, B, Q, R = _f(A), _f(B), _f(Q), _f(R)
        if B.ndim == 1:
            B = _f(B.reshape(-1, 1))
        assert A.ndim == 2 and A.shape[0] == A.shape[1], "A must be square"
        assert A.shape[0] == B.shape[0], "A and B row dimensions must match"
        assert Q.shape[0] == A.shape[0], "Q must match A dimensions"
        assert R.shape[0] == B.shape[1], "R must match B column dimension"
        assert N >= 2, "N must be >= 2"
        self.nx, self.nu, self.N = A.shape[0], B.shape[1], int(N)
        self.A, self.B, self.Q, self.R = A, B, Q, R
        opts = self._parse_options(dict(rho=1.0, fdyn=None, verbose=False, abs_pri_tol=1e-4, abs_dua_tol=1e-4,
                                        max_iter=100, check_termination=1, en_state_bound=False,
                                        en_input_bound=False, adaptive_rho=False, adaptive_rho_min=0.1,
                                        adaptive_rho_max=10.0, adaptive_rho_enable_clipping=True), varargin)
        self.rho = float(opts["rho"])
        for k in ("abs_pri_tol", "abs_dua_tol", "max_iter", "check_termination", "adaptive_rho",
                  "adaptive_rho_min", "adaptive_rho_max", "adaptive_rho_enable_clipping"):
            self.settings[k] = opts[k]
        # Do not enable bound constraints in setup; only via set_bound_constraints (TinyMPC.m:71-73)
        self.settings["en_state_bound"] = False
        self.settings["en_input_bound"] = False
        fdyn = np.zeros(self.nx) if opts["fdyn"] is None else _f(opts["fdyn"]).reshape(-1)
        assert fdyn.size == self.nx, "fdyn must have nx entries"
        fdyn = _f(fdyn)

        self._L = _lib.load_library()
        if self._h:
            self._L.tinympc_reset(C.byref(self._h), 0)  # the reference replaces its global solver (bindings.cpp:92)
        self.batch = int(batch)
        status = self._L.tinympc_setup_batch(C.byref(self._h), _p(A), _p(B), _p(fdyn), _p(Q), _p(R), self.rho,
                                             self.nx, self.nu, self.N, self.batch, int(device), int(bool(opts["verbose"])))
        if status != 0:
            raise TinyMPCError(status, f"Setup failed with status {status}: {_lib.last_error()}")
        self.is_setup = True
        self._push_settings()
        if opts["verbose"]:
            print(f"TinyMPC solver setup successful (nx={self.nx}, nu={self.nu}, N={self.N})")

    # ------------------------------------------------------------------ ingest
    def set_x0(self, x0):
        self._check_setup()
        x0 = _f(np.asarray(x0, dtype=np.float64).reshape(-1))
        _lib.check(self._L.tinympc_set_x0(self._h, _p(x0), x0.size, 0))

    def set_x_ref(self, x_ref):
        self._check_setup()
        xr = _f(self._expand_matrix(x_ref, self.nx, self.N))
        rows, cols = (xr.shape + (1,))[:2] if xr.ndim else (1, 1)
        _lib.check(self._L.tinympc_set_x_ref(self._h, _p(xr), rows, cols, 0))

    def set_u_ref(self, u_ref):
        self._check_setup()
        ur = _f(self._expand_matrix(u_ref, self.nu, self.N - 1))
        rows, cols = (ur.shape + (1,))[:2] if ur.ndim else (1, 1)
        _lib.check(self._L.tinympc_set_u_ref(self._h, _p(ur), rows, cols, 0))

    def update_settings(self, **kw):
        self._check_setup()
        for k, v in kw.items():
            if k in self.settings:  # unknown names are ignored, as isfield() does (TinyMPC.m:129-133)
                self.settings[k] = v
        self._push_settings()

    def set_bound_constraints(self, x_min, x_max, u_min, u_max):
        self._check_setup()
        self.x_min = _f(self._expand_bounds(x_min, self.nx, self.N, -BOUND_INF))
        self.x_max = _f(self._expand_bounds(x_max, self.nx, self.N, +BOUND_INF))
        self.u_min = _f(self._expand_bounds(u_min, self.nu, self.N - 1, -BOUND_INF))
        self.u_max = _f(self._expand_bounds(u_max, self.nu, self.N - 1, +BOUND_INF))
        for a, shape in ((self.x_min, (self.nx, self.N)), (self.x_max, (self.nx, self.N)),
                         (self.u_min, (self.nu, self.N - 1)), (self.u_max, (self.nu, self.N - 1))):
            if a.shape != shape:
                raise TinyMPCError(_lib.ERR_INVALID_INPUT, f"bound array has shape {a.shape}, expected {shape}")
        _lib.check(self._L.tinympc_set_bound_constraints(self._h, _p(self.x_min), _p(self.x_max),
                                                         _p(self.u_min), _p(self.u_max), 0))
        self.settings["en_state_bound"] = True
        self.settings["en_input_bound"] = True
        self._push_settings()

    def set_linear_constraints(self, Alin_x, blin_x, Alin_u, blin_u):
        self._check_setup()
        ax, bx = self._mat(Alin_x, self.nx), _f(np.asarray(blin_x, dtype=np.float64).reshape(-1))
        au, bu = self._mat(Alin_u, self.nu), _f(np.asarray(blin_u, dtype=np.float64).reshape(-1))
        nlx = ax.shape[0] if ax.size else 0
        nlu = au.shape[0] if au.size else 0
        _lib.check(self._L.tinympc_set_linear_constraints(self._h, _p(ax), _p(bx), nlx, _p(au), _p(bu), nlu))
        self.settings["en_state_linear"] = bool(nlx)
        self.settings["en_input_linear"] = bool(nlu)
        if nlx or nlu:
            self._push_settings()

    def set_cone_constraints(self, Acx, qcx, cx, Acu, qcu, cu):
        self._check_setup()
        ax, qx = np.asarray(Acx, dtype=np.int32).reshape(-1), np.asarray(qcx, dtype=np.int32).reshape(-1)
        au, qu = np.asarray(Acu, dtype=np.int32).reshape(-1), np.asarray(qcu, dtype=np.int32).reshape(-1)
        cxa, cua = _f(np.asarray(cx, dtype=np.float64).reshape(-1)), _f(np.asarray(cu, dtype=np.float64).reshape(-1))
        _lib.check(self._L.tinympc_set_cone_constraints(
            self._h, ax.ctypes.data_as(c_int_p), qx.ctypes.data_as(c_int_p), _p(cxa), ax.size,
            au.ctypes.data_as(c_int_p), qu.ctypes.data_as(c_int_p), _p(cua), au.size))
        self.settings["en_state_soc"] = bool(ax.size and qx.size and cxa.size)
        self.settings["en_input_soc"] = bool(au.size and qu.size and cua.size)
        if self.settings["en_state_soc"] or self.settings["en_input_soc"]:
            self._push_settings()

    def set_equality_constraints(self, Aeq_x, beq_x, Aeq_u, beq_u):
        """Aeq*s == beq as the two inequalities [A; -A] s <= [b; -b] (TinyMPC.m:296-317)."""
        self._check_setup()
        ax, bx = self._mat(Aeq_x, self.nx), np.asarray(beq_x, dtype=np.float64).reshape(-1)
        au, bu = self._mat(Aeq_u, self.nu), np.asarray(beq_u, dtype=np.float64).reshape(-1)
        lx = (np.vstack([ax, -ax]), np.concatenate([bx, -bx])) if ax.size else (np.zeros((0, self.nx)), np.zeros(0))
        lu = (np.vstack([au, -au]), np.concatenate([bu, -bu])) if au.size else (np.zeros((0, self.nu)), np.zeros(0))
        self.set_linear_constraints(lx[0], lx[1], lu[0], lu[1])

    def set_cache_terms(self, Kinf, Pinf, Quu_inv, AmBKt):
        self._check_setup()
        k, p_, q, a = _f(Kinf), _f(Pinf), _f(Quu_inv), _f(AmBKt)
        assert k.shape == (self.nu, self.nx) and p_.shape == (self.nx, self.nx)
        assert q.shape == (self.nu, self.nu) and a.shape == (self.nx, self.nx)
        _lib.check(self._L.tinympc_set_cache_terms(self._h, _p(k), _p(p_), _p(q), _p(a), 0))

    def set_sensitivity_matrices(self, dK, dP, dC1, dC2):
        self._check_setup()
        dK, dP, dC1, dC2 = _f(dK), _f(dP), _f(dC1), _f(dC2)
        assert dK.shape == (self.nu, self.nx), "dK must be nu x nx"
        assert dP.shape == (self.nx, self.nx), "dP must be nx x nx"
        assert dC1.shape == (self.nu, self.nu), "dC1 must be nu x nu"
        assert dC2.shape == (self.nx, self.nx), "dC2 must be nx x nx"
        _lib.check(self._L.tinympc_set_sensitivity_matrices(self._h, _p(dK), _p(dP), _p(dC1), _p(dC2), 0))

    # ------------------------------------------------------------------ solve / egress
    def solve(self) -> int:
        """Always returns 0, like the reference (TinyMPC.m:146); see get_stats() for the core status."""
        self._check_setup()
        _lib.check(self._L.tinympc_solve(self._h, 0))
        return 0

    def get_solution(self) -> dict:
        self._check_setup()
        x = np.zeros((self.nx, self.N), order="F")
        u = np.zeros((self.nu, self.N - 1), order="F")
        _lib.check(self._L.tinympc_get_solution(self._h, _p(x), _p(u), 0))
        return {"states": x, "controls": u}

    def get_stats(self) -> dict:
        """The MEX verb get_stats (bindings.cpp:264-285; not surfaced by TinyMPC.m) plus all residuals."""
        self._check_setup()
        it, st = C.c_int(), C.c_int()
        ps, pi = C.c_double(), C.c_double()
        _lib.check(self._L.tinympc_get_stats(self._h, C.byref(it), C.byref(st), C.byref(ps), C.byref(pi), 0))
        res = (C.c_double * 4)()
        _lib.check(self._L.tinympc_get_residuals(self._h, res))
        return dict(iter=it.value, status=st.value, primal_residual_state=ps.value, primal_residual_input=pi.value,
                    dual_residual_state=res[1], dual_residual_input=res[3], solved=int(st.value == 1))

    def get_cache(self) -> dict:
        """Device-computed LQR cache (what compute_cache_terms would be compared against)."""
        self._check_setup()
        K = np.zeros((self.nu, self.nx), order="F")
        P = np.zeros((self.nx, self.nx), order="F")
        Qi = np.zeros((self.nu, self.nu), order="F")
        Am = np.zeros((self.nx, self.nx), order="F")
        it = C.c_int()
        _lib.check(self._L.tinympc_get_cache(self._h, _p(K), _p(P), _p(Qi), _p(Am), C.byref(it)))
        return dict(Kinf=K, Pinf=P, Quu_inv=Qi, AmBKt=Am, C1=Qi, C2=Am, riccati_iters=it.value)

    def codegen(self, output_dir, source_dir=None):
        """Write the embedded project's data files from the cache on the device, then -- as the class does after
        the MEX call (TinyMPC.m:159-169, 415-434) -- copy the solver sources next to them and create build/.
        The sources are the `codegen_src` tree of a TinyMPC checkout: `source_dir`, else $TINYMPC_CODEGEN_SRC,
        else a `codegen_src` directory beside this file; without one only the generated files are written."""
        self._check_setup()
        status = self._L.tinympc_codegen(self._h, str(output_dir).encode(), 0)
        if status != 0:
            raise TinyMPCError(status, f"Code generation failed with status: {status}: {_lib.last_error()}")
        self._copy_build_artifacts(output_dir, source_dir)

    def codegen_with_sensitivity(self, output_dir, dK, dP, dC1, dC2, source_dir=None):
        self._check_setup()
        self.set_sensitivity_matrices(dK, dP, dC1, dC2)
        dK, dP, dC1, dC2 = _f(dK), _f(dP), _f(dC1), _f(dC2)
        status = self._L.tinympc_codegen_with_sensitivity(self._h, str(output_dir).encode(), _p(dK), _p(dP), _p(dC1), _p(dC2), 0)
        if status != 0:
            raise TinyMPCError(status, f"Code generation with sensitivity failed with status: {status}: {_lib.last_error()}")
        self._copy_build_artifacts(output_dir, source_dir)

    @staticmethod
    def _copy_build_artifacts(output_dir, source_dir=None):
        import os
        import shutil
        src = source_dir or os.environ.get("TINYMPC_CODEGEN_SRC") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "codegen_src")
        if os.path.isdir(src):
            shutil.copytree(src, str(output_dir), dirs_exist_ok=True)
        os.makedirs(os.path.join(str(output_dir), "build"), exist_ok=True)

    def _cache_buffers(self):
        nx, nu = self.nx, self.nu
        return (np.zeros((nu, nx), order="F"), np.zeros((nx, nx), order="F"),
                np.zeros((nu, nu), order="F"), np.zeros((nx, nx), order="F"))

    def compute_cache_terms(self):
        """[Kinf, Pinf, Quu_inv, AmBKt] of the class's own Riccati loop (TinyMPC.m:194-221: full Q and R, rho
        added once, P0 = Q, 1e-8 regulariser, norm(K - Kprev) < 1e-10, at most 5000 steps), run on the device."""
        self._check_setup()
        K, P, Qi, Am = self._cache_buffers()
        it = C.c_int()
        _lib.check(self._L.tinympc_compute_cache_terms(self._h, _p(K), _p(P), _p(Qi), _p(Am), C.byref(it), 0))
        self.cache_terms_iters = it.value
        return K, P, Qi, Am

    def solve_lqr(self, rho_val: float):
        """[K, P, C1, C2] for Q + rho_val*I, R + rho_val*I (TinyMPC.m:336-366; idare there, a device-side
        fixed-point recursion to stationarity here)."""
        self._check_setup()
        K, P, C1, C2 = self._cache_buffers()
        _lib.check(self._L.tinympc_solve_lqr(self._h, float(rho_val), _p(K), _p(P), _p(C1), _p(C2), None))
        return K, P, C1, C2

    def compute_sensitivity_autograd(self):
        """[dK, dP, dC1, dC2]: forward differences of solve_lqr in rho, h = 1e-6 (TinyMPC.m:223-241)."""
        self._check_setup()
        dK, dP, dC1, dC2 = self._cache_buffers()
        _lib.check(self._L.tinympc_compute_sensitivity(self._h, _p(dK), _p(dP), _p(dC1), _p(dC2), 0))
        return dK, dP, dC1, dC2

    def print_problem_data(self):
        self._check_setup()
        _lib.check(self._L.tinympc_print_problem_data(self._h))

    def reset(self):
        if self.is_setup:
            self._L.tinympc_reset(C.byref(self._h), 0)
            self.is_setup = False

    def __del__(self):
        try:
            if self.is_setup and self._L is not None:
                self._L.tinympc_reset(C.byref(self._h), 0)
                self.is_setup = False
        except Exception:
            pass

    # ------------------------------------------------------------------ batched extensions
    def set_x0_batch(self, x0s, first: int = 0):
        """x0s: nx x count (column b = instance first+b), numpy array or a CUDA torch tensor (count x nx
        contiguous, i.e. the same memory layout)."""
        self._check_setup()
        if hasattr(x0s, "data_ptr") and getattr(x0s, "is_cuda", False):
            assert x0s.dtype.itemsize == 8 and x0s.is_contiguous() and x0s.numel() % self.nx == 0
            count = x0s.numel() // self.nx
            # the C ABI's contract: the producer of the tensor has finished (the handle's stream is ordered against no
            # torch stream); the copy itself completes inside the call
            import torch
            torch.cuda.current_stream(x0s.device).synchronize()
            _lib.check(self._L.tinympc_set_x0_batch_device(self._h, C.c_void_p(x0s.data_ptr()), first, count))
            return
        a = _f(x0s)
        assert a.shape[0] == self.nx
        _lib.check(self._L.tinympc_set_x0_batch(self._h, _p(a), first, a.shape[1]))

    def set_x_ref_batch(self, x_refs, first: int = 0):
        """Per-instance state references for instances first, first+1, ...: a numpy array of shape (nx, count) (one goal per
        instance, held over the horizon) or (nx, N, count) (a trajectory per instance), or a CUDA torch tensor with the same memory
        layout, (count, nx) or (count, N, nx) contiguous. set_x_ref() returns every instance to the shared reference. Goals run on
        layout D's goal form where the handle runs layout D; a converging batch beyond one resident set (16-lane shapes) runs it
        with slot refill, bit-identical to the plain goal kernel (jit_info(): 'goal slot-refill'; TINYMPC_REFILL=0 switches it off).
        Trajectories run on layout D's trajectory form after prepare(), and beyond that form's resident set (4,096 quadrotors at
        N=50) with slot refill as well ('per-instance-trajectories slot-refill')."""
        self._check_setup()
        self._set_batch("references", (x_refs,), (self.nx,), (self.N,), self._L.tinympc_set_x_ref_batch,
                        self._L.tinympc_set_x_ref_batch_device, first, self.nx)

    def set_u_ref_batch(self, u_refs, first: int = 0):
        """Per-instance input references: (nu, count) or (nu, N-1, count); see set_x_ref_batch."""
        self._check_setup()
        self._set_batch("references", (u_refs,), (self.nu,), (self.N - 1,), self._L.tinympc_set_u_ref_batch,
                        self._L.tinympc_set_u_ref_batch_device, first, self.nu)

    # reference tracks: upload once, step per tick (include/tinympc_hip.h)
    def set_x_ref_track_batch(self, x_tracks, first: int = 0):
        """Per-instance state reference TRACKS for instances first, first+1, ...: a numpy array of shape (nx, T, count) -- T >= 1 knots
        per instance, independent of N; (nx, T) on a single-instance solver -- or a CUDA torch tensor with the same memory layout,
        (count, T, nx) contiguous float64. Kept on the device: instance b at step k tracks columns min(k+i, T-1), i = 0..N-1, of its
        track, so a closed-loop tick uploads nothing but x0 (set_ref_step_batch, advance_ref_step, set_ref_auto_advance). The first
        call must name the whole batch; set_x_ref() / a whole-batch set_x_ref_batch() leave the mode. After prepare() a tick runs on
        layout D's trajectory form, with slot refill for a converging batch beyond one resident set (see set_x_ref_batch)."""
        self._check_setup()
        self._set_track(x_tracks, self.nx, self._L.tinympc_set_x_ref_track_batch, self._L.tinympc_set_x_ref_track_batch_device, first)

    def set_u_ref_track_batch(self, u_tracks, first: int = 0):
        """Per-instance input reference tracks: (nu, T, count); see set_x_ref_track_batch (window columns min(k+i, T-1), i = 0..N-2)."""
        self._check_setup()
        self._set_track(u_tracks, self.nu, self._L.tinympc_set_u_ref_track_batch, self._L.tinympc_set_u_ref_track_batch_device, first)

    def _set_track(self, tracks, rows, f_host, f_device, first):
        if hasattr(tracks, "data_ptr") and getattr(tracks, "is_cuda", False):
            import torch
            ok = tracks.dtype == torch.float64 and tracks.is_contiguous() and tracks.shape[-1] == rows and \
                (tracks.dim() == 3 or (tracks.dim() == 2 and self.batch == 1)) and tracks.shape[-2] >= 1
            if not ok:
                raise TinyMPCError(_lib.ERR_INVALID_INPUT, "tracks on the device must be contiguous float64 tensors of shape (count, T, %d) "
                                   "with T >= 1, got %s %s" % (rows, tracks.dtype, tuple(tracks.shape)))
            count = int(tracks.shape[0]) if tracks.dim() == 3 else 1
            torch.cuda.current_stream(tracks.device).synchronize()  # (the set_x0_batch contract)
            _lib.check(f_device(self._h, C.c_void_p(tracks.data_ptr()), rows, int(tracks.shape[-2]), int(first), count))
            return
        a = np.asarray(tracks, dtype=np.float64)
        if a.ndim == 2 and self.batch == 1:
            a = a.reshape(a.shape + (1,))
        if a.ndim != 3 or a.shape[0] != rows or a.shape[1] < 1:
            raise TinyMPCError(_lib.ERR_INVALID_INPUT, "tracks must be %d x T x count with T >= 1%s, got %s"
                               % (rows, " (or %d x T)" % rows if self.batch == 1 else "", a.shape))
        a = _f(a)
        _lib.check(f_host(self._h, _p(a), rows, int(a.shape[1]), int(first), int(a.shape[2])))

    def set_ref_step_batch(self, steps, first: int = 0):
        """The steps (positions in their tracks) of instances first, first+1, ...: a vector of `count` integers >= 0, or a contiguous
        int32 CUDA tensor of `count` elements on the handle's GPU (validated on the device)."""
        self._check_setup()
        if hasattr(steps, "data_ptr") and getattr(steps, "is_cuda", False):
            import torch
            if steps.dtype != torch.int32 or not steps.is_contiguous() or steps.dim() != 1:
                raise TinyMPCError(_lib.ERR_INVALID_INPUT, "steps on the device must be a contiguous int32 tensor of shape (count,), got %s %s"
                                   % (steps.dtype, tuple(steps.shape)))
            torch.cuda.current_stream(steps.device).synchronize()  # (the set_x0_batch contract)
            _lib.check(self._L.tinympc_set_ref_step_batch_device(self._h, C.c_void_p(steps.data_ptr()), int(first), int(steps.numel())))
            return
        raw = np.atleast_1d(np.asarray(steps))
        if raw.ndim != 1 or not np.issubdtype(raw.dtype, np.integer) or (raw.size and (raw.min() < -2**31 or raw.max() >= 2**31)):
            raise TinyMPCError(_lib.ERR_INVALID_INPUT, "steps must be a vector of count 32-bit integers, got %s %s" % (raw.dtype, raw.shape))
        a = np.ascontiguousarray(raw, dtype=np.int32)
        _lib.check(self._L.tinympc_set_ref_step_batch(self._h, a.ctypes.data_as(c_int_p), int(first), int(a.size)))

    def advance_ref_step(self, delta: int = 1):
        """Every instance's step += delta, on the device (no copy, no synchronisation for delta >= 0)."""
        self._check_setup()
        _lib.check(self._L.tinympc_advance_ref_step_batch(self._h, int(delta)))

    def set_ref_auto_advance(self, delta: int = 1):
        """mpc_step() adds delta >= 0 to every instance's step after its solve; 0 switches it off."""
        self._check_setup()
        _lib.check(self._L.tinympc_set_ref_auto_advance(self._h, int(delta)))

    def get_ref_step_batch(self, first: int = 0, count: int | None = None) -> np.ndarray:
        self._check_setup()
        count = self.batch - first if count is None else count
        out = np.zeros(max(count, 0), dtype=np.int32)
        _lib.check(self._L.tinympc_get_ref_step_batch(self._h, out.ctypes.data_as(c_int_p), int(first), int(count)))
        return out

    def set_bound_constraints_batch(self, x_min, x_max, u_min, u_max, first: int = 0):
        """Per-instance box bounds for instances first, first+1, ...: numpy arrays of shape (nx, count) / (nu, count) (one box per
        instance, held over the horizon) or (nx, N, count) / (nu, N-1, count) (bounds per knot), or CUDA torch tensors with the same
        memory layout, (count, nx) / (count, nu) or (count, N, nx) / (count, N-1, nu) contiguous float64. All four in the same form.
        Enables both bound families, as set_bound_constraints does; set_bound_constraints() returns every instance to shared bounds.
        One box per instance (beside references constant over the horizon) runs on layout D's goal form, with slot refill where a
        shared box would have it (see set_x_ref_batch); bounds per knot run on layout D's per-knot bounds form after prepare(), with
        slot refill beyond that form's resident set ('per-knot-bounds slot-refill')."""
        self._check_setup()
        self._set_batch("bounds", (x_min, x_max, u_min, u_max), (self.nx, self.nx, self.nu, self.nu), (self.N, self.N, self.N - 1, self.N - 1),
                        self._L.tinympc_set_bound_constraints_batch, self._L.tinympc_set_bound_constraints_batch_device, first)
        self.settings["en_state_bound"] = True
        self.settings["en_input_bound"] = True

    def set_linear_constraints_batch(self, Alin_x, blin_x, Alin_u, blin_u, first: int = 0):
        """Per-instance linear constraints a'x <= b / a'u <= b for instances first, first+1, ...: numpy arrays of shape (nlx, nx, count),
        (nlx, count), (nlu, nu, count), (nlu, count) -- or contiguous float64 CUDA tensors with the same memory layout, (count, nx, nlx),
        (count, nlx), (count, nu, nlu), (count, nlu); an empty side is None (or an array without elements). On a single-instance solver
        the arrays may lack the count axis. The row counts belong to the batch, the values to the instance; b = +inf switches one row
        off for one instance. The first call names the whole batch unless the solver holds shared rows of the same counts (the other
        instances then keep those); set_linear_constraints() returns every instance to shared rows. Enables the linear family of every
        non-empty side, as set_linear_constraints does, and keeps the ADMM state: re-send the rows between two mpc_step() ticks.
        Runs on layout A -- or, after prepare(), on layout D's per-instance linear-row form (nx+nu <= 16, N <= 22, bounds constant over
        the horizon, cones that share no row), with references that are constant over the horizon or per-instance trajectories / tracks
        (set_x_ref_batch, the track verbs: the form then reads every wavefront's own reference rows); a trajectory shared by the batch
        through set_x_ref() / set_u_ref() keeps the mode on layout A."""
        self._check_setup()
        sides = []
        for A, b, cols, name in ((Alin_x, blin_x, self.nx, "x"), (Alin_u, blin_u, self.nu, "u")):
            empty = A is None or (hasattr(A, "numel") and A.numel() == 0) or (not hasattr(A, "numel") and np.asarray(A).size == 0)
            if empty:
                sides.append((None, None, 0, None, False))
                continue
            if hasattr(A, "data_ptr") and getattr(A, "is_cuda", False):
                import torch
                if not (hasattr(b, "data_ptr") and getattr(b, "is_cuda", False)):
                    raise TinyMPCError(_lib.ERR_INVALID_INPUT, "linear rows: all must be CUDA tensors, or none")
                if A.dim() == 2 and self.batch == 1:
                    A, b = A.reshape((1,) + tuple(A.shape)), b.reshape(1, -1)
                ok = A.dtype == torch.float64 and b.dtype == torch.float64 and A.is_contiguous() and b.is_contiguous() and A.dim() == 3 and \
                    b.dim() == 2 and A.shape[1] == cols and tuple(b.shape) == (A.shape[0], A.shape[2])
                if not ok:
                    raise TinyMPCError(_lib.ERR_INVALID_INPUT, "linear rows on the device must be contiguous float64 tensors of shape (count, %d, nl%s) "
                                       "and (count, nl%s), got %s and %s" % (cols, name, name, tuple(A.shape), tuple(b.shape)))
                sides.append((C.c_void_p(A.data_ptr()), C.c_void_p(b.data_ptr()), int(A.shape[2]), int(A.shape[0]), True, (A, b)))
            else:
                A, b = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64)
                if A.ndim == 2 and self.batch == 1:
                    A, b = A.reshape(A.shape + (1,)), b.reshape(-1, 1)
                if A.ndim != 3 or A.shape[1] != cols or b.shape != (A.shape[0], A.shape[2]):
                    raise TinyMPCError(_lib.ERR_INVALID_INPUT, "linear rows must be nl%s x %d x count and nl%s x count, got %s and %s"
                                       % (name, cols, name, A.shape, b.shape))
                A, b = _f(A), _f(b)
                sides.append((_p(A), _p(b), int(A.shape[0]), int(A.shape[2]), False, (A, b)))
        (pax, pbx, nlx, cx, dx, *keep_x), (pau, pbu, nlu, cu, du, *keep_u) = sides
        if nlx and nlu and (cx != cu or dx != du):
            raise TinyMPCError(_lib.ERR_INVALID_INPUT, "linear rows: both sides must have the same count and be on the same side of the bus")
        on_device = dx if nlx else du
        count = cx if nlx else cu if nlu else 0
        if on_device:
            import torch
            torch.cuda.current_stream((keep_x or keep_u)[0][0].device).synchronize()  # (the set_x0_batch contract)
        f = self._L.tinympc_set_linear_constraints_batch_device if on_device else self._L.tinympc_set_linear_constraints_batch
        _lib.check(f(self._h, pax, pbx, nlx, pau, pbu, nlu, int(first), int(count)))
        if nlx:
            self.settings["en_state_linear"] = True
        if nlu:
            self.settings["en_input_linear"] = True

    def set_linear_constraints_knots_batch(self, Alin_x, blin_x, Alin_u, blin_u, first: int = 0):
        """Per-KNOT linear constraints a_i'x_i <= b_i / a_i'u_i <= b_i for instances first, first+1, ...: numpy arrays of shape
        (nlx, nx, N, count), (nlx, N, count), (nlu, nu, N-1, count), (nlu, N-1, count) -- or contiguous float64 CUDA tensors with the same
        memory layout, (count, N, nx, nlx), (count, N, nlx), (count, N-1, nu, nlu), (count, N-1, nlu); an empty side is None. The row counts
        belong to the batch, the values to the knot and the instance; b = +inf switches one row off at one knot. The first call names the
        whole batch, later calls may replace a sub-range; set_linear_constraints() returns every instance to shared rows, a whole-batch
        set_linear_constraints_batch() to rows constant over the horizon. Enables the linear family of every non-empty side and keeps the
        ADMM state: re-send the shifted rows between two mpc_step() ticks. Batched solvers only. Runs on layout A -- or, after prepare()
        (before or after this call), on the per-knot variant of layout D's per-instance linear-row form: nx+nu <= 16, bounds constant
        over the horizon, references constant over the horizon or per-instance trajectories / tracks (a trajectory shared by the batch
        through set_x_ref() keeps layout A), cones that share no row, and a horizon and row count whose rows of all knots fit a wavefront's
        share of the LDS (one row per side up to N = 22, two up to N = 12, three up to N = 8; beside per-instance trajectories or tracks,
        whose N+2 reference rows share that space: N = 17, 10, 7 for the quadrotor); launch_info()["layout"] and jit_info()
        (" per-knot-linear", with "refused(...)" in front after a refused plan) say which."""
        self._check_setup()
        sides = []
        for A, b, cols, knots, name in ((Alin_x, blin_x, self.nx, self.N, "x"), (Alin_u, blin_u, self.nu, self.N - 1, "u")):
            empty = A is None or (hasattr(A, "numel") and A.numel() == 0) or (not hasattr(A, "numel") and np.asarray(A).size == 0)
            if empty:
                sides.append((None, None, 0, None, False))
                continue
            if hasattr(A, "data_ptr") and getattr(A, "is_cuda", False):
                import torch
                if not (hasattr(b, "data_ptr") and getattr(b, "is_cuda", False)):
                    raise TinyMPCError(_lib.ERR_INVALID_INPUT, "per-knot linear rows: all must be CUDA tensors, or none")
                ok = A.dtype == torch.float64 and b.dtype == torch.float64 and A.is_contiguous() and b.is_contiguous() and A.dim() == 4 and \
                    b.dim() == 3 and A.shape[1] == knots and A.shape[2] == cols and tuple(b.shape) == (A.shape[0], knots, A.shape[3])
                if not ok:
                    raise TinyMPCError(_lib.ERR_INVALID_INPUT, "per-knot linear rows on the device must be contiguous float64 tensors of shape "
                                       "(count, %d, %d, nl%s) and (count, %d, nl%s), got %s and %s"
                                       % (knots, cols, name, knots, name, tuple(A.shape), tuple(b.shape)))
                sides.append((C.c_void_p(A.data_ptr()), C.c_void_p(b.data_ptr()), int(A.shape[3]), int(A.shape[0]), True, (A, b)))
            else:
                A, b = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64)
                if A.ndim != 4 or A.shape[1] != cols or A.shape[2] != knots or b.shape != (A.shape[0], knots, A.shape[3]):
                    raise TinyMPCError(_lib.ERR_INVALID_INPUT, "per-knot linear rows must be nl%s x %d x %d x count and nl%s x %d x count, got %s and %s"
                                       % (name, cols, knots, name, knots, A.shape, b.shape))
                A, b = _f(A), _f(b)
                sides.append((_p(A), _p(b), int(A.shape[0]), int(A.shape[3]), False, (A, b)))
        (pax, pbx, nlx, cx, dx, *keep_x), (pau, pbu, nlu, cu, du, *keep_u) = sides
        if nlx and nlu and (cx != cu or dx != du):
            raise TinyMPCError(_lib.ERR_INVALID_INPUT, "per-knot linear rows: both sides must have the same count and be on the same side of the bus")
        on_device = dx if nlx else du
        count = cx if nlx else cu if nlu else 0
        if on_device:
            import torch
            torch.cuda.current_stream((keep_x or keep_u)[0][0].device).synchronize()  # (the set_x0_batch contract)
        f = self._L.tinympc_set_linear_constraints_knots_batch_device if on_device else self._L.tinympc_set_linear_constraints_knots_batch
        _lib.check(f(self._h, pax, pbx, nlx, pau, pbu, nlu, int(first), int(count)))
        if nlx:
            self.settings["en_state_linear"] = True
        if nlu:
            self.settings["en_input_linear"] = True

    def set_cone_slopes_batch(self, cx, cu, first: int = 0):
        """Per-instance cone slopes for instances first, first+1, ... on the cone structure set_cone_constraints() installed: numpy arrays
        of shape (ncx, count) / (ncu, count) in the order of the cone list -- or contiguous float64 CUDA tensors (count, ncx) /
        (count, ncu); a side without cones is None. The structure belongs to the batch, the slopes to the instance: instance first+b
        solves what a single-instance solver would after set_cone_constraints(Acx, qcx, cx[:, b], Acu, qcu, cu[:, b]). Instances the
        call does not name keep the shared slopes; set_cone_constraints() returns every instance to shared slopes. Changes no enable
        flag and keeps the ADMM state: re-send the slopes between two mpc_step() ticks. On a single-instance solver the arrays may lack
        the count axis."""
        self._check_setup()
        sides = []
        for c, name in ((cx, "x"), (cu, "u")):
            empty = c is None or (hasattr(c, "numel") and c.numel() == 0) or (not hasattr(c, "numel") and np.asarray(c).size == 0)
            if empty:
                sides.append((None, 0, None, False, None))
            elif hasattr(c, "data_ptr") and getattr(c, "is_cuda", False):
                import torch
                if c.dim() == 1 and self.batch == 1:
                    c = c.reshape(1, -1)
                if c.dtype != torch.float64 or not c.is_contiguous() or c.dim() != 2:
                    raise TinyMPCError(_lib.ERR_INVALID_INPUT, "cone slopes on the device must be a contiguous float64 tensor of shape (count, nc%s), "
                                       "got %s %s" % (name, c.dtype, tuple(c.shape)))
                sides.append((C.c_void_p(c.data_ptr()), int(c.shape[1]), int(c.shape[0]), True, c))
            else:
                a = np.asarray(c, dtype=np.float64)
                if a.ndim == 1 and self.batch == 1:
                    a = a.reshape(-1, 1)
                if a.ndim != 2:
                    raise TinyMPCError(_lib.ERR_INVALID_INPUT, "cone slopes must be nc%s x count, got %s" % (name, a.shape))
                a = _f(a)
                sides.append((_p(a), int(a.shape[0]), int(a.shape[1]), False, a))
        (px, ncx, nbx, dx, keep_x), (pu, ncu, nbu, du, keep_u) = sides
        if ncx and ncu and (nbx != nbu or dx != du):
            raise TinyMPCError(_lib.ERR_INVALID_INPUT, "cone slopes: both sides must have the same count and be on the same side of the bus")
        if not ncx and not ncu:
            raise TinyMPCError(_lib.ERR_INVALID_INPUT, "cone slopes: no slopes on either side")
        on_device = dx if ncx else du
        count = nbx if ncx else nbu
        if on_device:
            import torch
            torch.cuda.current_stream((keep_x if ncx else keep_u).device).synchronize()  # (the set_x0_batch contract)
        f = self._L.tinympc_set_cone_slopes_batch_device if on_device else self._L.tinympc_set_cone_slopes_batch
        _lib.check(f(self._h, px, ncx, pu, ncu, int(first), int(count)))

    def set_model_batch(self, A, B, Q, R, fdyn=None, first: int = 0):
        """Per-instance models for instances first, first+1, ...: numpy arrays of shape (nx, nx, count), (nx, nu, count), (nx, nx, count),
        (nu, nu, count) and, optionally, fdyn (nx, count) -- or contiguous float64 CUDA tensors with the same memory layout, (count, nx, nx)
        holding A_b', (count, nu, nx) holding B_b', (count, nx, nx), (count, nu, nu), (count, nx). Of Q and R only the diagonals are used;
        N and the settings stay the handle's, and so does rho unless set_rho_batch() gives an instance its own. Instance b then solves what a single-instance solver set up with its model would
        solve. clear_model_batch() returns every instance to the shared model; get_cache_batch() reads the per-instance caches."""
        self._check_setup()
        nx, nu = self.nx, self.nu
        arrays = [A, B, Q, R] + ([fdyn] if fdyn is not None else [])
        shapes = [(nx, nx), (nx, nu), (nx, nx), (nu, nu)] + ([(nx,)] if fdyn is not None else [])
        on_device = [hasattr(a, "data_ptr") and getattr(a, "is_cuda", False) for a in arrays]
        if any(on_device):
            import torch
            if not all(on_device):
                raise TinyMPCError(_lib.ERR_INVALID_INPUT, "models: all must be CUDA tensors, or none")
            for a, sh in zip(arrays, shapes):
                if a.dtype != torch.float64 or not a.is_contiguous() or tuple(a.shape[1:]) != tuple(reversed(sh)):
                    raise TinyMPCError(_lib.ERR_INVALID_INPUT, "models on the device must be contiguous float64 tensors of shape (count, %s), got %s %s"
                                       % (", ".join(str(d) for d in reversed(sh)), a.dtype, tuple(a.shape)))
            counts = {int(a.shape[0]) for a in arrays}
            ptrs = [C.c_void_p(a.data_ptr()) for a in arrays] + ([None] if fdyn is None else [])
            f = self._L.tinympc_set_model_batch_device
        else:
            arrays = [np.asarray(a, dtype=np.float64) for a in arrays]
            for a, sh in zip(arrays, shapes):
                if a.ndim != len(sh) + 1 or tuple(a.shape[:-1]) != sh:
                    raise TinyMPCError(_lib.ERR_INVALID_INPUT, "models must be %s x count, got %s" % (" x ".join(str(d) for d in sh), a.shape))
            counts = {int(a.shape[-1]) for a in arrays}
            arrays = [_f(a) for a in arrays]
            ptrs = [_p(a) for a in arrays] + ([None] if fdyn is None else [])
            f = self._L.tinympc_set_model_batch
        if len(counts) != 1:
            raise TinyMPCError(_lib.ERR_INVALID_INPUT, "models: all must have the same count")
        (count,) = counts
        if on_device[0]:
            torch.cuda.current_stream(arrays[0].device).synchronize()  # (the set_x0_batch contract)
        pA, pB, pQ, pR, pf = ptrs
        _lib.check(f(self._h, pA, pB, pf, pQ, pR, int(first), count))

    def set_rho_batch(self, rhos, first: int = 0):
        """Per-instance ADMM penalty for instances first, first+1, ...: a numpy vector of `count` finite values > 0, or a contiguous
        float64 CUDA tensor of `count` elements on the handle's GPU. Instance first+b then solves what a single-instance solver set up
        with (its model, rhos[b]) would solve. This is the per-instance model mode of set_model_batch (the two commute; instances
        neither names keep the shared model / rho); clear_model_batch() returns every instance to the shared model and rho, and
        get_rho_batch() reads the values back."""
        self._check_setup()
        if hasattr(rhos, "data_ptr") and getattr(rhos, "is_cuda", False):
            import torch
            if rhos.dtype != torch.float64 or not rhos.is_contiguous() or rhos.dim() != 1:
                raise TinyMPCError(_lib.ERR_INVALID_INPUT, "rho on the device must be a contiguous float64 tensor of shape (count,), got %s %s"
                                   % (rhos.dtype, tuple(rhos.shape)))
            torch.cuda.current_stream(rhos.device).synchronize()  # (the set_x0_batch contract)
            _lib.check(self._L.tinympc_set_rho_batch_device(self._h, C.c_void_p(rhos.data_ptr()), int(first), int(rhos.numel())))
            return
        a = np.ascontiguousarray(np.asarray(rhos, dtype=np.float64))
        if a.ndim != 1:
            raise TinyMPCError(_lib.ERR_INVALID_INPUT, "rho must be a vector of count values, got %s" % (a.shape,))
        _lib.check(self._L.tinympc_set_rho_batch(self._h, _p(a), int(first), int(a.size)))

    def clear_model_batch(self):
        """Every instance back on the shared model and rho of setup()."""
        self._check_setup()
        _lib.check(self._L.tinympc_clear_model_batch(self._h))

    def get_cache_batch(self, first: int = 0, count: int | None = None) -> dict:
        """The LQR cache of instances first .. first+count-1: Kinf (nu, nx, count), Pinf (nx, nx, count), Quu_inv (nu, nu, count),
        AmBKt (nx, nx, count), riccati_iters (count,). Without per-instance models: the shared cache, repeated."""
        self._check_setup()
        count = self.batch - first if count is None else count
        n = max(count, 0)
        K = np.zeros((self.nu, self.nx, n), order="F")
        P = np.zeros((self.nx, self.nx, n), order="F")
        Qi = np.zeros((self.nu, self.nu, n), order="F")
        Am = np.zeros((self.nx, self.nx, n), order="F")
        it = np.zeros(n, dtype=np.int32)
        _lib.check(self._L.tinympc_get_cache_batch(self._h, _p(K), _p(P), _p(Qi), _p(Am), it.ctypes.data_as(_lib.c_int_p), int(first), int(count)))
        return dict(Kinf=K, Pinf=P, Quu_inv=Qi, AmBKt=Am, riccati_iters=it)

    # ------------------------------------------------------------------ closed-loop rollout on the device
    _ROLLOUT_LOGS = ("x", "u", "iter", "status")

    def rollout(self, ticks: int, disturbance=None, log=("x", "u", "iter", "status"), out=None) -> dict:
        """`ticks` closed-loop ticks on the device, from the x0 the solver holds: solve, log, x0 <- plant(x0, first control) +
        disturbance, the tracks' auto-advance -- no copy and no synchronisation between ticks (include/tinympc_hip.h,
        tinympc_rollout_batch). Returns a dict of the logs named in `log`: "x" (nx, ticks+1, batch), "u" (nu, ticks, batch), "iter" and
        "status" (ticks, batch) int32, and "gpu_ms", the device time of the whole queue. disturbance: (nx, ticks, batch) or None.
        The device form -- a CUDA torch tensor (batch, ticks, nx) for the disturbance, and / or `out`, a dict of contiguous CUDA tensors
        "x" (batch, ticks+1, nx), "u" (batch, ticks, nu) float64, "iter" / "status" (batch, ticks) int32 (the same memory) -- logs
        into the tensors. With `out` the call returns once the work is queued: order reads behind the solver's stream
        (synchronize()). Without it the tensors are allocated here and the call waits."""
        self._check_setup()
        E = _lib.ERR_INVALID_INPUT
        ticks = int(ticks)
        if ticks < 1:
            raise TinyMPCError(E, "rollout: ticks must be >= 1 (got %d)" % ticks)
        log = tuple(log) if out is None else tuple(out)
        if any(k not in self._ROLLOUT_LOGS for k in log):
            raise TinyMPCError(E, "rollout: logs are named %s, got %s" % (self._ROLLOUT_LOGS, log))
        nx, nu, B = self.nx, self.nu, self.batch
        w_dev = hasattr(disturbance, "data_ptr") and getattr(disturbance, "is_cuda", False)
        if w_dev or out is not None:
            import torch
            shapes = {"x": (B, ticks + 1, nx), "u": (B, ticks, nu), "iter": (B, ticks), "status": (B, ticks)}
            dtypes = {"x": torch.float64, "u": torch.float64, "iter": torch.int32, "status": torch.int32}
            if disturbance is not None and not w_dev:
                raise TinyMPCError(E, "rollout: with out= the disturbance must be a CUDA tensor (or None)")
            if w_dev and (disturbance.dtype != torch.float64 or not disturbance.is_contiguous() or tuple(disturbance.shape) != (B, ticks, nx)):
                raise TinyMPCError(E, "rollout: the disturbance on the device must be a contiguous float64 tensor of shape (%d, %d, %d), got %s %s"
                                   % (B, ticks, nx, disturbance.dtype, tuple(disturbance.shape)))
            own = out is None
            if own:
                out = {k: torch.empty(shapes[k], dtype=dtypes[k], device=disturbance.device) for k in log}
            for k, t in out.items():
                if not (hasattr(t, "data_ptr") and getattr(t, "is_cuda", False)) or t.dtype != dtypes[k] or not t.is_contiguous() or tuple(t.shape) != shapes[k]:
                    raise TinyMPCError(E, "rollout: out[%r] must be a contiguous CUDA %s tensor of shape %s" % (k, dtypes[k], shapes[k]))
            logs = _lib.RolloutLogs(*[out[k].data_ptr() if k in out else None for k in self._ROLLOUT_LOGS])
            for t in list(out.values()) + ([disturbance] if w_dev else []):
                torch.cuda.current_stream(t.device).synchronize()  # (the set_x0_batch contract)
            _lib.check(self._L.tinympc_rollout_batch_device(self._h, ticks, C.c_void_p(disturbance.data_ptr()) if w_dev else None, C.byref(logs)))
            if own:
                self.synchronize()
            return out
        w = None
        if disturbance is not None:
            w = np.asarray(disturbance, dtype=np.float64)
            if w.shape != (nx, ticks, B):
                raise TinyMPCError(E, "rollout: the disturbance must be %d x %d x %d (nx x ticks x batch), got %s" % (nx, ticks, B, w.shape))
            w = _f(w)
        res = {}
        if "x" in log:
            res["x"] = np.zeros((nx, ticks + 1, B), order="F")
        if "u" in log:
            res["u"] = np.zeros((nu, ticks, B), order="F")
        for k in ("iter", "status"):
            if k in log:
                res[k] = np.zeros((ticks, B), dtype=np.int32, order="F")
        logs = _lib.RolloutLogs(*[res[k].ctypes.data if k in res else None for k in self._ROLLOUT_LOGS])
        ms = C.c_float(0.0)
        _lib.check(self._L.tinympc_rollout_batch(self._h, ticks, _p(w) if w is not None else None, C.byref(logs), C.byref(ms)))
        res["gpu_ms"] = float(ms.value)
        return res

    def plant_step(self, disturbance=None):
        """x0 <- plant(x0, first controls of the last solve) + disturbance, on the device (tinympc_plant_step_batch): the rollout's
        plant step on its own. disturbance: (nx, batch) or None."""
        self._check_setup()
        w = None
        if disturbance is not None:
            w = np.asarray(disturbance, dtype=np.float64)
            if w.shape != (self.nx, self.batch):
                raise TinyMPCError(_lib.ERR_INVALID_INPUT, "plant_step: the disturbance must be %d x %d (nx x batch), got %s" % (self.nx, self.batch, w.shape))
            w = _f(w)
        _lib.check(self._L.tinympc_plant_step_batch(self._h, _p(w) if w is not None else None))

    def set_plant_batch(self, A, B, f=None, first: int = 0):
        """A plant that differs from the controller's model, for instances first, first+1, ...: numpy arrays A (nx, nx, count),
        B (nx, nu, count) and, optionally, f (nx, count) -- or contiguous float64 CUDA tensors with the same memory layout, (count, nx, nx)
        holding A_b', (count, nu, nx) holding B_b', (count, nx). The first call names the whole batch. rollout() and plant_step() then
        advance the state with it; the controller is untouched. clear_plant_batch() returns to the model's own plant."""
        self._check_setup()
        nx, nu = self.nx, self.nu
        arrays = [A, B] + ([f] if f is not None else [])
        shapes = [(nx, nx), (nx, nu)] + ([(nx,)] if f is not None else [])
        if any(a is None for a in arrays):
            raise TinyMPCError(_lib.ERR_INVALID_INPUT, "plant: A and B are required")
        on_device = [hasattr(a, "data_ptr") and getattr(a, "is_cuda", False) for a in arrays]
        if any(on_device):
            import torch
            if not all(on_device):
                raise TinyMPCError(_lib.ERR_INVALID_INPUT, "plant: all must be CUDA tensors, or none")
            for a, sh in zip(arrays, shapes):
                if a.dtype != torch.float64 or not a.is_contiguous() or a.dim() != len(sh) + 1 or tuple(a.shape[1:]) != tuple(reversed(sh)):
                    raise TinyMPCError(_lib.ERR_INVALID_INPUT, "plant on the device must be contiguous float64 tensors of shape (count, %s), got %s %s"
                                       % (", ".join(str(d) for d in reversed(sh)), a.dtype, tuple(a.shape)))
            counts = {int(a.shape[0]) for a in arrays}
            ptrs = [C.c_void_p(a.data_ptr()) for a in arrays] + ([None] if f is None else [])
            fn = "tinympc_set_plant_batch_device"
        else:
            arrays = [np.asarray(a, dtype=np.float64) for a in arrays]
            for a, sh in zip(arrays, shapes):
                if a.ndim != len(sh) + 1 or tuple(a.shape[:-1]) != sh:
                    raise TinyMPCError(_lib.ERR_INVALID_INPUT, "plant must be %s x count, got %s" % (" x ".join(str(d) for d in sh), a.shape))
            counts = {int(a.shape[-1]) for a in arrays}
            arrays = [_f(a) for a in arrays]
            ptrs = [_p(a) for a in arrays] + ([None] if f is None else [])
            fn = "tinympc_set_plant_batch"
        if len(counts) != 1:
            raise TinyMPCError(_lib.ERR_INVALID_INPUT, "plant: all must have the same count")
        (count,) = counts
        if on_device[0]:
            torch.cuda.current_stream(arrays[0].device).synchronize()  # (the set_x0_batch contract)
        _lib.check(getattr(self._L, fn)(self._h, *ptrs, int(first), count))

    def clear_plant_batch(self):
        """rollout() and plant_step() advance every instance with the controller's own model again."""
        self._check_setup()
        _lib.check(self._L.tinympc_clear_plant_batch(self._h))

    # ------------------------------------------------------------------ rollout metrics
    _METRICS = ("steps", "cost", "x_violation", "u_violation", "iterations", "max_iterations", "unconverged", "settle")
    _METRICS_FLOAT = ("cost", "x_violation", "u_violation")

    def set_rollout_metrics(self, qx=None, ru=None, settle_tol: float = 0.0):
        """Turn the rollout metrics on (or replace their weights) and zero them: from now on every plant step of rollout() and
        plant_step() scores the instance on the device (include/tinympc_hip.h, tinympc_set_rollout_metrics). qx: (nx,) weights of the
        state error, ru: (nu,) weights of the input error; None: the diagonals of the Q / R given to setup. settle_tol: the state
        counts as away from its reference while max_i |x_i - xr_i| > settle_tol (<= 0: the settle step is not kept)."""
        self._check_setup()
        w = []
        for name, v, M, n in (("qx", qx, self.Q, self.nx), ("ru", ru, self.R, self.nu)):
            a = np.asarray(np.diag(M) if M.ndim == 2 else M, dtype=np.float64) if v is None else np.asarray(v, dtype=np.float64)
            if a.shape != (n,):
                raise TinyMPCError(_lib.ERR_INVALID_INPUT, "rollout metrics: %s must have shape (%d,), got %s" % (name, n, a.shape))
            w.append(np.ascontiguousarray(a))
        if np.ndim(settle_tol) != 0:
            raise TinyMPCError(_lib.ERR_INVALID_INPUT, "rollout metrics: settle_tol must be a scalar")
        score = _lib.RolloutScore(_p(w[0]), _p(w[1]), float(settle_tol))
        _lib.check(self._L.tinympc_set_rollout_metrics(self._h, C.byref(score)))

    def reset_rollout_metrics(self):
        """Zero every instance's metrics, queued on the solver's stream (the weights stay)."""
        self._check_setup()
        _lib.check(self._L.tinympc_reset_rollout_metrics(self._h))

    def clear_rollout_metrics(self):
        """Turn the rollout metrics off: plant steps run the plain kernel again."""
        self._check_setup()
        _lib.check(self._L.tinympc_clear_rollout_metrics(self._h))

    def rollout_metrics(self, device: bool = False):
        """The metrics accumulated since the last reset, a dict of (batch,) arrays: "steps", "cost", "x_violation", "u_violation",
        "iterations", "max_iterations", "unconverged", "settle" (cost and the violations float64, the counts int64); waits for the
        solver's stream. device=True: the rows themselves as a (batch, 8) float64 CUDA tensor view (columns in the order above) of
        memory the solver owns -- no copy and no wait: order reads behind the solver's stream (synchronize())."""
        self._check_setup()
        if device:
            import torch
            ptr = c_double_p()
            _lib.check(self._L.tinympc_get_rollout_metrics_device_ptr(self._h, C.byref(ptr)))

            class _Rows:
                __cuda_array_interface__ = dict(shape=(self.batch, 8), typestr="<f8", data=(C.cast(ptr, C.c_void_p).value, False), version=2)

            return torch.as_tensor(_Rows(), device="cuda")  # (torch takes the device from the pointer)
        rows = np.zeros((self.batch, 8))
        _lib.check(self._L.tinympc_get_rollout_metrics(self._h, _p(rows)))
        return {k: (rows[:, i].copy() if k in self._METRICS_FLOAT else rows[:, i].astype(np.int64)) for i, k in enumerate(self._METRICS)}

    # ------------------------------------------------------------------ rollout noise
    def set_rollout_noise(self, process=None, measurement=None, seed: int = 0, first_instance: int = 0):
        """Turn the rollout noise on (or replace it) and set its tick to 0: from now on every plant step of rollout() and plant_step()
        draws seeded normal noise on the device (include/tinympc_hip.h, tinympc_set_rollout_noise). process / measurement: standard
        deviations per state row, (nx,) shared by the batch or (nx, batch) one column per instance (both given: the same form); None:
        that family is off. Process noise is added to the state the plant carries on; measurement noise only to the state the next
        solve reads (x_log, plant_state() and the metrics keep the true state). seed: 64 bits. first_instance: the global index of this
        solver's instance 0 -- a shard of a fleet draws what the same instances draw unsharded."""
        self._check_setup()
        E = _lib.ERR_INVALID_INPUT
        if process is None and measurement is None:
            raise TinyMPCError(E, "rollout noise: process or measurement is required")
        arrays, forms = [], set()
        for name, v in (("process", process), ("measurement", measurement)):
            if v is None:
                arrays.append(None)
                continue
            a = np.asarray(v, dtype=np.float64)
            if a.shape != (self.nx,) and a.shape != (self.nx, self.batch):
                raise TinyMPCError(E, "rollout noise: %s must have shape (%d,) or (%d, %d), got %s" % (name, self.nx, self.nx, self.batch, a.shape))
            forms.add(a.ndim)
            arrays.append(_f(a) if a.ndim == 2 else np.ascontiguousarray(a))
        if len(forms) != 1:
            raise TinyMPCError(E, "rollout noise: process and measurement must both be (nx,) or both (nx, batch)")
        for name, v in (("seed", seed), ("first_instance", first_instance)):
            if np.ndim(v) != 0 or int(v) != v or not 0 <= int(v) < 2 ** 64:
                raise TinyMPCError(E, "rollout noise: %s must be an integer in [0, 2^64), got %r" % (name, v))
        noise = _lib.RolloutNoise(*[_p(a) if a is not None else None for a in arrays], 1 if forms == {2} else 0, int(seed), int(first_instance))
        _lib.check(self._L.tinympc_set_rollout_noise(self._h, C.byref(noise)))

    def clear_rollout_noise(self):
        """Turn the rollout noise off: plant steps run the plain (or scored) kernel again, from the true state."""
        self._check_setup()
        _lib.check(self._L.tinympc_clear_rollout_noise(self._h))

    def rollout_noise(self, first_tick: int, ticks: int) -> dict:
        """What the plant steps of noise ticks first_tick .. first_tick + ticks - 1 add, regenerated on the device by the steps' own
        draw: {"w": process terms, "v": measurement terms}, each (nx, ticks, batch) as a rollout's disturbance (zeros for a family
        that is off). A noise-free solver given "w" as its disturbance reproduces a process-noise rollout bit for bit."""
        self._check_setup()
        E = _lib.ERR_INVALID_INPUT
        for name, v, lo in (("first_tick", first_tick, 0), ("ticks", ticks, 1)):
            if np.ndim(v) != 0 or int(v) != v or int(v) < lo:
                raise TinyMPCError(E, "rollout_noise: %s must be an integer >= %d, got %r" % (name, lo, v))
        if int(first_tick) + int(ticks) > 2 ** 32:
            raise TinyMPCError(E, "rollout_noise: ticks [%d, %d) reach 2^32" % (int(first_tick), int(first_tick) + int(ticks)))
        w = np.zeros((self.nx, int(ticks), self.batch), order="F")
        v = np.zeros((self.nx, int(ticks), self.batch), order="F")
        _lib.check(self._L.tinympc_get_rollout_noise(self._h, int(first_tick), int(ticks), _p(w), _p(v)))
        return {"w": w, "v": v}

    def plant_state(self) -> np.ndarray:
        """The true state of every instance, (nx, batch): what the plant carries on while measurement noise is on, else x0. Waits for
        the solver's stream."""
        self._check_setup()
        x = np.zeros((self.nx, self.batch), order="F")
        _lib.check(self._L.tinympc_get_plant_state_batch(self._h, _p(x)))
        return x

    def _set_batch(self, what, arrays, rows, full, f_host, f_device, first, *extra):
        """The per-instance verbs: numpy arrays of shape (rows, count) / (rows, cols, count), or contiguous float64 CUDA tensors with the
        same memory layout, (count, rows) / (count, cols, rows) -- one column held over the horizon, or cols = full. All arrays in the
        same form; f(handle, *arrays, *extra, cols, first, count) with cols = 1 or the first array's full column count."""
        on_device = [hasattr(a, "data_ptr") and getattr(a, "is_cuda", False) for a in arrays]
        if any(on_device):
            import torch
            if not all(on_device):
                raise TinyMPCError(_lib.ERR_INVALID_INPUT, "%s: all must be CUDA tensors, or none" % what)
            for a, r, c in zip(arrays, rows, full):
                if a.dtype != torch.float64 or not a.is_contiguous() or a.dim() not in (2, 3) or a.shape[-1] != r or \
                        (a.dim() == 3 and a.shape[1] != c):
                    raise TinyMPCError(_lib.ERR_INVALID_INPUT, "%s on the device must be contiguous float64 tensors of shape "
                                       "(count, %d) or (count, %d, %d), got %s %s" % (what, r, c, r, a.dtype, tuple(a.shape)))
            forms = {(a.dim(), a.shape[0]) for a in arrays}
            ptrs = [C.c_void_p(a.data_ptr()) for a in arrays]
        else:
            arrays = [np.asarray(a, dtype=np.float64) for a in arrays]
            for a, r, c in zip(arrays, rows, full):
                if a.ndim not in (2, 3) or a.shape[0] != r or (a.ndim == 3 and a.shape[1] != c):
                    raise TinyMPCError(_lib.ERR_INVALID_INPUT, "%s must be %d x count or %d x %d x count, got %s" % (what, r, r, c, a.shape))
            forms = {(a.ndim, a.shape[-1]) for a in arrays}
            arrays = [_f(a) for a in arrays]
            ptrs = [_p(a) for a in arrays]
        if len(forms) != 1:
            raise TinyMPCError(_lib.ERR_INVALID_INPUT, "%s: all must have the same form and count" % what)
        (ndim, count), = forms
        cols = 1 if ndim == 2 else full[0]  # (the library checks the range and that device memory is on the handle's GPU)
        if on_device[0]:
            torch.cuda.current_stream(arrays[0].device).synchronize()  # (the set_x0_batch contract)
        _lib.check((f_device if on_device[0] else f_host)(self._h, *ptrs, *extra, cols, first, count))

    def _tick_buffers(self):
        """Persistent buffers of the per-tick verbs (addresses cached: see _lib.fast_tick_functions)."""
        if self._tick is None or self._tick[0].shape != (self.nx, self.batch):
            xb = np.zeros((self.nx, self.batch), order="F")
            ub = np.zeros((self.nu, self.batch), order="F")
            f_session, f_step = _lib.fast_tick_functions()
            self._tick = (xb, ub, xb.ctypes.data, ub.ctypes.data, f_session, f_step)
        return self._tick

    def mpc_step(self, x0s) -> np.ndarray:
        """One closed-loop tick for every instance: measured states in (nx x batch, or an nx-vector for
        batch 1), warm-started solve, first controls out (nu x batch). One call, one synchronisation."""
        self._check_setup()
        xb, ub, xa, ua, _, f_step = self._tick_buffers()
        a = np.asarray(x0s, dtype=np.float64)
        assert a.size == self.nx * self.batch, f"x0s must be {self.nx} x {self.batch}"
        xb[...] = a.reshape(self.nx, self.batch)
        rc = f_step(self._h.value, xa, ua)
        if rc:
            _lib.check(rc)
        return ub.copy(order="F")

    # ------------------------------------------------------------------ closed-loop session (resident kernel)
    def session_begin(self):
        """Launch the solve kernel once and keep it resident: `session_step` then costs no kernel launch and no stream
        synchronisation per tick (include/tinympc_hip.h). Single-instance handles."""
        self._check_setup()
        _lib.check(self._L.tinympc_session_begin(self._h))

    def session_step(self, x0) -> np.ndarray:
        """One tick inside a session: measured state in, warm-started solve, first controls out."""
        self._check_setup()
        xb, ub, xa, ua, f_session, _ = self._tick_buffers()
        a = np.asarray(x0, dtype=np.float64)
        assert a.size == self.nx
        xb[:, 0] = a.reshape(-1)
        rc = f_session(self._h.value, xa, ua)
        if rc:
            _lib.check(rc)
        return ub[:, 0].copy()

    def bench_closed_loop(self, A, B, x0, ticks: int, skip: int = 0, session=False, fdyn=None) -> dict:
        """`ticks` closed-loop ticks driven from C (libtinympc_bench.so: tinympc_bench_closed_loop, include/tinympc_hip_bench.h): what a
        caller written in C pays per tick -- no Python call inside a tick. With session=True the caller has opened the session; session="verbs": the reference's own three verbs per
        tick (set_x0 + solve + get_solution), launched or -- after set_resident(True) -- resident.
        Returns the per-tick durations (us) of the counted ticks (`tick_us`), their mean / median / maximum, the iterations per tick
        and the final state. A measurement helper, not part of the reference class's surface."""
        self._check_setup()
        if not 0 <= int(skip) < int(ticks):
            raise ValueError(f"bench_closed_loop: need 0 <= skip < ticks (got skip={skip}, ticks={ticks})")
        a, b = _f(A), _f(B)
        x = _f(np.asarray(x0, dtype=np.float64).reshape(-1, 1).copy())
        f = _f(np.asarray(fdyn, dtype=np.float64).reshape(-1, 1)) if fdyn is not None else None
        sec, its = C.c_double(0.0), C.c_long(0)
        per = np.zeros(ticks)
        rc = _lib.load_bench_library().tinympc_bench_closed_loop(self._h, self.nx, self.nu, self.N, _p(a), _p(b), _p(f) if f is not None else None, _p(x), int(ticks),
                                                                 int(skip), 2 if session == "verbs" else int(bool(session)), C.byref(sec), C.byref(its), _p(per))
        _lib.check(rc)
        n = ticks - skip
        return dict(us_per_tick=1e6 * sec.value / n, us_per_tick_median=float(np.median(per[skip:])), us_per_tick_max=float(np.max(per[skip:])),
                    iterations_per_tick=its.value / n, x=x.ravel().copy(), tick_us=per[skip:].copy())

    def debug_setup_timing(self) -> dict:
        """Host microseconds of the phases of this handle's setup (tinympc_debug_setup_timing, include/tinympc_hip_bench.h)."""
        self._check_setup()
        out = np.zeros(10)
        _lib.check(self._L.tinympc_debug_setup_timing(self._h, _p(out)))
        return dict(zip(("prologue_us", "device_arena_us", "pinned_arena_us", "stage_and_queue_us", "queue_precompute_us", "wait_us", "total_us",
                         "riccati_loop_clocks", "riccati_loop_us", "riccati_steps"), out))

    def set_resident(self, on: bool = True):
        """Resident solves (tinympc_set_resident): set_x0 / solve / get_solution served by the resident session kernel instead of a
        launch per solve -- bit-identical results, a 2.5x shorter tick. Off by default (include/tinympc_hip.h says why)."""
        self._check_setup()
        _lib.check(self._L.tinympc_set_resident(self._h, int(bool(on))))

    def session_end(self):
        self._check_setup()
        _lib.check(self._L.tinympc_session_end(self._h))

    def reset_workspace(self):
        self._check_setup()
        _lib.check(self._L.tinympc_reset_workspace(self._h))

    def solve_timed(self) -> float:
        """Synchronous solve; returns the kernel duration in ms (HIP events on the handle's stream)."""
        self._check_setup()
        ms = C.c_float()
        _lib.check(self._L.tinympc_solve_timed(self._h, C.byref(ms)))
        return float(ms.value)

    def solve_queued(self):
        """Queue a timed solve on the handle's stream and return at once (tinympc_solve_queued); collect_kernel_ms() waits and
        returns the kernel durations of everything queued since the last collect."""
        self._check_setup()
        _lib.check(self._L.tinympc_solve_queued(self._h))

    def collect_kernel_ms(self) -> list[float]:
        self._check_setup()
        buf = (C.c_float * 4096)()
        n = C.c_int()
        _lib.check(self._L.tinympc_collect_kernel_ms(self._h, buf, 4096, C.byref(n)))
        return [float(buf[i]) for i in range(n.value)]

    def solve_async(self):
        self._check_setup()
        _lib.check(self._L.tinympc_solve_async(self._h))

    def synchronize(self):
        self._check_setup()
        _lib.check(self._L.tinympc_synchronize(self._h))

    def get_solution_batch(self, first: int = 0, count: int | None = None) -> dict:
        self._check_setup()
        count = self.batch - first if count is None else count
        x = np.zeros((self.nx, self.N, count), order="F")
        u = np.zeros((self.nu, self.N - 1, count), order="F")
        _lib.check(self._L.tinympc_get_solution_batch(self._h, _p(x), _p(u), first, count))
        return {"states": x, "controls": u}

    def get_first_controls_batch(self, first: int = 0, count: int | None = None) -> np.ndarray:
        self._check_setup()
        count = self.batch - first if count is None else count
        u0 = np.zeros((self.nu, count), order="F")
        _lib.check(self._L.tinympc_get_first_controls_batch(self._h, _p(u0), first, count))
        return u0

    def get_stats_batch(self, first: int = 0, count: int | None = None) -> dict:
        self._check_setup()
        count = self.batch - first if count is None else count
        it = np.zeros(count, dtype=np.int32)
        st = np.zeros(count, dtype=np.int32)
        res = np.zeros((4, count), order="F")
        _lib.check(self._L.tinympc_get_stats_batch(self._h, it.ctypes.data_as(c_int_p), st.ctypes.data_as(c_int_p),
                                                   _p(res), first, count))
        return dict(iter=it, status=st, residuals=res)

    def get_rho_batch(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """Current rho of every instance (adaptive rho adapts it per instance and keeps it across solves; with per-instance models on,
        the instance's own value -- set_rho_batch)."""
        self._check_setup()
        count = self.batch - first if count is None else count
        rho = np.zeros(count)
        _lib.check(self._L.tinympc_get_rho_batch(self._h, _p(rho), first, count))
        return rho

    def prepare(self):
        """Choose (and, if needed, specialise) the solve kernel for the current constraints / settings now, instead of at the
        first solve that needs it (seconds the first time a shape is seen). It also says that run-time specialisation is welcome on this
        handle: a batch with per-instance models (set_model_batch, before or after this call) then runs on layout D's per-instance
        model form -- nx+nu <= 16, references and bounds constant over the horizon, a horizon that form holds -- instead of layout A,
        and a batch with per-instance linear rows (set_linear_constraints_batch or set_linear_constraints_knots_batch, before or after
        this call) on layout D's per-instance linear-row form under the same conditions (launch_info()["layout"] and jit_info() say which). Per-instance cone slopes
        (set_cone_slopes_batch) are the other half of that mode and run on the same form, whose cone slope is always the instance's;
        cones that share rows stay on layout A. Per-instance reference trajectories and tracks (set_x_ref_batch / set_u_ref_batch with
        a trajectory per instance, set_x_ref_track_batch / set_u_ref_track_batch; before or after this call) run on layout D's
        per-instance trajectory form under the same conditions on shape and bounds, with the shared model and no constraint families.
        Both together -- per-instance rows, rows per knot or cone slopes on per-instance trajectories or tracks -- run on the linear-row
        form that reads every wavefront's own reference rows (jit_info(): "... per-instance-linear per-instance-trajectories"), where rows
        and reference rows fit a wavefront's LDS share together; a trajectory shared by the batch through set_x_ref() / set_u_ref() is not
        one of these and keeps the mode on layout A -- send it through set_x_ref_batch() to stay on layout D. Box bounds per knot and
        per instance (set_bound_constraints_batch with (nx, N, count) / (nu, N-1, count) arrays), with or without per-instance
        trajectories or tracks, run on layout D's per-knot bounds form where the horizon's clamp rows fit a wavefront's LDS share
        (jit_info(): "... per-knot-bounds"; box path, the shared model and rho). The trajectory and per-knot bounds forms run a
        converging batch beyond one resident set with slot refill (jit_info(): "... slot-refill"); where such a form is already the
        handle's, this call builds that variant too."""
        self._check_setup()
        self._push_settings()
        _lib.check(self._L.tinympc_prepare(self._h))

    def launch_info(self) -> dict:
        self._check_setup()
        v = [C.c_int() for _ in range(5)]
        _lib.check(self._L.tinympc_get_launch_info(self._h, *[C.byref(x) for x in v]))
        return dict(lanes_per_instance=v[0].value, instances_per_wave=v[1].value, workgroups=v[2].value,
                    lds_bytes=v[3].value, tables_in_lds=bool(v[4].value), layout=chr(self._L.tinympc_get_layout(self._h)))

    def jit_info(self) -> str:
        """Origin of the kernel of the current configuration: 'compiled-in ...', 'compiled ...', 'disk-cache ...' or
        'refused(<reason>)' (tinympc_get_jit_info). ' slot-refill' where the launch runs layout D's slot-refill variant: the shared
        box path, the goal form (one goal and / or one box per instance), or after prepare() the trajectory and per-knot bounds forms
        (a trajectory, track or bound schedule per instance)."""
        self._check_setup()
        self._push_settings()
        buf = C.create_string_buffer(1024)
        _lib.check(self._L.tinympc_get_jit_info(self._h, buf, len(buf)))
        return buf.value.decode()

    # ------------------------------------------------------------------ private helpers
    def _check_setup(self):
        if not self.is_setup:
            raise TinyMPCError(_lib.ERR_NOT_INITIALIZED, "Solver not setup. Call setup() first.") from None

    def _push_settings(self):
        s = self.settings
        _lib.check(self._L.tinympc_update_settings(
            self._h, float(s["abs_pri_tol"]), float(s["abs_dua_tol"]), int(s["max_iter"]), int(s["check_termination"]),
            int(bool(s["en_state_bound"])), int(bool(s["en_input_bound"])), int(bool(s["en_state_soc"])),
            int(bool(s["en_input_soc"])), int(bool(s["en_state_linear"])), int(bool(s["en_input_linear"])),
            int(bool(s["adaptive_rho"])), float(s["adaptive_rho_min"]), float(s["adaptive_rho_max"]),
            int(bool(s["adaptive_rho_enable_clipping"])), 0))

    @staticmethod
    def _parse_options(defaults: dict, given: dict) -> dict:
        opts = dict(defaults)
        for k, v in given.items():
            if k in opts:  # unknown keys are silently dropped (TinyMPC.m:372)
                opts[k] = v
        return opts

    @staticmethod
    def _mat(a, cols: int) -> np.ndarray:
        a = np.asarray(a, dtype=np.float64)
        if a.size == 0:
            return _f(np.zeros((0, cols)))
        return _f(a.reshape(-1, cols) if a.ndim == 1 else a)

    @staticmethod
    def _expand_bounds(inp, dim: int, horizon: int, default: float) -> np.ndarray:
        """expand_bounds, TinyMPC.m:378-391."""
        if inp is None or (hasattr(inp, "__len__") and np.size(inp) == 0):
            return np.full((dim, horizon), default)
        a = np.asarray(inp, dtype=np.float64)
        if a.ndim == 0 or a.size == 1:
            return np.full((dim, horizon), float(a.reshape(-1)[0]))
        if a.shape == (dim,) or a.shape == (dim, 1) or a.shape == (1, dim):
            return np.repeat(a.reshape(dim, 1), horizon, axis=1)
        return a  # assume the user provides correct dimensions

    @staticmethod
    def _expand_matrix(ref, dim: int, horizon: int) -> np.ndarray:
        """expand_matrix, TinyMPC.m:393-405."""
        a = np.asarray(ref, dtype=np.float64)
        if a.ndim == 0 or a.size == 1:
            return np.full((dim, horizon), float(a.reshape(-1)[0]))
        if a.shape == (dim,) or a.shape == (dim, 1) or a.shape == (1, dim):
            return np.repeat(a.reshape(dim, 1), horizon, axis=1)
        return a
