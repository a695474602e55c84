"""Systems whose precompute inverse swaps rows, and the plain reference they are checked against (no GPU import).

Every Riccati step of the LQR precompute (tiny_api.cpp:124-190) inverts S = R1 + B'PB with partial pivoting, in five implementations:
rows_inverse (tinympc_precompute_rows.hip), wg_lu_inverse (tinympc_kernels.hip: k_precompute, k_lqr), k_lu_inverse and k_gain_solve
(tinympc_precompute_large.hip) and lu_inverse (oracle/tinympc_oracle.c). Every other system of the suite gives an S whose largest
entry of each column sits on the diagonal, in every step (docs/NOTEBOOK.md, "Pivot swaps in the precompute inverse"): no row swap,
no permutation, no cross-lane fetch ever ran. swap_system() below makes them run: input columns of unequal length that share a
direction, under a small R, so that an off-diagonal entry of a column of S exceeds its diagonal one.

Holds: the generator, the case table, a numpy restatement of the precompute that records the pivots of every S it inverts, and the
inputs of the short solve the GPU tests run on these caches. tests/test_pivot_swap_cpu.py checks that the inputs do what they are
for, tests/test_pivot_swap_gpu.py runs the kernels on them."""
from __future__ import annotations

import numpy as np


def swap_system(P, nx, nu, N, corr=0.7, spread=0.6, rlo=0.1, rhi=0.2, rho=0.1, seed=None):
    """`seed`: the per-instance seed of a batched handle's models (default: the shape's own)."""
    rng = np.random.default_rng(nx * 100 + nu if seed is None else seed)
    A = 0.85 * np.eye(nx) + (0.1 / np.sqrt(nx)) * rng.standard_normal((nx, nx))
    b0 = rng.standard_normal(nx) / np.sqrt(nx)
    scale = 1.0 + spread * rng.permutation(nu)            # input columns of unequal, shuffled length
    j = int(np.argmin(scale)); scale[0], scale[j] = scale[j], scale[0]   # column 0 is the shortest
    G = rng.standard_normal((nx, nu)) / np.sqrt(nx)
    B = (corr * b0[:, None] + (1 - corr) * G) * scale[None, :]           # a shared direction: correlated columns
    return P.Problem("swap", A, B, np.diag(rng.uniform(1, 10, nx)), np.diag(rng.uniform(rlo, rhi, nu)), N, rho, rng.standard_normal(nx))


# name -> (nx, nu, kernel form). The smallest shapes that reach each form of the inverse.
CASES = {
    "rows4x2": (4, 2, "rows"),      # class (4,4): two padded rows
    "rows6x3": (6, 3, "rows"),      # its exact class
    "rows8x4": (8, 4, "rows"),      # exact class (8,4)
    "rows12x4": (12, 4, "rows"),    # exact class (12,4)
    "lds13x2": (13, 2, "lds"),      # k_precompute, working set in LDS: nx beyond the rows kernel
    "lds6x5": (6, 5, "lds"),        # ... nu beyond it
    "lds20x6": (20, 6, "lds"),
    "global48x16": (48, 16, "global"),  # k_precompute, working set beyond LDS: global scratch
    "large66x6": (66, 6, "large"),      # layout M, k_lu_inverse (one wavefront, LDS)
    "large70x14": (70, 14, "large"),
    "gain80x66": (80, 66, "gain"),      # layout M, nu > 64: k_gain_solve
}
FORMS = ("rows", "lds", "global", "large", "gain")


def layout_m(name):
    return CASES[name][2] in ("large", "gain")


def problem(P, name):
    """The case's system with the horizon of its short solve: N = 6, layout M N = 4; nu > 64: corr = 0.5, spread = 0.1."""
    nx, nu, _ = CASES[name]
    N = 4 if layout_m(name) else 6
    return swap_system(P, nx, nu, N, corr=0.5, spread=0.1) if nu > 64 else swap_system(P, nx, nu, N)


def rows_class(nx, nu):
    """(NXP, NUP) of the k_precompute_rows instantiation that takes (nx, nu): launch_precompute_rows, restated."""
    if (nx, nu) in ((4, 1), (6, 3)):
        return nx, nu
    return (4 if nx <= 4 else 8 if nx <= 8 else 12), 4


def pivots(S):
    """Partial-pivot LU of S (largest magnitude, first of equals -- Eigen's PartialPivLU, every kernel's rule): per column k the
    POSITION of its pivot among the rows as they stand after the earlier swaps (!= k: the `if (piv != k)` branch runs), and the index
    that row had in S."""
    lu = np.array(S, dtype=np.float64)
    n = lu.shape[0]
    orig = np.arange(n)
    pos = np.zeros(n, dtype=np.int64)
    src = np.zeros(n, dtype=np.int64)
    for k in range(n):
        piv = k + int(np.argmax(np.abs(lu[k:, k])))  # (argmax: the first of equals)
        pos[k] = piv
        if piv != k:
            lu[[k, piv], :] = lu[[piv, k], :]
            orig[[k, piv]] = orig[[piv, k]]
        src[k] = orig[k]
        lu[k + 1:, k] /= lu[k, k]
        lu[k + 1:, k + 1:] -= np.outer(lu[k + 1:, k], lu[k, k + 1:])
    return pos, src


def swaps(pos):
    return int(np.sum(np.asarray(pos) != np.arange(len(pos))))


def riccati(prob):
    """tiny_api.cpp:124-190 in numpy: the diagonals of Q and R augmented by rho twice (:90-91, :134-135), P0 = rho I (:148),
    K = solve(S, B'PA) (:154), P = Q1 + A'P(A - BK) (:155), stop at max|K - Kprev| < 1e-5 keeping THAT step's K and P (:157);
    Quu_inv and AmBKt from them (:169-170). Also what the swap counter saw: `pivots` (per step: positions), `final` (positions,
    original rows) for the S of Quu_inv, that S itself, and the stopping differences of every step."""
    A, B = np.asarray(prob.A, dtype=np.float64), np.asarray(prob.B, dtype=np.float64)
    nx, nu = B.shape
    Q1 = np.diag(np.diag(prob.Q) + 2.0 * prob.rho)
    R1 = np.diag(np.diag(prob.R) + 2.0 * prob.rho)
    Pm = prob.rho * np.eye(nx)
    Kprev = np.zeros((nu, nx))
    piv, diffs = [], []
    K = Pn = None
    for _ in range(1000):
        S = R1 + B.T @ Pm @ B
        piv.append(pivots(S)[0])
        K = np.linalg.solve(S, B.T @ Pm @ A)
        Pn = Q1 + A.T @ Pm @ (A - B @ K)
        diffs.append(float(np.max(np.abs(K - Kprev))))
        if diffs[-1] < 1e-5:
            break
        Kprev, Pm = K, Pn
    S = R1 + B.T @ Pn @ B
    return dict(Kinf=K, Pinf=Pn, Quu_inv=np.linalg.inv(S), AmBKt=(A - B @ K).T, riccati_iters=len(diffs), diffs=diffs, pivots=piv,
                final=pivots(S), S=S)


def solve_inputs(prob, batch, Kinf):
    """The short solve on a case's cache: x0s (nx, batch) of graded size, and input bounds at +-0.3 of the scale of the unconstrained
    first control -Kinf x0 (its largest entry over the batch), so that the clamp is active; states unbounded. max_iter = 15 with zero
    tolerances: every instance runs all fifteen iterations."""
    rng = np.random.default_rng(prob.nx * 100 + prob.nu + 7)
    x0s = np.asfortranarray(rng.standard_normal((prob.nx, batch)) * np.linspace(0.4, 1.0, batch)[None, :])
    ulim = 0.3 * float(np.max(np.abs(Kinf @ x0s)))
    return x0s, ulim


SOLVE_SETTINGS = dict(max_iter=15, abs_pri_tol=0.0, abs_dua_tol=0.0)


def solve_problem(P, name, Kinf):
    """-> (problem with the input bounds installed, x0s): batch 5, layout M 17 (one ragged tile of 16 + 1)."""
    prob = problem(P, name)
    x0s, ulim = solve_inputs(prob, 17 if layout_m(name) else 5, Kinf)
    prob.u_min, prob.u_max = np.full(prob.nu, -ulim), np.full(prob.nu, ulim)
    return prob, x0s


# ---- the systems the suite had before (restated; a test imports nothing from GPU test modules) ----
def tame_rows_system(P, nx, nu):
    """test_hip_parity.py::test_register_resident_precompute_on_every_shape_class"""
    rng = np.random.default_rng(100 * nx + nu)
    A = 0.92 * np.eye(nx) + (0.25 / np.sqrt(nx)) * rng.standard_normal((nx, nx))
    B = 0.3 * rng.standard_normal((nx, nu))
    Q, R = np.diag(rng.uniform(0.5, 20.0, nx)), np.diag(rng.uniform(0.2, 4.0, nu))
    return P.Problem("rows", A, B, Q, R, 8, float(rng.uniform(0.3, 6.0)), rng.standard_normal(nx))


def tame_large_system(P, nx, nu, N, seed):
    """test_large_systems_gpu.py::_system"""
    rng = np.random.default_rng(seed)
    A = np.eye(nx) * 0.98 + 0.015 * rng.standard_normal((nx, nx))
    B = 0.08 * rng.standard_normal((nx, nu))
    return P.Problem("large", A, B, np.diag(rng.uniform(1, 10, nx)), np.diag(rng.uniform(0.5, 2, nu)), N, 2.0, rng.standard_normal(nx))


def tame_models(prob, batch, seed=1):
    """test_instance_models_gpu.py::_models: seeded perturbations of `prob` -> A, B, Q, R of shape (.., .., batch)."""
    rng = np.random.default_rng(1000 + seed)
    nx, nu = prob.nx, prob.nu
    A = prob.A[:, :, None] + 1e-2 * rng.uniform(-1.0, 1.0, (nx, nx, batch))
    B = prob.B[:, :, None] * rng.uniform(0.85, 1.15, (nx, nu, batch))
    Q = np.zeros((nx, nx, batch))
    R = np.zeros((nu, nu, batch))
    Q[np.arange(nx), np.arange(nx), :] = np.diag(prob.Q)[:, None] * rng.uniform(0.85, 1.15, (nx, batch))
    R[np.arange(nu), np.arange(nu), :] = np.diag(prob.R)[:, None] * rng.uniform(0.85, 1.15, (nu, batch))
    return A, B, Q, R


def mixed_models(P, nx, nu, N, batch):
    """A batched handle's models: odd instances swap systems with seeds of their own, even instances the tame perturbations of a tame
    base system (the handle's own model) -> (base problem, A, B, Q, R of shape (.., .., batch), the instance problems)."""
    base = tame_rows_system(P, nx, nu)
    base.N = N
    base.rho = 0.1  # (rho stays the handle's: the swap systems' value)
    A, B, Q, R = tame_models(base, batch)
    probs = []
    for b in range(batch):
        if b % 2:
            sw = swap_system(P, nx, nu, N, seed=7000 + 100 * nx + 10 * nu + b)
            A[:, :, b], B[:, :, b], Q[:, :, b], R[:, :, b] = sw.A, sw.B, sw.Q, sw.R
        probs.append(P.Problem("mixed", A[:, :, b].copy(), B[:, :, b].copy(), Q[:, :, b].copy(), R[:, :, b].copy(), N, base.rho, base.x0))
    return base, A, B, Q, R, probs
