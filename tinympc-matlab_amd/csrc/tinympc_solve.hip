// tinympc_solve.hip -- k_admm_solve: the whole TinyMPC solve() as ONE persistent kernel (gfx950, FP64); layout A's box path.
// Layout A has two more variants of the same kernel, which share its body (tinympc_solve_a_body.h) and its launcher
// (tinympc_solve_a.h): k_admm_solve_fam (tinympc_solve_fam.hip, the cone / linear slack families) and k_admm_solve_adapt
// (tinympc_solve_adapt.hip, adaptive rho). A fourth, k_admm_solve_iref (below), carries per-instance references, and a fifth,
// k_admm_solve_ibnd, per-instance bounds as well.
//
//   M1 solve                 admm.cpp:109-207      F1 forward_pass          admm.cpp:25-35
//   S1 update_slack          admm.cpp:43-59        D1 update_dual           admm.cpp:65-69
//   L1 update_linear_cost    admm.cpp:75-83        R1 termination_condition admm.cpp:89-107
//   C1 v/z copies            admm.cpp:196-197      B1 backward_pass_grad    admm.cpp:13-20
//
// Design (DESIGN.md has the full rationale and the measurements behind each choice):
//   * one wavefront = 64/W MPC instances, W lanes per instance, one lane per state/input row;
//   * the ADMM state that survives an iteration (duals g|y, slack v|z, feed-forward d) lives in LDS
//     for the whole solve: HBM is touched once at entry and once at exit (plus the stale-v stream, below);
//   * each sweep step is ONE (nx+nu)x(nx+nu) mat-vec per instance: the operand vector is spread over
//     the W lanes of the instance and broadcast with DPP row_newbcast fused into v_fmac_f64 (W=16),
//     so a step is KT FP64 FMAs per lane and no LDS round trip sits on the dependency chain;
//   * slack projection, dual ascent, linear-cost refresh and the four inf-norm residuals are row-local,
//     so they are fused into the forward sweep, lane by lane, right after the lane's row of
//     x_{i+1} / u_i has been produced; their LDS operands are prefetched one step ahead;
//   * a lone wavefront issues at most one VALU instruction every ~4 cycles (8 for FP64), so the kernel
//     is instruction-issue bound. The sweep bodies are therefore branch-free (lanes that must not store
//     write to a per-lane dummy row instead of being masked off), address arithmetic is reduced to
//     pointer increments (arrays carry a padding row at each end so the prefetch needs no clamping),
//     the sweeps are unrolled by two so that the prefetch registers ping-pong without moves, and the
//     FMA chain and the row-local math are single asm blocks (no per-statement hazard padding).
//
#include "tinympc_solve_a.h"

namespace tinympc {

// LDS plan per workgroup (= one wavefront), in doubles:
//   G[N+2][64]  V[N+2][64]   row k+1 = knot k. Row 0 and row N+1 are padding touched by the one-step-
//                            ahead prefetch at the ends of a sweep; row N+1 doubles as the per-lane
//                            dummy slot that lanes which must not store (converged instance, padding
//                            lanes) write to, so the sweeps need no exec masking.
//   D[(N-1)*IPW*nu + 64]     feed-forward term, compact; the last 64 are dummy / overshoot slots
//   tables (optional)        lo | hi | linref [N+2][W], pNref[W]
size_t solve_lds_bytes(int nx, int nu, int N, int W, bool tables_in_lds) {
    const int ipw = 64 / W;
    size_t d = (size_t)2 * (N + 2) * 64 + (size_t)(N - 1) * ipw * nu + 64;
    d = (d + 1) & ~(size_t)1;
    if (tables_in_lds) d += tables_doubles(W, N);
    (void)nx;
    return d * sizeof(double);
}

bool choose_geometry(int nx, int nu, int *W, int *KT) {
    const int nxu = nx + nu;
    if (nx < 1 || nu < 1 || nxu > 64) return false;
    if (nxu <= 8) { *W = 16; *KT = 8; }
    else if (nxu <= 12) { *W = 16; *KT = 12; }
    else if (nxu <= 16) { *W = 16; *KT = 16; }
    else if (nxu <= 32) { *W = 32; *KT = 32; }
    else { *W = 64; *KT = 64; }
    return true;
}

// GMEM: the working copy of the state lives in p.scratch (HBM) instead of LDS -- the fallback for horizons
// that do not fit 160 KB of LDS. Same code, same results; the row-local operands then come from L2.
template <int W, int KT, bool TLDS, bool GMEM>
__global__ void __launch_bounds__(64) k_admm_solve(const SolveParams p) {
    constexpr SolveExt E = SolveExt::Box;
#include "tinympc_solve_a_body.h"
}
template hipError_t launch_solve_a_e<SolveExt::Box>(const SolveParams &, int, int, size_t, hipStream_t);

// k_admm_solve_iref: the box path for a batched handle whose instances track their OWN references (tinympc_set_x_ref_batch /
// _u_ref_batch). The only difference is where the reference-dependent operands come from: the backward sweep streams the instance's
// linref rows -(Xref .* Q) | -(Uref .* R) from SolveParams::iref_lr, one 512-byte line per knot and wavefront (the lanes' order is the
// kernel's own), and pNref comes from iref_pn. Both are built by k_build_inst_tables with k_build_tables' expressions, so an instance
// whose references are the shared ones computes exactly what k_admm_solve computes. Bounds stay the shared tables (LDS or L2).
template <int W, int KT, bool TLDS, bool GMEM>
__global__ void __launch_bounds__(64) k_admm_solve_iref(const SolveParams p) {
    constexpr SolveExt E = SolveExt::InstRefs;
#include "tinympc_solve_a_body.h"
}
template hipError_t launch_solve_a_e<SolveExt::InstRefs>(const SolveParams &, int, int, size_t, hipStream_t);

// k_admm_solve_ibnd: k_admm_solve_iref for a batched handle whose instances also have their OWN bounds (tinympc_set_bound_constraints_batch).
// The forward sweep streams the instance's clamp rows lo | hi from SolveParams::ibnd (k_build_inst_tables, k_build_tables' expressions)
// four knots ahead, as the backward sweep streams the linref rows; an instance whose bounds and references are the shared ones computes
// exactly what k_admm_solve computes.
template <int W, int KT, bool TLDS, bool GMEM>
__global__ void __launch_bounds__(64) k_admm_solve_ibnd(const SolveParams p) {
    constexpr SolveExt E = SolveExt::InstBounds;
#include "tinympc_solve_a_body.h"
}
template hipError_t launch_solve_a_e<SolveExt::InstBounds>(const SolveParams &, int, int, size_t, hipStream_t);

hipError_t launch_solve_a(const SolveParams &p, SolveExt ext, int W, int KT, size_t lds_bytes, hipStream_t stream) {
    switch (ext) {
        case SolveExt::Box: return launch_solve_a_e<SolveExt::Box>(p, W, KT, lds_bytes, stream);
        case SolveExt::Families: return launch_solve_a_e<SolveExt::Families>(p, W, KT, lds_bytes, stream);
        case SolveExt::Adaptive:
            if (!p.adapt || !p.rho_inst) return hipErrorInvalidValue;
            return launch_solve_a_e<SolveExt::Adaptive>(p, W, KT, lds_bytes, stream);
        case SolveExt::InstRefs:
            if (!p.iref_lr || !p.iref_pn) return hipErrorInvalidValue;
            return launch_solve_a_e<SolveExt::InstRefs>(p, W, KT, lds_bytes, stream);
        case SolveExt::InstBounds:
            if (!p.iref_lr || !p.iref_pn || !p.ibnd) return hipErrorInvalidValue;
            return launch_solve_a_e<SolveExt::InstBounds>(p, W, KT, lds_bytes, stream);
        case SolveExt::InstModels:
            if (!p.iref_lr || !p.iref_pn || !p.ibnd) return hipErrorInvalidValue;
            return launch_solve_a_e<SolveExt::InstModels>(p, W, KT, lds_bytes, stream);
        case SolveExt::InstFamilies:
            if (!p.iref_lr || !p.iref_pn || !p.ibnd || !p.ilin || !p.fam) return hipErrorInvalidValue;
            return launch_solve_a_e<SolveExt::InstFamilies>(p, W, KT, lds_bytes, stream);
        case SolveExt::InstFamiliesKnots:
            if (!p.iref_lr || !p.iref_pn || !p.ibnd || !p.ilin || !p.fam || p.ilin_knots != p.N) return hipErrorInvalidValue;
            return launch_solve_a_e<SolveExt::InstFamiliesKnots>(p, W, KT, lds_bytes, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace tinympc
