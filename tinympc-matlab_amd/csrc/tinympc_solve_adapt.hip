// tinympc_solve_adapt.hip -- k_admm_solve_adapt: the solve loop with adaptive rho. The body is
// k_admm_solve's (tinympc_solve_a_body.h); what adaptive rho adds:
//
// admm.cpp:117-174            every 5th iteration (i > 0 && i % 5 == 0), after update_linear_cost and before
//                             the termination test: benchmark_rho_adaptation + Taylor update of the cache
// rho_benchmark.cpp:44-150    format_matrices   -- the reference assembles a dense KKT-style system
// rho_benchmark.cpp:152-180   compute_residuals -- four inf-norms of dense mat-vecs with it
// rho_benchmark.cpp:182-198   predict_rho       -- rho * sqrt(normalised primal / normalised dual), clipped
// rho_benchmark.cpp:200-216   update_matrices_with_derivatives -- Kinf, Pinf (C1, C2) += d_rho * sensitivities
//   * rho is PER INSTANCE (each instance of a batch adapts on its own) and persists across solves in p.rho_inst,
//     like the reference's cache->rho. The reference's cache is then K0 + (rho - rho0) dK, P0 + (rho - rho0) dP, so
//     the lane's rows of the two sweep operators are rebuilt from (base row) + (rho - rho0) * (derivative row) after
//     every adaptation (tables: k_build_adapt, tinympc_kernels.hip) -- no per-instance matrices are stored anywhere;
//   * the dense system is never formed. With x_decision = [x_0; u_0; x_1; ...] its rows/columns are knots, so the
//     four norms are row-local maxima that ride on the forward sweep of an adaptation iteration, plus ONE extra
//     mat-vec per step, [A'; B'] g_{i+1} (the A_matrix' * y_vector term), and one Pinf * x_{N-1} at the end:
//        primal rows     u_i - znew_i                    |  (A x_i + B u_i - x_{i+1}) - vnew_{i+1}
//        dual cols x_i   2 Q.*x_i + A' g_{i+1} - g_i     |  x_0: no -g_0 ; x_{N-1}: Pinf x + Q.*x - g_{N-1}
//        dual cols u_i   2 R.*u_i + y_i + B' g_{i+1}
//     The dynamics defect A x_i + B u_i - x_{i+1} is taken as exactly 0 (x_{i+1} was just computed as that sum;
//     the reference's dense product differs from it by rounding only, ~1e-16 relative to the norms it enters).
//   * the linear-cost terms of the iteration were formed with the OLD rho and Pinf (update_linear_cost runs before
//     the adaptation), the termination test and the backward pass use the NEW rho and Kinf: the backward sweep of
//     an adaptation iteration therefore takes rho / p_N's reference term from before the update.
//   Not adapted: Quu_inv and AmBKt (the reference updates the copies C1 / C2, which no solve phase reads) and the
//   affine-dynamics constants APf / BPf (not in the snapshot).
#include "tinympc_solve_a.h"

namespace tinympc {

template <int W, int KT, bool TLDS, bool GMEM>
__global__ void __launch_bounds__(64) k_admm_solve_adapt(const SolveParams p) {
    constexpr SolveExt E = SolveExt::Adaptive;
#include "tinympc_solve_a_body.h"
}
template hipError_t launch_solve_a_e<SolveExt::Adaptive>(const SolveParams &, int, int, size_t, hipStream_t);

}  // namespace tinympc
