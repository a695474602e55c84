// tinympc_ifam_a.hip -- k_admm_solve_ifam: layout A's solve kernel for a batched handle whose instances have their OWN linear
// (half-space) rows (tinympc_set_linear_constraints_batch). The body is k_admm_solve's (tinympc_solve_a_body.h), in the form of
// k_admm_solve_fam -- the cone / linear slack families with their duals and linear-cost term in HBM -- on the per-instance rows of
// k_admm_solve_ibnd (every instance's linref rows, pNref and clamp rows streamed from the per-instance tables), plus ONE difference: a
// lane reads the linear rows' a_k | b_k | ||a_k||^2 from its instance's vectors in SolveParams::ilin, [group][3 nl][64]
// (k_build_inst_lin), instead of the shared description's. The first FAM_REG_ROWS rows stay in registers for the whole solve, the rest
// is read per use, wide systems walk all of them per use with group sums: k_admm_solve_fam's three paths. Cones, enable flags and
// rounds come from the shared description. An instance whose rows are the shared ones computes exactly what k_admm_solve_fam computes.
#include "tinympc_solve_a.h"

namespace tinympc {

// A wave-uniform kernel argument given a vector register as its home (the empty asm makes it opaque, hence per lane, to the compiler).
#define TINY_VGPR_HOME(x) asm volatile("" : "+v"(x))

template <int W, int KT, bool TLDS, bool GMEM>
__global__ void __launch_bounds__(64) k_admm_solve_ifam(const SolveParams p_) {
    constexpr SolveExt E = SolveExt::InstFamilies;
    // 16 lanes per instance: the families' body keeps more wave-uniform values alive through the ADMM loop than there are scalar
    // registers -- k_admm_solve_fam parks 36-50 of them in the lanes of a vector register, this variant, with the per-instance rows'
    // pointers on top, parked 42-59. Nearly all of them are the arguments' pointers, which only ever enter per-lane addresses: here
    // they live in vector registers from the start (one pair each, 366-508 VGPRs in all), and nothing is spilled, scalar or vector.
    // What the loops' control flow reads (N, max_iter, check_termination, the families' description) stays scalar. The wider forms
    // have no vector registers to spare for this (the 64-lane form went to scratch) and keep their 59-83 parked scalars.
    SolveParams p = p_;
    if constexpr (W == 16) {
        TINY_VGPR_HOME(p.G); TINY_VGPR_HOME(p.V); TINY_VGPR_HOME(p.GC); TINY_VGPR_HOME(p.GL); TINY_VGPR_HOME(p.LX); TINY_VGPR_HOME(p.D);
        TINY_VGPR_HOME(p.sol_x); TINY_VGPR_HOME(p.sol_u); TINY_VGPR_HOME(p.istats); TINY_VGPR_HOME(p.dstats);
        TINY_VGPR_HOME(p.iref_lr); TINY_VGPR_HOME(p.iref_pn); TINY_VGPR_HOME(p.ibnd); TINY_VGPR_HOME(p.ilin); TINY_VGPR_HOME(p.x0);
        TINY_VGPR_HOME(p.rho); TINY_VGPR_HOME(p.abs_pri_tol); TINY_VGPR_HOME(p.abs_dua_tol); TINY_VGPR_HOME(p.ops);
        TINY_VGPR_HOME(p.u0_host); TINY_VGPR_HOME(p.host_sol); TINY_VGPR_HOME(p.x0_mirror);
        TINY_VGPR_HOME(p.scratch); TINY_VGPR_HOME(p.tables);
        TINY_VGPR_HOME(p.groups); TINY_VGPR_HOME(p.batch); TINY_VGPR_HOME(p.scratch_stride);
    }
#include "tinympc_solve_a_body.h"
}
template hipError_t launch_solve_a_e<SolveExt::InstFamilies>(const SolveParams &, int, int, size_t, hipStream_t);

}  // namespace tinympc
