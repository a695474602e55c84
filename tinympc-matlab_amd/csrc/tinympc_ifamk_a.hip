// tinympc_ifamk_a.hip -- k_admm_solve_ifamk: layout A's solve kernel for a batched handle whose instances have their OWN linear
// (half-space) rows at every KNOT of the horizon (tinympc_set_linear_constraints_knots_batch): a_{k,i}' x_i <= b_{k,i}. The body is
// k_admm_solve_ifam's (tinympc_solve_a_body.h, tinympc_ifam_a.hip) with ONE difference: the families' code takes the knot. The store,
// SolveParams::ilin, holds per wavefront N slots of 3 nl vectors a_k | b_k | 1 / ||a_k||^2 behind the slope vectors, laid out in the
// forward sweep's own skew (k_build_inst_lin_knots): slot 0 is knot 0 on the state lanes -- the call in front of the sweep --, slot i+1
// is what step i finishes, knot i+1 on the state lanes and knot i on the input lanes, so a step reads 3 nl whole 512-byte lines. The
// registers that k_admm_solve_ifam fills once per solve with the first FAM_REG_ROWS rows hold, half each, the first rows of the step's
// slot and of the next step's, fetched one step ahead; rows beyond them are read per use, wide systems walk all of them per use with
// group sums: the same three paths. An instance whose rows are the same at every knot computes exactly what k_admm_solve_ifam computes.
#include "tinympc_solve_a.h"

namespace tinympc {

// A wave-uniform kernel argument given a vector register as its home (the empty asm makes it opaque, hence per lane, to the compiler).
#define TINY_VGPR_HOME(x) asm volatile("" : "+v"(x))

template <int W, int KT, bool TLDS, bool GMEM>
__global__ void __launch_bounds__(64) k_admm_solve_ifamk(const SolveParams p_) {
    constexpr SolveExt E = SolveExt::InstFamiliesKnots;
    // 16 lanes per instance: the arguments' pointers live in vector registers from the start, as in k_admm_solve_ifam (see there)
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
template hipError_t launch_solve_a_e<SolveExt::InstFamiliesKnots>(const SolveParams &, int, int, size_t, hipStream_t);

}  // namespace tinympc
