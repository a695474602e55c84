// tinympc_imod_a.hip -- k_admm_solve_imod: layout A's solve kernel for a batched handle whose instances have their OWN models
// (tinympc_set_model_batch: A, B, fdyn, Q, R per instance). The body is k_admm_solve's (tinympc_solve_a_body.h), in the form of
// k_admm_solve_ibnd -- every instance's linref rows, pNref and clamp rows streamed from the per-instance tables, which
// k_build_inst_tables builds from the instance's own Pinf and cost diagonals -- plus ONE difference: a lane loads its two operator rows
// and its constants cf | cb from its instance's block of SolveParams::ops, [batch][ops_doubles(W, KT)] (k_build_operators over the
// instances), instead of the one shared block. They stay in registers for the whole solve, as always: the ADMM loop is InstBounds' loop.
// An instance whose model is the shared one computes exactly what k_admm_solve computes.
#include "tinympc_solve_a.h"

namespace tinympc {

template <int W, int KT, bool TLDS, bool GMEM>
__global__ void __launch_bounds__(64) k_admm_solve_imod(const SolveParams p) {
    constexpr SolveExt E = SolveExt::InstModels;
#include "tinympc_solve_a_body.h"
}
template hipError_t launch_solve_a_e<SolveExt::InstModels>(const SolveParams &, int, int, size_t, hipStream_t);

}  // namespace tinympc
