// tinympc_solve_fam.hip -- k_admm_solve_fam: layout-A solve kernel + the second-order-cone and linear-inequality slack
// families (BASELINE config 4). The body is k_admm_solve's (tinympc_solve_a_body.h).
//
// PARITY UNPINNED. The reference tree has no source for these families (they live in the newer
// TinyMPC/TinyMPC core behind the calls at /root/reference/src/bindings.cpp:408-478); this variant implements the same
// restatement of the upstream algorithm as the CPU checker under oracle/ and is tested against it and against first principles
// (cone / half-space feasibility). On top of the box family (g|y, v|z -- as in k_admm_solve, in LDS) every row carries
//   cone family    dual gc|yc, slack vcnew|zcnew = projection of (x|u) + (gc|yc) onto the row's cone
//                  { (w, t) : ||w||_2 <= mu * t } (rows in no cone are left as they are);
//   linear family  dual gl|yl, slack vlnew|zlnew = (x|u) + (gl|yl) pushed through the half-spaces
//                  a_k' s <= b_k one after another;
// the slacks are transient, the duals persist (HBM, prefetched one step ahead), and the linear cost gets
//   q_i (r_i) -= rho * (vcnew - gc) + rho * (vlnew - gl)      ("Lx", stored in HBM, forward -> backward).
// Termination still looks at the box family only, as upstream does.
// Cross-row quantities reuse the fused DPP mat-vec with 0/1 mask rows instead of a shuffle butterfly:
//   ||w||^2 = Cn_row . s.^2     t = Ct_row . s     a_k' s = Ty_row . (a_k .* s)
// so any number of pairwise-disjoint cones costs two mat-vecs per step, and each linear row one.
//
#include "tinympc_solve_a.h"

namespace tinympc {

template <int W, int KT, bool TLDS, bool GMEM>
__global__ void __launch_bounds__(64) k_admm_solve_fam(const SolveParams p) {
    constexpr SolveExt E = SolveExt::Families;
#include "tinympc_solve_a_body.h"
}
template hipError_t launch_solve_a_e<SolveExt::Families>(const SolveParams &, int, int, size_t, hipStream_t);

}  // namespace tinympc
